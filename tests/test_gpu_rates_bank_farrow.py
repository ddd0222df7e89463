"""GPU tests of per-channel taps with per-channel rates for FIRFarrow (the BANK kernels of csrc/kernels_rates_farrow.hip): mrhip_set_channel_taps_farrow
and mrhip_set_channel_pnfb on a filter of mrhip_create_farrow_rates*, FIRFilter.set_channel_taps_farrow(H), FIRFilter.set_channel_pnfb(PN)
and FIRFilter.per_channel_taps_and_rates_farrow(H, rates, Nphi, polyorder) -- one FIRFilter(H[c], rates[c], Nphi, polyorder) per channel
behind one filter object.

Bar (include/multirate_hip.h, "Per-channel taps with per-channel rates for FIRFarrow"): for every channel c the outputs and the count of
every call, the end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx) and the history are BIT FOR BIT those of the oracle's
O.FIRFilter(H[c], rates[c], Nphi, tx=tx, polyorder=P, pnfb=fit of H[c]) fed x[c] -- under STRICT and FUSED, on the universal kernel
(reported as farrow_rates_bank_generic, MRHIP_FORCE_GENERIC=1) and on the multi kernel (farrow_rates_bank_multi,
MRHIP_FARROW_RATES_BANK_MULTI=1).  No tolerance anywhere.  The rows of H are all different and so are the rows of x: channels of equal
rate no longer give equal rows, and a kernel that reads the wrong bank fails.  The shapes are those of tests/test_gpu_rates_farrow.py, the
smallest at which these kernels can go wrong.  The module also holds the write-only-own-outputs cases of the two kernels (poisoned
buffers of tests/output_bounds_cases.py, a checker per row).
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, POISON, make_buffer, row_pad
from test_gpu_rates_bank_arb import RAGGED
from test_gpu_rates_farrow import (CASES, CHUNKINGS, R1, R3, R4, R67, SHAPES, X_LENS, X_LENS_MULTI, _assert_rows_only_written, _check_end, _chunks, _fit,
                                   _state5, _tt)

pytestmark = pytest.mark.gpu

GENERIC, MULTI = "farrow_rates_bank_generic", "farrow_rates_bank_multi"
SHARED = {False: "farrow_rates_generic", True: "farrow_rates_multi"}
assert {(s, t) for s, t in CASES if s != (32, 250, 4)} == {(s, t) for s in SHAPES for t in ((np.float32, np.float32), (np.float64, np.complex64))}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


_SIGNALS = {}


def _signal(seed, Nphi, hLen, x_len, th, tx, nch):
    """one tap vector per channel (about unit gain per phase), all different, and one row of samples per channel, all different"""
    key = (seed, Nphi, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, nch)
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        H = (rng.standard_normal((nch, hLen)) * Nphi / max(hLen, 1)).astype(th)
        x = rng.random((nch, x_len)) - 0.5
        if np.dtype(tx).kind == "c":
            x = x + 1j * (rng.random((nch, x_len)) - 0.5)
        x = x.astype(tx)
        assert len({H[c].tobytes() for c in range(nch)}) == nch
        assert x_len == 0 or len({x[c].tobytes() for c in range(nch)}) == nch
        H.setflags(write=False), x.setflags(write=False)
        _SIGNALS[key] = (H, x)
    return _SIGNALS[key]


def _oracle(pkg, O, h, rate, Nphi, P, tx, pnfb=None):
    """the reference of one channel: the oracle's FIRFilter(h, rate, Nphi, polyorder = P) on the library's per-row fit of h, or on `pnfb`"""
    return O.FIRFilter(h, float(rate), Nphi, tx=tx, polyorder=P, pnfb=_fit(pkg, O, h, Nphi, P) if pnfb is None else pnfb)


_REFS = {}


def _reference(pkg, O, seed, rates, Nphi, hLen, P, x_len, th, tx, how, fused, lengths=None):
    """per channel, the oracle's filter of (H[c], rates[c]) fed x[c] in the pieces of `how`: (outputs [c][piece], end states [c],
    histories [c]); computed once per case and shared by the two kernels.  lengths: per piece, the channels' own lengths (a ragged
    call: channel c is fed the first lengths[i][c] samples of the piece)."""
    key = (seed, tuple(rates), Nphi, hLen, P, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), fused, str(lengths))
    if key not in _REFS:
        H, x = _signal(seed, Nphi, hLen, x_len, th, tx, len(rates))
        O.set_fused(fused)
        try:
            refs = [_oracle(pkg, O, H[c], r, Nphi, P, tx) for c, r in enumerate(rates)]
            pieces = _chunks(x_len, how)
            outs = [[r.filt(x[c, a:(b if lengths is None else a + lengths[i][c])]) for i, (a, b) in enumerate(pieces)] for c, r in enumerate(refs)]
        finally:
            O.set_fused(False)
        _REFS[key] = (outs, [_state5(r.state) for r in refs], [r.history for r in refs])
    return _REFS[key]


def _env(monkeypatch, multi, grid=None):
    """the universal kernels (MRHIP_FORCE_GENERIC is read when the device object is created) or the multi ones wherever their plans fit
    (MRHIP_FARROW_RATES_BANK_MULTI=1; MRHIP_FARROW_RATES_MULTI=1 for a filter whose taps are still shared)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if multi else "1")
    monkeypatch.setenv("MRHIP_FARROW_RATES_BANK_MULTI", "1")
    monkeypatch.setenv("MRHIP_FARROW_RATES_MULTI", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_FARROW_RATES_BANK_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_FARROW_RATES_BANK_GRID", str(grid))


def _filter(pkg, monkeypatch, H, rates, Nphi, P, tx, multi, fused=False, grid=None, pnfb=None):
    _env(monkeypatch, multi, grid)
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    return pkg.FIRFilter.per_channel_taps_and_rates_farrow(H, rates, Nphi, P, numerics=numerics, pnfb=pnfb).bind(tx, len(rates))


def _run_case(pkg, O, monkeypatch, torch, rates, Nphi, hLen, P, x_len, th, tx, multi, fused, chunkings=CHUNKINGS, grid=None):
    seed = 1000 * Nphi + hLen + x_len
    nch = len(rates)
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, nch)
    xd = torch.from_numpy(np.array(x)).cuda()
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        outs, states, hists = _reference(pkg, O, seed, rates, Nphi, hLen, P, x_len, th, tx, how, fused)
        f = _filter(pkg, monkeypatch, H, rates, Nphi, P, tx, multi, fused, grid)
        want_dtype = outs[0][0].dtype
        assert f.output_dtype == want_dtype
        some_zero_beside_outputs = False
        for i, (a, b) in enumerate(pieces):
            what = f"rates {rates[:4]} Nphi {Nphi} hLen {hLen} P {P} x_len {x_len} {np.dtype(th).name}/{np.dtype(tx).name} {name} piece {i} [{a}, {b})"
            bound = f.outputlength_bound(b - a)
            y = torch.zeros((nch, bound), dtype=_tt(torch, want_dtype), device="cuda")
            xin = xd[:, a:b] if nch > 1 else xd[0, a:b]
            counts = f.filt_into(y if nch > 1 else y[0], xin)
            want = [len(outs[c][i]) for c in range(nch)]
            assert counts.dtype == np.int64 and list(counts) == want, (what, list(counts), want)      # counts_out
            assert [s.last_count for s in f.channel_states] == want, what                             # last_count
            yh = y.cpu().numpy()
            for c in range(nch):
                assert_bit_equal(yh[c, :want[c]], outs[c][i], f"{what}: channel {c}")
            if b > a:
                assert f.last_kernel_name() == (MULTI if multi else GENERIC), what
            some_zero_beside_outputs = some_zero_beside_outputs or (min(want) == 0 < max(want))
        _check_end(f, states, hists, f"{name} x_len {x_len}")
        if rates is R4 and name == "prime" and x_len == 1500:
            assert some_zero_beside_outputs       # the short-input path of one channel while its neighbours produce outputs
        f.close()


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("shape,types", CASES, ids=[f"{s[0]}x{s[1]}p{s[2]}-{np.dtype(t[0]).name}-{np.dtype(t[1]).name}" for s, t in CASES])
def test_every_channel_is_its_one_channel_filter(pkg, O, monkeypatch, torch_cuda, shape, types, fused, multi):
    (Nphi, hLen, P), (th, tx) = shape, types
    for rates in (R3, R4):
        for x_len in X_LENS + (X_LENS_MULTI if multi else []):               # (the multi kernel: also lanes with 1, 2 and 3 live slots of four)
            _run_case(pkg, O, monkeypatch, torch_cuda, rates, Nphi, hLen, P, x_len, th, tx, multi, fused)


@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("P", [4, 1], ids=["p4", "p1"])
@pytest.mark.parametrize("x_len", X_LENS_MULTI)
def test_a_count_that_ends_inside_a_lanes_runs(pkg, O, monkeypatch, torch_cuda, x_len, P, fused):
    """the multi kernel's sizes: lanes with four, three, two and one live outputs, a tile behind a channel's count"""
    _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, P, x_len, np.float32, np.float32, True, fused, chunkings={"whole": None})
    _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, P, x_len, np.float64, np.complex128, True, fused, chunkings={"whole": None})
    outs, _, _ = _reference(pkg, O, 1000 * 32 + 250 + x_len, R3, 32, 250, P, x_len, np.float32, np.float32, None, fused)
    tails = sorted(len(outs[c][0]) % 1024 for c in range(3))                # the sizes are what tests/test_gpu_rates_farrow.py says they are
    assert tails == ([6, 139, 485] if x_len == 1030 else [52, 363, 988]), tails


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("rates", [R67, R1], ids=["nch67", "nch1"])
def test_a_second_wave_of_the_schedule_kernel_and_one_channel(pkg, O, monkeypatch, torch_cuda, rates, fused, multi):
    for x_len in X_LENS:
        _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, 4, x_len, np.float32, np.float32, multi, fused)
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 3, 40, 2, 1500, np.float64, np.complex64, multi, fused, chunkings={"prime": 97})


@pytest.mark.parametrize("grid", [1, 2, 3, 2000])
def test_multi_kernel_on_any_grid(pkg, O, monkeypatch, torch_cuda, grid):
    """one workgroup for every tile, a few, and more workgroups than tiles: a workgroup's run crosses several channels -- several banks --
    in the 97-sample pieces also a channel whose count is 0 in that call"""
    _run_case(pkg, O, monkeypatch, torch_cuda, R4, 32, 250, 4, 1500, np.float32, np.float32, True, False, chunkings={"whole": None, "prime": 97}, grid=grid)
    _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, 4, 2100, np.float32, np.float32, True, False, chunkings={"whole": None}, grid=grid)


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
def test_ragged_calls(pkg, O, monkeypatch, torch_cuda, fused, multi):
    """mrhip_filt_device_rates_ragged: every channel against the oracle fed its own samples, a channel of length 0 among them"""
    torch = torch_cuda
    rates, Nphi, hLen, P, th, tx = R4, 32, 250, 4, np.float32, np.float32
    x_len, seed = 1500 * len(RAGGED), 4242
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, 4)
    xd = torch.from_numpy(np.array(x)).cuda()
    outs, states, hists = _reference(pkg, O, seed, rates, Nphi, hLen, P, x_len, th, tx, 1500, fused, lengths=RAGGED)
    f = _filter(pkg, monkeypatch, H, rates, Nphi, P, tx, multi, fused)
    for i, lens in enumerate(RAGGED):
        bound = f.outputlength_bound(max(lens))
        y = torch.zeros((4, bound), dtype=torch.float32, device="cuda")
        counts = f.filt_into(y, xd[:, 1500 * i:1500 * (i + 1)], lengths=lens)
        want = [len(outs[c][i]) for c in range(4)]
        assert list(counts) == want, (i, list(counts), want)
        yh = y.cpu().numpy()
        for c in range(4):
            assert_bit_equal(yh[c, :want[c]], outs[c][i], f"ragged call {i} {lens}: channel {c}")
        assert f.last_kernel_name() == (MULTI if multi else GENERIC)
    _check_end(f, states, hists, "after the ragged calls")
    f.close()


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
def test_set_channel_pnfb_with_banks_of_no_taps(pkg, O, monkeypatch, torch_cuda, fused, multi):
    """banks unrelated to any h (mrhip_set_channel_pnfb, rounded to the tap type as mrhip_create_farrow_pnfb rounds), on a filter built
    from taps and on one built from a caller-fitted bank; oracle and GPU evaluate the same numbers"""
    torch = torch_cuda
    rates, Nphi, hLen, P, x_len = R4, 32, 250, 4, 1500
    H, x = _signal(51, Nphi, hLen, x_len, np.float32, np.float32, 4)
    rng = np.random.default_rng(52)
    PN = rng.standard_normal((4, 8, P + 1)) / np.array([1.0, 32.0, 32.0 ** 2, 32.0 ** 3, 32.0 ** 4])      # Float64 that no Float32 holds
    rounded = PN.astype(np.float32).astype(np.float64)
    assert not np.array_equal(PN, rounded) and len({rounded[c].tobytes() for c in range(4)}) == 4
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, multi)
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    a = pkg.FIRFilter.per_channel_rates_farrow(np.array(H[0]), rates, Nphi, P, numerics=numerics).bind(np.float32, 4)
    a.set_channel_pnfb(PN)
    b = pkg.FIRFilter.per_channel_taps_and_rates_farrow(H, rates, Nphi, P, numerics=numerics, pnfb=PN).bind(np.float32, 4)
    O.set_fused(fused)
    try:
        for f in (a, b):
            assert f.pnfb().shape == (4, 8, P + 1)
            assert_bit_equal(f.pnfb(), rounded, "the installed banks, in the tap type")
            refs = [_oracle(pkg, O, H[c], r, Nphi, P, np.float32, pnfb=rounded[c]) for c, r in enumerate(rates)]
            for lo, hi in _chunks(x_len, 97):
                ys = f.filt(xd[:, lo:hi])
                for c, r in enumerate(refs):
                    assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c, lo:hi]), f"[{lo}, {hi}) channel {c}")
                assert f.last_kernel_name() == (MULTI if multi else GENERIC)
            _check_end(f, [_state5(r.state) for r in refs], [r.history for r in refs], "banks of no taps")
            f.close()
    finally:
        O.set_fused(False)


@pytest.mark.parametrize("types", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.complex64)], ids=["f32", "f32-f64", "f64-c64"])
def test_the_two_calls_install_the_same_banks_and_the_queries_answer_per_channel(pkg, O, monkeypatch, torch_cuda, types):
    """set_channel_taps_farrow(H) and set_channel_pnfb(fits of H) give bit-equal filters; pnfb() is per_channel_farrow(H, ...).pnfb() and
    tapsforphase gives row c from bank c, before any call and after"""
    torch = torch_cuda
    th, tx = types
    Nphi, hLen, P = 32, 250, 4
    H, x = _signal(81, Nphi, hLen, 300, th, tx, 3)
    xd = torch.from_numpy(np.array(x)).cuda()
    fits = np.stack([_fit(pkg, O, H[c], Nphi, P) for c in range(3)])
    bank = pkg.FIRFilter.per_channel_farrow(H, 1.5, Nphi, P).bind(tx, 3)
    phases = (0.0, 1.0, 17.375, 32.999, 33.0)
    want_pnfb, want_rows = bank.pnfb(), [bank.tapsforphase(p) for p in phases]
    assert want_pnfb.shape == (3, 8, P + 1) and want_rows[0].shape == (3, 8) and want_rows[0].dtype == np.dtype(th)
    assert_bit_equal(want_pnfb, fits, "the bank filter's fit against the per-row fit")
    ones = [pkg.FIRFilter(np.array(H[c]), 1.5, Nphi, P).bind(tx, 1) for c in range(3)]
    for c, one in enumerate(ones):                                          # bank c is bit for bit the bank of mrhip_create_farrow(h_c, ...)
        assert_bit_equal(want_pnfb[c], one.pnfb(), f"bank {c} against the one-channel filter")
        for p, rows in zip(phases, want_rows):
            assert_bit_equal(rows[c], one.tapsforphase(p), f"tapsforphase({p}) row {c}")
        one.close()
    _env(monkeypatch, False)
    by_taps = pkg.FIRFilter.per_channel_rates_farrow(np.array(H[0]), R3, Nphi, P).bind(tx, 3)
    assert by_taps.pnfb().shape == (8, P + 1) and by_taps.tapsforphase(2.5).shape == (8,)            # before the call: as today
    assert_bit_equal(by_taps.pnfb(), fits[0], "the shared bank")
    by_taps.set_channel_taps_farrow(H)
    by_pnfb = pkg.FIRFilter.per_channel_rates_farrow(np.array(H[1]), R3, Nphi, P, pnfb=fits[2]).bind(tx, 3)
    by_pnfb.set_channel_pnfb(fits)
    unbound = pkg.FIRFilter.per_channel_taps_and_rates_farrow(H, R3, Nphi, P).bind(tx, 3)              # (installed at bind)
    outs = []
    for f in (by_taps, by_pnfb, unbound):
        for when in ("before any call", "after a call"):
            assert_bit_equal(f.pnfb(), want_pnfb, f"pnfb {when}")
            for p, rows in zip(phases, want_rows):
                got = f.tapsforphase(p)
                assert got.dtype == rows.dtype
                assert_bit_equal(got, rows, f"tapsforphase({p}) {when}")
            ys = f.filt(xd)
            assert f.last_kernel_name() == GENERIC
        outs.append([y.cpu().numpy() for y in ys])
        with pytest.raises(pkg.MultirateHIPError):
            f.tapsforphase(33.5)
    for other in outs[1:]:
        for c in range(3):
            assert_bit_equal(other[c], outs[0][c], f"the filters of the two calls: channel {c}")
    assert [_state5(s) for s in by_taps.channel_states] == [_state5(s) for s in by_pnfb.channel_states] == [_state5(s) for s in unbound.channel_states]
    for f in (by_taps, by_pnfb, unbound, bank):
        f.close()


def _changed_reference(pkg, O, H0, H1, rates0, rates1, Nphi, P, x, tx, pieces, change_at):
    """channel c: the oracle filter of H0[c] at rates0[c] for the pieces before `change_at`; then a filter REBUILT from the bank of H1[c] at
    rates1[c], given the old one's (inputDeficit, phiAccumulator) through set_state and its history through set_history"""
    outs, states, hists = [], [], []
    for c in range(len(rates0)):
        r = _oracle(pkg, O, H0[c], rates0[c], Nphi, P, tx)
        row = []
        for i, (a, b) in enumerate(pieces):
            if i == change_at:
                st, hist = r.state, r.history
                r = _oracle(pkg, O, H1[c], rates1[c], Nphi, P, tx)
                r.set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
                r.set_history(hist)
            row.append(r.filt(x[c, a:b]))
        outs.append(row), states.append(_state5(r.state)), hists.append(r.history)
    return outs, states, hists


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("rates_too", [False, True], ids=["taps", "taps-and-rates"])
def test_set_channel_taps_farrow_between_calls(pkg, O, monkeypatch, torch_cuda, rates_too, multi):
    """700 samples in 97-sample pieces, new taps (and, rates_too, new rates in the same gap) after the third piece"""
    torch = torch_cuda
    rates, Nphi, hLen, P, x_len, th, tx = R4, 32, 250, 4, 700, np.float32, np.float32
    new_rates = [1.37, 0.5, 2.123, 3.01] if rates_too else rates
    H0, x = _signal(61, Nphi, hLen, x_len, th, tx, 4)
    H1, _ = _signal(62, Nphi, hLen, x_len, th, tx, 4)
    pieces = _chunks(x_len, 97)
    outs, states, hists = _changed_reference(pkg, O, H0, H1, rates, new_rates, Nphi, P, x, tx, pieces, 3)
    xd = torch.from_numpy(np.array(x)).cuda()
    f = _filter(pkg, monkeypatch, H0, rates, Nphi, P, tx, multi)
    for i, (a, b) in enumerate(pieces):
        if i == 3:
            before = [_state5(s) for s in f.channel_states]
            hist_before = f.history.copy()
            if rates_too:
                f.set_channel_rates(new_rates)
            f.set_channel_taps_farrow(H1)
            assert [_state5(s) for s in f.channel_states] == before          # accumulator, deficit and history stay
            assert [s.rate for s in f.channel_states] == list(new_rates)
            assert_bit_equal(f.history, hist_before, "history across set_channel_taps_farrow")
        ys = f.filt(xd[:, a:b])
        for c in range(4):
            assert_bit_equal(ys[c].cpu().numpy(), outs[c][i], f"piece {i}, channel {c}")
        assert f.last_kernel_name() == (MULTI if multi else GENERIC)
    _check_end(f, states, hists, "after the change of taps")
    f.close()


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_reset_keeps_taps_and_rates(pkg, O, monkeypatch, torch_cuda, multi):
    torch = torch_cuda
    Nphi, hLen, P, x_len, th, tx = 32, 250, 4, 1500, np.float32, np.float32
    new_rates = [1.37, 0.5, 2.123, 3.01]
    seed = 1000 * Nphi + hLen + x_len
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, 4)
    xd = torch.from_numpy(np.array(x)).cuda()
    f = _filter(pkg, monkeypatch, H, R4, Nphi, P, tx, multi)
    f.set_channel_rates(new_rates)
    f.filt(xd[:, :333])
    f.reset()
    assert [(s.rate,) + _state5(s) + (s.last_count,) for s in f.channel_states] == [(r, 1, 1.0, 1, 0.0, 1, 0) for r in new_rates]
    assert not f.history.any()
    outs, states, hists = _reference(pkg, O, seed, new_rates, Nphi, hLen, P, x_len, th, tx, None, False)
    ys = f.filt(xd)
    for c in range(4):
        assert_bit_equal(ys[c].cpu().numpy(), outs[c][0], f"after reset: channel {c}")
    assert f.last_kernel_name() == (MULTI if multi else GENERIC)
    _check_end(f, states, hists, "after reset")
    f.close()


def _poisoned(torch, dtype, nch, cap):
    y = torch.empty((nch, cap), dtype=dtype, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    return y


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("installed", [False, True], ids=["shared-taps", "channel-taps"])
def test_refusals_leave_the_filter_as_it_was(pkg, O, monkeypatch, torch_cuda, installed, multi):
    """every refusal of the two calls through ctypes, on a filter whose taps are still shared and on one that has its banks: state,
    history, banks and the next call's outputs are what they would have been"""
    torch = torch_cuda
    lib = pkg.load_library()
    rates, Nphi, hLen, P, n = R3, 32, 250, 4, 300
    H, x = _signal(91, Nphi, hLen, 2 * n, np.float32, np.float32, 3)
    other_taps = np.ascontiguousarray(_signal(92, Nphi, hLen, 2 * n, np.float32, np.float32, 3)[0])
    other_pnfb = np.ascontiguousarray(np.random.default_rng(93).standard_normal((3, 8, P + 1)))
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, multi)
    f = pkg.FIRFilter.per_channel_rates_farrow(np.array(H[0]), rates, Nphi, P).bind(np.float32, 3)
    if installed:
        f.set_channel_taps_farrow(H)
    kernel = (MULTI if multi else GENERIC) if installed else SHARED[multi]
    first = f.filt(xd[:, :n])
    assert f.last_kernel_name() == kernel                                   # (never called: the names the filter always reported)
    before = [_state5(s) + (s.last_count,) for s in f.channel_states]
    hist_before, banks_before = f.history.copy(), (f.pnfb(), f.tapsforphase(3.25))
    assert banks_before[0].shape == ((3, 8, P + 1) if installed else (8, P + 1))
    hnd = f._handle
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def refused(rc, code, text):
        assert rc == code, (rc, code)
        msg = lib.mrhip_last_error().decode()
        assert text in msg, msg

    taps_fn, pnfb_fn = lib.mrhip_set_channel_taps_farrow, lib.mrhip_set_channel_pnfb
    refused(taps_fn(None, ptr(other_taps), hLen, 0), 1, "mrhip_set_channel_taps_farrow")
    refused(pnfb_fn(None, ptr(other_pnfb), 8, P), 1, "mrhip_set_channel_pnfb")
    refused(taps_fn(hnd, None, hLen, 0), 1, "mrhip_set_channel_taps_farrow: h is NULL")
    refused(pnfb_fn(hnd, None, 8, P), 1, "mrhip_set_channel_pnfb: pnfb is NULL")
    refused(taps_fn(hnd, ptr(other_taps), hLen - 1, 0), 1, "mrhip_set_channel_taps_farrow: hLen")
    refused(taps_fn(hnd, ptr(other_taps), hLen + 1, 0), 1, "hLen")
    for T_, P_ in ((7, P), (9, P), (8, P - 1), (8, P + 1)):
        refused(pnfb_fn(hnd, ptr(other_pnfb), T_, P_), 1, "mrhip_set_channel_pnfb: tapsPerPhi and polyorder")
    refused(taps_fn(hnd, ptr(other_taps), hLen, 7), 1, "mrhip_set_channel_taps_farrow: bad tap dtype")
    refused(taps_fn(hnd, ptr(other_taps), hLen, -1), 1, "bad tap dtype")
    for th in (2, 3):
        refused(taps_fn(hnd, ptr(other_taps.astype(np.complex128)), hLen, th), 5, "mrhip_set_channel_taps_farrow: complex taps with per-channel rates are left out")
    refused(taps_fn(hnd, ptr(other_taps.astype(np.float64)), hLen, 1), 1, "mrhip_set_channel_taps_farrow: the taps must have the filter's tap dtype")
    arb = pkg.FIRFilter.per_channel_rates(np.array(H[0]), rates, Nphi).bind(np.float32, 3)
    refused(taps_fn(arb._handle, ptr(other_taps), hLen, 0), 1, "mrhip_set_channel_taps_farrow: a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_taps")
    refused(pnfb_fn(arb._handle, ptr(other_pnfb), 8, P), 1, "mrhip_set_channel_pnfb: a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_taps")
    one = pkg.FIRFilter(np.array(H[0]), 2.123, Nphi, P).bind(np.float32, 3)
    bank = pkg.FIRFilter.per_channel_farrow(H, 2.123, Nphi, P).bind(np.float32, 3)
    for g in (one, bank):
        refused(taps_fn(g._handle, ptr(other_taps), hLen, 0), 1, "mrhip_set_channel_taps_farrow takes a filter of mrhip_create_farrow_rates")
        refused(pnfb_fn(g._handle, ptr(other_pnfb), 8, P), 1, "mrhip_set_channel_pnfb takes a filter of mrhip_create_farrow_rates")
    # (a rank-deficient fit needs polyorder + 1 > Nphi, which no constructor lets through: that refusal has no case here)
    # set_channel_taps keeps refusing a FIRFarrow filter with status 5
    refused(lib.mrhip_set_channel_taps(hnd, ptr(other_taps), hLen, 0), 5, "FIRFarrow")
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.set_channel_taps(other_taps)
    assert e.value.code == 5
    for call in (lambda: f.set_channel_taps_farrow(other_taps[:2]), lambda: f.set_channel_taps_farrow(other_taps[:, :-1]),
                 lambda: f.set_channel_taps_farrow(other_taps.astype(np.float64)), lambda: f.set_channel_pnfb(other_pnfb[:, :7]),
                 lambda: f.set_channel_pnfb(other_pnfb[:, :, :P]), lambda: one.set_channel_taps_farrow(other_taps), lambda: bank.set_channel_pnfb(other_pnfb),
                 lambda: arb.set_channel_taps_farrow(other_taps)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == 1
    for call in (lambda: f.set_channel_taps_farrow(other_taps.astype(np.complex64)), lambda: f.set_channel_pnfb(other_pnfb.astype(np.complex128))):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == 5
    # nothing moved
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == before
    assert_bit_equal(f.history, hist_before, "history after the refused calls")
    for g, w in zip((f.pnfb(), f.tapsforphase(3.25)), banks_before):
        assert_bit_equal(g, w, "banks after the refused calls")
    # and the stream goes on as if nothing had happened
    O.set_fused(False)
    refs = [_oracle(pkg, O, H[c] if installed else H[0], r, Nphi, P, np.float32) for c, r in enumerate(rates)]
    second = f.filt(xd[:, n:])
    assert f.last_kernel_name() == kernel
    for c, r in enumerate(refs):
        assert_bit_equal(first[c].cpu().numpy(), r.filt(x[c, :n]), f"first call, channel {c}")
        assert_bit_equal(second[c].cpu().numpy(), r.filt(x[c, n:]), f"the call after the refusals, channel {c}")
    assert [_state5(s) for s in f.channel_states] == [_state5(r.state) for r in refs]
    # what refuses a filter with per-channel rates keeps refusing; the bound answers as before
    nw = C.c_int64(-7)
    y = _poisoned(torch, torch.float32, 3, f.outputlength_bound(n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mrhip_filt_device(hnd, C.c_void_p(xd.data_ptr()), n, 2 * n, C.c_void_p(y.data_ptr()), y.shape[1], y.shape[1], C.byref(nw), stream) == 5
    assert (y.view(torch.uint8) == POISON).all().item()
    assert f.outputlength_bound(n) == math.ceil(n * max(rates)) + 2
    for g in (arb, one, bank, f):
        g.close()


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_states_numerics_and_history_calls_work_as_before(pkg, O, monkeypatch, torch_cuda, multi):
    """mrhip_set_channel_states, mrhip_set_numerics and mrhip_set_history on a filter that has its banks"""
    torch = torch_cuda
    rates, Nphi, hLen, P, x_len = R4, 32, 250, 4, 700
    H, x = _signal(77, Nphi, hLen, x_len, np.float32, np.float32, 4)
    xd = torch.from_numpy(np.array(x)).cuda()
    start = [(3, 1.0), (1, 17.625), (120, 32.99999), (2, 5.5)]             # per-channel (inputDeficit, phiAccumulator)
    hist = np.random.default_rng(3).random((4, 7)).astype(np.float32)
    f = _filter(pkg, monkeypatch, H, rates, Nphi, P, np.float32, multi)
    f.set_channel_states([d for d, _ in start], [a for _, a in start])
    f.set_history(hist)
    lib = pkg.load_library()
    assert lib.mrhip_set_numerics(f._handle, pkg.NUMERICS_FUSED) == 0
    O.set_fused(True)
    try:
        refs = [_oracle(pkg, O, H[c], r, Nphi, P, np.float32) for c, r in enumerate(rates)]
        for r, (d, a), hr in zip(refs, start, hist):
            r.set_state(int(math.floor(a)), int(d), float(a))
            r.set_history(hr)
        for lo, hi in _chunks(x_len, 97):
            ys = f.filt(xd[:, lo:hi])
            for c, r in enumerate(refs):
                assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c, lo:hi]), f"[{lo}, {hi}) channel {c}")
    finally:
        O.set_fused(False)
    assert f.last_kernel_name() == (MULTI if multi else GENERIC)
    _check_end(f, [_state5(r.state) for r in refs], [r.history for r in refs], "after set_channel_states")
    f.close()


# ---- write only your own outputs: a checker per row -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "A", "B", "C"])
@pytest.mark.parametrize("types", [(np.float32, np.float32), (np.float64, np.complex64)], ids=["f32", "c128"])
@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, O, monkeypatch, torch_cuda, multi, types, layout):
    torch = torch_cuda
    th, tx = types
    rates, Nphi, hLen, P = R4, 32, 250, 4
    sizes = [257, 5, 40, 300, 500]             # (500 at 2.123: 1062 outputs, a lane of the multi kernel with one live slot of four)
    x_len = sum(sizes)
    H, x = _signal(31, Nphi, hLen, x_len, th, tx, 4)
    pieces = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
    O.set_fused(False)
    refs = [_oracle(pkg, O, H[c], r, Nphi, P, tx) for c, r in enumerate(rates)]
    f = _filter(pkg, monkeypatch, H, rates, Nphi, P, tx, multi)
    oy, _, ox = LAYOUTS[layout]
    xback = torch.zeros((4, ox + x_len + 3), dtype=_tt(torch, tx), device="cuda")
    xback[:, ox:ox + x_len] = torch.from_numpy(np.array(x)).cuda()
    saw_zero = False
    for i, (a, b) in enumerate(pieces):
        want = [r.filt(x[c, a:b]) for c, r in enumerate(refs)]
        cap = f.outputlength_bound(b - a)
        es = np.dtype(want[0].dtype).itemsize
        pad = row_pad(layout, oy, cap, es)
        view, backing = make_buffer(torch, want[0].dtype, 4, cap, oy, pad)
        counts = f.filt_into(view, xback[:, ox + a:ox + b])
        assert list(counts) == [len(w) for w in want]
        assert f.last_kernel_name() == (MULTI if multi else GENERIC)
        _assert_rows_only_written(backing, 4, cap, oy, pad, counts, want, f"{layout} piece {i} [{a}, {b})")
        saw_zero = saw_zero or (min(counts) == 0 < max(counts))
    assert saw_zero                                                         # a call in which one channel's count is 0
    assert [_state5(s) for s in f.channel_states] == [_state5(r.state) for r in refs]
    f.close()
