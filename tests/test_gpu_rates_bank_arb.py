"""GPU tests of per-channel taps with per-channel rates for FIRArbitrary (the BANK kernels of csrc/kernels_rates_arb.hip): mrhip_set_channel_taps on a
filter of mrhip_create_arbitrary_rates, FIRFilter.set_channel_taps(H) and FIRFilter.per_channel_taps_and_rates(H, rates, Nphi) -- one
FIRFilter(H[c], rates[c], Nphi) per channel behind one filter object.

Bar (include/multirate_hip.h, "Per-channel taps with per-channel rates for FIRArbitrary"): for every channel c the outputs and the count
of every call, the end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx) and the history are BIT FOR BIT those of the oracle's
O.FIRFilter(H[c], rates[c], Nphi, tx=tx) fed x[c] -- under STRICT and FUSED, on the universal kernel (reported as arb_rates_bank_generic,
MRHIP_FORCE_GENERIC=1) and on the tiled one (arb_rates_bank_tiled, MRHIP_ARB_RATES_BANK_TILED=1).  No tolerance anywhere.  The rows of H
are all different and so are the rows of x: channels of equal rate no longer give equal rows, and a kernel that reads the wrong bank
fails.  The shapes are those of tests/test_gpu_rates_arb.py, the smallest at which these kernels can go wrong.  The module also holds the
write-only-own-outputs cases of the two kernels (poisoned buffers of tests/output_bounds_cases.py, a checker per row).
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, POISON, make_buffer, row_pad
from test_gpu_rates_arb import (CASES, CHUNKINGS, R1, R3, R4, R67, X_LENS, _assert_rows_only_written, _check_end, _chunks, _state5, _tt)

pytestmark = pytest.mark.gpu

GENERIC, TILED = "arb_rates_bank_generic", "arb_rates_bank_tiled"
SHARED = {False: "arb_rates_generic", True: "arb_rates_tiled"}


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
        H.setflags(write=False), x.setflags(write=False)
        _SIGNALS[key] = (H, x)
    return _SIGNALS[key]


_REFS = {}


def _reference(O, seed, rates, Nphi, hLen, x_len, th, tx, how, fused, lengths=None):
    """per channel, O.FIRFilter(H[c], rates[c], Nphi, tx=tx) fed x[c] in the pieces of `how`: (outputs [c][piece], end states [c],
    histories [c]); computed once per case and shared by the two kernels.  lengths: per piece, the channels' own lengths (a ragged
    call: channel c is fed the first lengths[i][c] samples of the piece)."""
    key = (seed, tuple(rates), Nphi, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), fused, str(lengths))
    if key not in _REFS:
        H, x = _signal(seed, Nphi, hLen, x_len, th, tx, len(rates))
        O.set_fused(fused)
        try:
            refs = [O.FIRFilter(H[c], float(r), Nphi, tx=tx) for c, r in enumerate(rates)]
            pieces = _chunks(x_len, how)
            outs = [[r.filt(x[c, a:(b if lengths is None else a + lengths[i][c])]) for i, (a, b) in enumerate(pieces)] for c, r in enumerate(refs)]
        finally:
            O.set_fused(False)
        _REFS[key] = (outs, [_state5(r.state) for r in refs], [r.history for r in refs])
    return _REFS[key]


def _env(monkeypatch, tiled, grid=None):
    """the universal kernels (MRHIP_FORCE_GENERIC is read when the device object is created) or the tiled ones wherever their LDS plans
    fit (MRHIP_ARB_RATES_BANK_TILED=1; MRHIP_ARB_RATES_TILED=1 for a filter whose taps are still shared)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if tiled else "1")
    monkeypatch.setenv("MRHIP_ARB_RATES_BANK_TILED", "1")
    monkeypatch.setenv("MRHIP_ARB_RATES_TILED", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_ARB_RATES_BANK_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_ARB_RATES_BANK_GRID", str(grid))


def _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled, fused=False, grid=None):
    _env(monkeypatch, tiled, grid)
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    return pkg.FIRFilter.per_channel_taps_and_rates(H, rates, Nphi, numerics=numerics).bind(tx, len(rates))


def _run_case(pkg, O, monkeypatch, torch, rates, Nphi, hLen, x_len, th, tx, tiled, fused, chunkings=CHUNKINGS, grid=None):
    seed = 1000 * Nphi + hLen + x_len
    nch = len(rates)
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, nch)
    xd = torch.from_numpy(np.array(x)).cuda()
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        outs, states, hists = _reference(O, seed, rates, Nphi, hLen, x_len, th, tx, how, fused)
        f = _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled, fused, grid)
        want_dtype = outs[0][0].dtype
        assert f.output_dtype == want_dtype
        some_zero_beside_outputs = False
        for i, (a, b) in enumerate(pieces):
            what = f"rates {rates[:4]} Nphi {Nphi} hLen {hLen} x_len {x_len} {np.dtype(th).name}/{np.dtype(tx).name} {name} piece {i} [{a}, {b})"
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
                assert f.last_kernel_name() == (TILED if tiled else GENERIC), what
            some_zero_beside_outputs = some_zero_beside_outputs or (min(want) == 0 < max(want))
        _check_end(f, states, hists, f"{name} x_len {x_len}")
        if rates is R4 and name == "prime" and x_len == 1500:
            assert some_zero_beside_outputs       # the short-input path of one channel while its neighbours produce outputs
        f.close()


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("bank,types", CASES, ids=[f"{b[0]}x{b[1]}-{np.dtype(t[0]).name}-{np.dtype(t[1]).name}" for b, t in CASES])
def test_every_channel_is_its_one_channel_filter(pkg, O, monkeypatch, torch_cuda, bank, types, fused, tiled):
    (Nphi, hLen), (th, tx) = bank, types
    for rates in (R3, R4):
        for x_len in X_LENS:
            _run_case(pkg, O, monkeypatch, torch_cuda, rates, Nphi, hLen, x_len, th, tx, tiled, fused)


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("rates", [R67, R1], ids=["nch67", "nch1"])
def test_a_second_wave_of_the_schedule_kernel_and_one_channel(pkg, O, monkeypatch, torch_cuda, rates, fused, tiled):
    for x_len in X_LENS:
        _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, x_len, np.float32, np.float32, tiled, fused)
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 3, 40, 1500, np.float64, np.complex64, tiled, fused, chunkings={"prime": 97})


@pytest.mark.parametrize("rates", [R4, R67], ids=["R4", "R67"])
@pytest.mark.parametrize("grid", [1, 2, 3, 2000])
def test_tiled_kernel_on_any_grid(pkg, O, monkeypatch, torch_cuda, grid, rates):
    """one workgroup for every tile, a few, and more workgroups than tiles (R4 at 1500 samples: 4 x 63 = 252 tiles, R67: 67 x 22 = 1474): a
    workgroup's run crosses several channels, in the 97-sample pieces also one whose count is 0 in that call"""
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, 1500, np.float32, np.float32, True, False, chunkings={"whole": None, "prime": 97}, grid=grid)


RAGGED = [[1500, 0, 257, 1499], [1500, 1, 257, 1499], [0, 0, 0, 5], [3, 1500, 1500, 0]]      # (the second differs from the first in the zero-length channel only)


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
def test_ragged_calls(pkg, O, monkeypatch, torch_cuda, fused, tiled):
    """mrhip_filt_device_rates_ragged: every channel against the oracle fed its own samples, a channel of length 0 among them"""
    torch = torch_cuda
    rates, Nphi, hLen, th, tx = R4, 32, 250, np.float32, np.float32
    x_len, seed = 1500 * len(RAGGED), 4242
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, 4)
    xd = torch.from_numpy(np.array(x)).cuda()
    outs, states, hists = _reference(O, seed, rates, Nphi, hLen, x_len, th, tx, 1500, fused, lengths=RAGGED)
    f = _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled, fused)
    for i, lens in enumerate(RAGGED):
        bound = f.outputlength_bound(max(lens))
        y = torch.zeros((4, bound), dtype=torch.float32, device="cuda")
        counts = f.filt_into(y, xd[:, 1500 * i:1500 * (i + 1)], lengths=lens)
        want = [len(outs[c][i]) for c in range(4)]
        assert list(counts) == want, (i, list(counts), want)
        yh = y.cpu().numpy()
        for c in range(4):
            assert_bit_equal(yh[c, :want[c]], outs[c][i], f"ragged call {i} {lens}: channel {c}")
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    _check_end(f, states, hists, "after the ragged calls")
    f.close()


def _changed_taps_reference(O, H0, H1, rates0, rates1, Nphi, x, tx, pieces, change_at):
    """channel c: the oracle filter of H0[c] at rates0[c] for the pieces before `change_at`; then a filter REBUILT from H1[c] at
    rates1[c], given the old one's (inputDeficit, phiAccumulator) through set_state and its history through set_history"""
    outs, states, hists = [], [], []
    for c in range(len(rates0)):
        r = O.FIRFilter(H0[c], float(rates0[c]), Nphi, tx=tx)
        row = []
        for i, (a, b) in enumerate(pieces):
            if i == change_at:
                st, hist = r.state, r.history
                r = O.FIRFilter(H1[c], float(rates1[c]), Nphi, tx=tx)
                r.set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
                r.set_history(hist)
            row.append(r.filt(x[c, a:b]))
        outs.append(row), states.append(_state5(r.state)), hists.append(r.history)
    return outs, states, hists


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("rates_too", [False, True], ids=["taps", "taps-and-rates"])
def test_set_channel_taps_between_calls(pkg, O, monkeypatch, torch_cuda, rates_too, tiled):
    """700 samples in 97-sample pieces, new taps (and, rates_too, new rates in the same gap) after the third piece"""
    torch = torch_cuda
    rates, Nphi, hLen, x_len, th, tx = R4, 32, 250, 700, np.float32, np.float32
    new_rates = [1.37, 0.5, 2.123, 3.01] if rates_too else rates
    H0, x = _signal(61, Nphi, hLen, x_len, th, tx, 4)
    H1, _ = _signal(62, Nphi, hLen, x_len, th, tx, 4)
    pieces = _chunks(x_len, 97)
    outs, states, hists = _changed_taps_reference(O, H0, H1, rates, new_rates, Nphi, x, tx, pieces, 3)
    xd = torch.from_numpy(np.array(x)).cuda()
    f = _filter(pkg, monkeypatch, H0, rates, Nphi, tx, tiled)
    for i, (a, b) in enumerate(pieces):
        if i == 3:
            before = [_state5(s) for s in f.channel_states]
            hist_before = f.history.copy()
            if rates_too:
                f.set_channel_rates(new_rates)
            f.set_channel_taps(H1)
            assert [_state5(s) for s in f.channel_states] == before          # accumulator, deficit and history stay
            assert_bit_equal(f.history, hist_before, "history across set_channel_taps")
        ys = f.filt(xd[:, a:b])
        for c in range(4):
            assert_bit_equal(ys[c].cpu().numpy(), outs[c][i], f"piece {i}, channel {c}")
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    _check_end(f, states, hists, "after the change of taps")
    f.close()


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
def test_equal_rows_give_the_shared_taps_filter(pkg, monkeypatch, torch_cuda, fused, tiled):
    """all rows of H equal to one h: outputs, counts, states and history bit-equal to per_channel_rates(h, ...) on the same input"""
    torch = torch_cuda
    rates, Nphi, hLen, x_len = R4, 32, 250, 1500
    H, x = _signal(71, Nphi, hLen, x_len, np.float32, np.float32, 4)
    h = np.array(H[2])
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, tiled)
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    shared = pkg.FIRFilter.per_channel_rates(h, rates, Nphi, numerics=numerics).bind(np.float32, 4)
    f = pkg.FIRFilter.per_channel_taps_and_rates(np.tile(h, (4, 1)), rates, Nphi, numerics=numerics).bind(np.float32, 4)
    for a, b in _chunks(x_len, 97):
        ya, yb = shared.filt(xd[:, a:b]), f.filt(xd[:, a:b])
        for c in range(4):
            assert_bit_equal(yb[c].cpu().numpy(), ya[c].cpu().numpy(), f"[{a}, {b}) channel {c}")
        assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [_state5(s) + (s.last_count,) for s in shared.channel_states]
        assert (shared.last_kernel_name(), f.last_kernel_name()) == (SHARED[tiled], TILED if tiled else GENERIC)
    assert_bit_equal(f.history, shared.history, "history")
    shared.close(), f.close()


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_reset_keeps_the_taps(pkg, O, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rates, Nphi, hLen, x_len, th, tx = R4, 32, 250, 1500, np.float32, np.float32
    seed = 1000 * Nphi + hLen + x_len
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, 4)
    xd = torch.from_numpy(np.array(x)).cuda()
    f = _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled)
    f.filt(xd[:, :333])
    f.reset()
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [(1, 1.0, 1, 0.0, 1, 0)] * 4
    assert not f.history.any()
    outs, states, hists = _reference(O, seed, rates, Nphi, hLen, x_len, th, tx, None, False)
    ys = f.filt(xd)
    for c in range(4):
        assert_bit_equal(ys[c].cpu().numpy(), outs[c][0], f"after reset: channel {c}")
    assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    _check_end(f, states, hists, "after reset")
    f.close()


@pytest.mark.parametrize("types", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.complex64)], ids=["f32", "f32-f64", "f64-c64"])
def test_tap_queries_are_those_of_the_bank_filter(pkg, monkeypatch, torch_cuda, types):
    """taps(0), taps(1) and tapsforphase equal those of per_channel_arbitrary(H, rate, Nphi), before any call and after"""
    torch = torch_cuda
    th, tx = types
    H, x = _signal(81, 32, 250, 300, th, tx, 3)
    bank = pkg.FIRFilter.per_channel_arbitrary(H, 1.5, 32).bind(tx, 3)
    want = (bank.taps(0), bank.taps(1), bank.tapsforphase(1.0), bank.tapsforphase(17.375), bank.tapsforphase(32.999))
    assert want[0].shape == (3, 8, 32) and want[2].shape == (3, 8)
    _env(monkeypatch, False)
    shared = pkg.FIRFilter.per_channel_rates(np.array(H[0]), R3, 32).bind(tx, 3)
    assert shared.taps(0).shape == (8, 32) and shared.tapsforphase(2.5).shape == (8,)       # before the call: as today
    assert_bit_equal(shared.taps(0), want[0][0], "the shared pfb")
    shared.set_channel_taps(H)
    f2 = pkg.FIRFilter.per_channel_taps_and_rates(H, R3, 32).bind(tx, 3)
    for f in (shared, f2):
        for when in ("before any call", "after a call"):
            got = (f.taps(0), f.taps(1), f.tapsforphase(1.0), f.tapsforphase(17.375), f.tapsforphase(32.999))
            for g, w, name in zip(got, want, ("pfb", "dpfb", "tapsforphase(1.0)", "tapsforphase(17.375)", "tapsforphase(32.999)")):
                assert g.dtype == w.dtype
                assert_bit_equal(g, w, f"{name} {when}")
            f.filt(torch.from_numpy(np.array(x)).cuda())
        f.close()
    bank.close()


def _poisoned(torch, dtype, nch, cap):
    y = torch.empty((nch, cap), dtype=dtype, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    return y


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("installed", [False, True], ids=["shared-taps", "channel-taps"])
def test_refusals_leave_the_filter_as_it_was(pkg, O, monkeypatch, torch_cuda, installed, tiled):
    """every refusal of mrhip_set_channel_taps through ctypes, on a filter whose taps are still shared and on one that has its banks:
    state, history, taps and the next call's outputs are what they would have been"""
    torch = torch_cuda
    lib = pkg.load_library()
    rates, Nphi, hLen, n = R3, 32, 250, 300
    seed = 91
    H, x = _signal(seed, Nphi, hLen, 2 * n, np.float32, np.float32, 3)
    Hn = np.ascontiguousarray(H)
    other_taps = np.ascontiguousarray(_signal(92, Nphi, hLen, 2 * n, np.float32, np.float32, 3)[0])
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, tiled)
    f = pkg.FIRFilter.per_channel_rates(np.array(H[0]), rates, Nphi).bind(np.float32, 3)
    if installed:
        f.set_channel_taps(H)
    kernel = (TILED if tiled else GENERIC) if installed else SHARED[tiled]
    first = f.filt(xd[:, :n])
    assert f.last_kernel_name() == kernel                                   # (never called: the names the filter always reported)
    before = [_state5(s) + (s.last_count,) for s in f.channel_states]
    hist_before, taps_before = f.history.copy(), (f.taps(0), f.taps(1), f.tapsforphase(3.25))
    hnd = f._handle
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def refused(rc, code, text):
        assert rc == code, (rc, code)
        msg = lib.mrhip_last_error().decode()
        assert text in msg, msg

    refused(lib.mrhip_set_channel_taps(hnd, None, hLen, 0), 1, "h is NULL")
    refused(lib.mrhip_set_channel_taps(hnd, ptr(other_taps), hLen - 1, 0), 1, "hLen")
    refused(lib.mrhip_set_channel_taps(hnd, ptr(other_taps), hLen + 1, 0), 1, "hLen")
    refused(lib.mrhip_set_channel_taps(hnd, ptr(other_taps.astype(np.float64)), hLen, 1), 1, "tap dtype")
    for th in (2, 3):
        refused(lib.mrhip_set_channel_taps(hnd, ptr(other_taps.astype(np.complex128)), hLen, th), 5, "complex taps with per-channel rates are left out")
    refused(lib.mrhip_set_channel_taps(hnd, ptr(other_taps), hLen, 7), 1, "tap dtype")
    refused(lib.mrhip_set_channel_taps(None, ptr(other_taps), hLen, 0), 1, "NULL")
    farrow = pkg.FIRFilter.per_channel_rates_farrow(np.array(H[0]), rates, Nphi, 4).bind(np.float32, 3)
    refused(lib.mrhip_set_channel_taps(farrow._handle, ptr(other_taps), hLen, 0), 5, "FIRFarrow")
    one = pkg.FIRFilter(np.array(H[0]), 2.123, Nphi).bind(np.float32, 3)
    bank = pkg.FIRFilter.per_channel_arbitrary(Hn, 2.123, Nphi).bind(np.float32, 3)
    for g in (one, bank):
        refused(lib.mrhip_set_channel_taps(g._handle, ptr(other_taps), hLen, 0), 1, "mrhip_set_channel_taps takes a filter of mrhip_create_arbitrary_rates")
    for call in (lambda: f.set_channel_taps(other_taps[:2]), lambda: f.set_channel_taps(other_taps[:, :-1]), lambda: f.set_channel_taps(other_taps.astype(np.float64)),
                 lambda: one.set_channel_taps(other_taps)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == 1
    for call in (lambda: f.set_channel_taps(other_taps.astype(np.complex64)), lambda: farrow.set_channel_taps(other_taps)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == 5
    # nothing moved
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == before
    assert_bit_equal(f.history, hist_before, "history after the refused calls")
    for g, w in zip((f.taps(0), f.taps(1), f.tapsforphase(3.25)), taps_before):
        assert_bit_equal(g, w, "taps after the refused calls")
    # and the stream goes on as if nothing had happened
    O.set_fused(False)
    refs = [O.FIRFilter(H[c] if installed else H[0], float(r), Nphi, tx=np.float32) for c, r in enumerate(rates)]
    second = f.filt(xd[:, n:])
    assert f.last_kernel_name() == kernel
    for c, r in enumerate(refs):
        assert_bit_equal(first[c].cpu().numpy(), r.filt(x[c, :n]), f"first call, channel {c}")
        assert_bit_equal(second[c].cpu().numpy(), r.filt(x[c, n:]), f"the call after the refusals, channel {c}")
    assert [_state5(s) for s in f.channel_states] == [_state5(r.state) for r in refs]
    # what refuses a filter with per-channel rates keeps refusing; the bound and the mod form answer as before
    nw = C.c_int64(-7)
    y = _poisoned(torch, torch.float32, 3, f.outputlength_bound(n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mrhip_filt_device(hnd, C.c_void_p(xd.data_ptr()), n, 2 * n, C.c_void_p(y.data_ptr()), y.shape[1], y.shape[1], C.byref(nw), stream) == 5
    assert (y.view(torch.uint8) == POISON).all().item()
    assert f.outputlength_bound(n) == math.ceil(n * max(rates)) + 2
    f.set_mod_form(True), f.set_mod_form(False)
    for g in (farrow, one, bank, f):
        g.close()


# ---- write only your own outputs: a checker per row -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "A", "B", "C"])
@pytest.mark.parametrize("types", [(np.float32, np.float32), (np.float64, np.complex64)], ids=["f32", "c128"])
@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, O, monkeypatch, torch_cuda, tiled, types, layout):
    torch = torch_cuda
    th, tx = types
    rates, Nphi, hLen = R4, 32, 250
    sizes = [257, 5, 40, 300]
    x_len = sum(sizes)
    H, x = _signal(31, Nphi, hLen, x_len, th, tx, 4)
    pieces = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
    O.set_fused(False)
    refs = [O.FIRFilter(H[c], float(r), Nphi, tx=tx) for c, r in enumerate(rates)]
    f = _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled)
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
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        _assert_rows_only_written(backing, 4, cap, oy, pad, counts, want, f"{layout} piece {i} [{a}, {b})")
        saw_zero = saw_zero or (min(counts) == 0 < max(counts))
    assert saw_zero                                                         # a call in which one channel's count is 0
    assert [_state5(s) for s in f.channel_states] == [_state5(r.state) for r in refs]
    f.close()
