"""GPU tests of COMPLEX per-channel taps on the FIRFarrow filter with per-channel rates (csrc/kernels_rates_farrow_ctaps.hip):
mrhip_set_channel_ctaps_farrow, mrhip_set_channel_pnfb_ctaps and mrhip_set_channel_pnfb_ctaps_device on a filter of
mrhip_create_farrow_rates*, FIRFilter.set_channel_ctaps_farrow(H), .set_channel_pnfb_ctaps(PN), .set_channel_pnfb_ctaps_device(PN) and
FIRFilter.per_channel_complex_taps_and_rates_farrow(H, rates, Nphi, polyorder) -- one FIRFilter(H[c]::Vector{Complex}, rates[c], Nphi,
polyorder) per channel behind one filter object.

Bar (include/multirate_hip.h, "Complex per-channel taps with per-channel rates for FIRFarrow"): for every channel c the outputs and the
count of every call, the end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx) and the history are BIT FOR BIT those of the
one-channel complex-tap filter fed x[c] -- tests/complex_taps_farrow_restatement.py (pinned to the oracle by
tests/test_complex_taps_farrow_cpu.py) handed the SAME polynomial bank as the device (set_channel_pnfb_ctaps: no bit of the fit is in
play), for real samples also the untouched oracle by components (O.FIRFilter(..., pnfb = real(PN[c])) and the same over imag, put
together), and in one case per kernel the GPU filters FIRFilter.complex_taps_farrow(..., pnfb = PN[c]) -- on the universal kernel
(reported as farrow_rates_ctaps_generic, MRHIP_FORCE_GENERIC=1) and on the multi kernel (farrow_rates_ctaps_multi,
MRHIP_FARROW_RATES_CTAPS_MULTI=1).  STRICT only; no tolerance anywhere.  Row 0 of H is random complex, row 1 a single 1j at tap 0, row 2
-conj(reverse(row 0)), further rows random, and the rows of x are all different (the signals of tests/test_gpu_rates_arb_ctaps.py): a
swapped bank, a shared bank or an exchanged re / im fails.  The shapes are those of tests/test_gpu_rates_farrow.py, the smallest at
which these kernels can go wrong.  The module also holds the write-only-own-outputs cases of the two kernels (poisoned buffers of
tests/output_bounds_cases.py, a checker per row).
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from complex_taps_farrow_restatement import ComplexTapsFarrowRestated, fit_pnfb
from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, POISON, make_buffer, row_pad
from test_gpu_rates_arb_ctaps import _signal
from test_gpu_rates_farrow import CHUNKINGS, R1, R3, R4, R67, SHAPES, X_LENS, X_LENS_MULTI, _assert_rows_only_written, _check_end, _chunks, _state5, _tt

pytestmark = pytest.mark.gpu

GENERIC, MULTI = "farrow_rates_ctaps_generic", "farrow_rates_ctaps_multi"
REAL = {False: "farrow_rates_generic", True: "farrow_rates_multi"}               # the filter's kernels before the install: the one real bank ...
REAL_BANK = {False: "farrow_rates_bank_generic", True: "farrow_rates_bank_multi"}  # ... and a real bank per channel
ALL_TYPES = [(th, tx) for th in (np.complex64, np.complex128) for tx in (np.float32, np.float64, np.complex64, np.complex128)]
FEW_TYPES = [(np.complex64, np.float32), (np.complex128, np.complex64)]
CASES = [((32, 250, 4), t) for t in ALL_TYPES] + [(s, t) for s in SHAPES for t in FEW_TYPES]
THREADS = 256
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multirate.jl_amd", "csrc", "rates_arb.h")
OPL = int(re.search(r"^constexpr int kFarrowRatesCtapsOPL = (\d+);", open(_SRC).read(), flags=re.M).group(1))      # outputs a lane of the multi kernel


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _real_of(th):
    return np.float64 if np.dtype(th) == np.complex128 else np.float32


_BANKS = {}


def _banks(pkg, seed, Nphi, hLen, P, x_len, th, tx, nch):
    """the taps and samples of _signal, and per channel the polynomial bank the device and every reference are handed: the fit of H[c]
    per component (the library's polyfit), every component rounded to the tap's scalar -- values a complex128 array holds exactly"""
    key = (seed, Nphi, hLen, P, x_len, np.dtype(th).name, np.dtype(tx).name, nch)
    if key not in _BANKS:
        H, x = _signal(seed, Nphi, hLen, x_len, th, tx, nch)
        rt = _real_of(th)
        PN = np.stack([fit_pnfb(np.array(H[c]), Nphi, P, pkg.polyfit) for c in range(nch)])
        PN = (PN.real.astype(rt).astype(np.float64) + 1j * PN.imag.astype(rt).astype(np.float64)).astype(np.complex128)
        assert PN.shape == (nch, -(-hLen // Nphi), P + 1) and len({PN[c].tobytes() for c in range(nch)}) == nch
        PN.setflags(write=False)
        _BANKS[key] = (H, PN, x)
    return _BANKS[key]


def _restated(pn, hLen, th, rate, Nphi, P, tx, state=None, hist=None):
    """the one-channel complex-tap filter on the bank `pn`, optionally handed a state (inputDeficit, phiAccumulator and, where it is to
    be compared afterwards, xIdx: a call on the short-input path leaves it where the last walk ended) and a history (samples of tx)"""
    r = ComplexTapsFarrowRestated(hLen, th, float(rate), Nphi, P, np.array(pn), tx)
    if state is not None:
        r.inputDeficit, r.phiAccumulator = int(state[0]), float(state[1])
        if len(state) > 2:
            r.xIdx = int(state[2])
    if hist is not None:
        assert len(hist) == r.historyLen
        r.history = [r._widen(v) for v in np.ascontiguousarray(hist, dtype=tx)]
    return r


def _rstate5(r):
    return (r.inputDeficit, r.phiAccumulator, r.phiIdx, r.alpha, r.xIdx)


_REFS = {}


def _reference(pkg, seed, rates, Nphi, hLen, P, x_len, th, tx, how, lengths=None):
    """per channel, the restatement on PN[c] at rates[c] fed x[c] in the pieces of `how`: (outputs [c][piece], end states [c],
    histories [c]); computed once per case and shared by the two kernels.  lengths: per piece, the channels' own lengths."""
    key = (seed, tuple(rates), Nphi, hLen, P, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), str(lengths))
    if key not in _REFS:
        _, PN, x = _banks(pkg, seed, Nphi, hLen, P, x_len, th, tx, len(rates))
        refs = [_restated(PN[c], hLen, th, r, Nphi, P, tx) for c, r in enumerate(rates)]
        pieces = _chunks(x_len, how)
        outs = [[r.filt(x[c, a:(b if lengths is None else a + lengths[i][c])], scalar=False) for i, (a, b) in enumerate(pieces)] for c, r in enumerate(refs)]
        _REFS[key] = (outs, [_rstate5(r) for r in refs], [r.history_array() for r in refs])
    return _REFS[key]


def _oracle_by_components(O, H, PN, x, rates, Nphi, P, tx, pieces):
    """real samples: a complex tap times a real sample is two real products, so channel c is O.FIRFilter(..., pnfb = real(PN[c])) and the
    same over imag(PN[c]), put together -- the untouched oracle (its h gives the length and the tap precision only)"""
    O.set_fused(False)
    outs = []
    for c, r in enumerate(rates):
        h = np.ascontiguousarray(H[c].real)
        fr = O.FIRFilter(h, float(r), Nphi, tx=tx, polyorder=P, pnfb=np.ascontiguousarray(PN[c].real))
        fi = O.FIRFilter(h, float(r), Nphi, tx=tx, polyorder=P, pnfb=np.ascontiguousarray(PN[c].imag))
        row = []
        for a, b in pieces:
            yr, yi = fr.filt(x[c, a:b]), fi.filt(x[c, a:b])
            y = np.empty(len(yr), dtype=np.result_type(yr.dtype, np.complex64))
            y.real, y.imag = yr, yi
            row.append(y)
        outs.append(row)
    return outs


def _env(monkeypatch, multi, grid=None):
    """the universal kernels (MRHIP_FORCE_GENERIC is read when the device object is created) or the multi ones on every call
    (MRHIP_FARROW_RATES_CTAPS_MULTI=1; the two older switches for a filter before its complex install)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if multi else "1")
    monkeypatch.setenv("MRHIP_FARROW_RATES_CTAPS_MULTI", "1")
    monkeypatch.setenv("MRHIP_FARROW_RATES_BANK_MULTI", "1")
    monkeypatch.setenv("MRHIP_FARROW_RATES_MULTI", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_FARROW_RATES_CTAPS_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_FARROW_RATES_CTAPS_GRID", str(grid))


def _filter(pkg, monkeypatch, H, PN, rates, Nphi, P, tx, multi, grid=None):
    _env(monkeypatch, multi, grid)
    return pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(H, rates, Nphi, P, pnfb=PN).bind(tx, len(rates))


def _run_case(pkg, O, monkeypatch, torch, rates, Nphi, hLen, P, x_len, th, tx, multi, chunkings=CHUNKINGS, grid=None, against_gpu=False):
    seed = 1000 * Nphi + hLen + x_len
    nch = len(rates)
    H, PN, x = _banks(pkg, seed, Nphi, hLen, P, x_len, th, tx, nch)
    xd = torch.from_numpy(np.array(x)).cuda()
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        outs, states, hists = _reference(pkg, seed, rates, Nphi, hLen, P, x_len, th, tx, how)
        by_components = _oracle_by_components(O, H, PN, x, rates, Nphi, P, tx, pieces) if np.dtype(tx).kind != "c" else None
        ones = [pkg.FIRFilter.complex_taps_farrow(np.array(H[c]), float(r), Nphi, P, pnfb=np.array(PN[c])).bind(tx, 1) for c, r in enumerate(rates)] if against_gpu else None
        f = _filter(pkg, monkeypatch, H, PN, rates, Nphi, P, tx, multi, grid)
        want_dtype = outs[0][0].dtype
        assert want_dtype.kind == "c" and f.output_dtype == want_dtype
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
                if by_components is not None:
                    assert_bit_equal(yh[c, :want[c]], by_components[c][i], f"{what}: channel {c} against the oracle by components")
                if ones is not None:
                    assert_bit_equal(yh[c, :want[c]], np.atleast_1d(ones[c].filt(x[c, a:b])), f"{what}: channel {c} against the GPU one-channel filter")
            if b > a:
                assert f.last_kernel_name() == (MULTI if multi else GENERIC), what
            some_zero_beside_outputs = some_zero_beside_outputs or (min(want) == 0 < max(want))
        _check_end(f, states, hists, f"{name} x_len {x_len}")
        if rates is R4 and name == "prime" and x_len == 1500:
            assert some_zero_beside_outputs       # the short-input path of one channel while its neighbours produce outputs
        f.close()
        for g in ones or ():
            g.close()


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("shape,types", CASES, ids=[f"{s[0]}x{s[1]}p{s[2]}-{np.dtype(t[0]).name}-{np.dtype(t[1]).name}" for s, t in CASES])
def test_every_channel_is_its_one_channel_filter(pkg, O, monkeypatch, torch_cuda, shape, types, multi):
    (Nphi, hLen, P), (th, tx) = shape, types
    for rates in (R3, R4):
        for x_len in X_LENS:
            _run_case(pkg, O, monkeypatch, torch_cuda, rates, Nphi, hLen, P, x_len, th, tx, multi)


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_every_channel_is_the_gpu_one_channel_filter(pkg, O, monkeypatch, torch_cuda, multi):
    _run_case(pkg, O, monkeypatch, torch_cuda, R4, 32, 250, 4, 1500, np.complex64, np.complex64, multi, chunkings={"prime": 97}, against_gpu=True)


def _live_slot_counts(count, bound):
    """over the tiles of one channel (the tiling goes by the call's bound): the live-slot counts of the lanes that have any, and
    whether a tile lies at or behind the channel's count"""
    tile, seen, behind = OPL * THREADS, set(), False
    for k0 in range(0, bound, tile):
        if k0 >= count:
            behind = True
            continue
        for tid in range(THREADS):
            live = sum(1 for j in range(OPL) if k0 + tid + THREADS * j < count)
            if live:
                seen.add(live)
    return seen, behind


@pytest.mark.parametrize("P", [4, 1], ids=["p4", "p1"])
def test_a_count_that_ends_inside_a_lanes_runs(pkg, O, monkeypatch, torch_cuda, P):
    """the multi kernel's sizes at rates R3 (a lane owns output tid of OPL consecutive runs of 256): 1030 samples give counts of 485, 1030
    and 2187, 2100 samples 988, 2100 and 4459 -- over the two sizes lanes occur with every number of live slots from 1 to OPL (OPL 2:
    485 = 256 + 229 has lanes with two and with one; OPL 4: 988 = 3 * 256 + 220 has four and three, 485 two and one), and the channel at
    rate 0.47 ends tiles in front of the call's bound, so whole tiles lie behind its count; the universal kernel at the same sizes
    shares the references"""
    seen, behind = set(), False
    for x_len, counts in zip(X_LENS_MULTI, ([485, 1030, 2187], [988, 2100, 4459])):
        for multi in (True, False):
            _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, P, x_len, np.complex64, np.float32, multi, chunkings={"whole": None})
        _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, P, x_len, np.complex128, np.complex128, True, chunkings={"whole": None})
        # the sizes are what the docstring says they are
        outs, _, _ = _reference(pkg, 1000 * 32 + 250 + x_len, R3, 32, 250, P, x_len, np.complex64, np.float32, None)
        assert [len(outs[c][0]) for c in range(3)] == counts, [len(outs[c][0]) for c in range(3)]
        bound = math.ceil(x_len * max(R3)) + 1                               # (at least; a larger bound only adds tiles behind the counts)
        for count in counts:
            s, b = _live_slot_counts(count, bound)
            seen, behind = seen | s, behind or b
    assert seen == set(range(1, OPL + 1)) and behind, (seen, behind)


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("rates", [R67, R1], ids=["nch67", "nch1"])
def test_a_second_wave_of_the_schedule_kernel_and_one_channel(pkg, O, monkeypatch, torch_cuda, rates, multi):
    for x_len in X_LENS:
        _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, 4, x_len, np.complex64, np.float32, multi)
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 3, 40, 2, 1500, np.complex128, np.complex64, multi, chunkings={"prime": 97})


@pytest.mark.parametrize("rates", [R4, R67], ids=["R4", "R67"])
@pytest.mark.parametrize("grid", [1, 2, 3, 2000])
def test_multi_kernel_on_any_grid(pkg, O, monkeypatch, torch_cuda, grid, rates):
    """one workgroup for every tile, a few, and more workgroups than tiles: a workgroup's run crosses several channels, in the 97-sample
    pieces also one whose count is 0 in that call"""
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, 4, 1500, np.complex64, np.float32, True, chunkings={"whole": None, "prime": 97}, grid=grid)


RAGGED = [[1500, 0, 257, 1499], [1500, 1, 257, 1499], [0, 0, 0, 5], [3, 1500, 1500, 0]]      # (the second differs from the first in the zero-length channel only)


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=["real-x", "complex-x"])
def test_ragged_calls(pkg, monkeypatch, torch_cuda, tx, multi):
    """mrhip_filt_device_rates_ragged: every channel against the restatement fed its own samples, a channel of length 0 among them"""
    torch = torch_cuda
    rates, Nphi, hLen, P, th = R4, 32, 250, 4, np.complex64
    x_len, seed = 1500 * len(RAGGED), 4242
    H, PN, x = _banks(pkg, seed, Nphi, hLen, P, x_len, th, tx, 4)
    xd = torch.from_numpy(np.array(x)).cuda()
    outs, states, hists = _reference(pkg, seed, rates, Nphi, hLen, P, x_len, th, tx, 1500, lengths=RAGGED)
    f = _filter(pkg, monkeypatch, H, PN, rates, Nphi, P, tx, multi)
    for i, lens in enumerate(RAGGED):
        bound = f.outputlength_bound(max(lens))
        y = torch.zeros((4, bound), dtype=torch.complex64, device="cuda")
        counts = f.filt_into(y, xd[:, 1500 * i:1500 * (i + 1)], lengths=lens)
        want = [len(outs[c][i]) for c in range(4)]
        assert list(counts) == want, (i, list(counts), want)
        yh = y.cpu().numpy()
        for c in range(4):
            assert_bit_equal(yh[c, :want[c]], outs[c][i], f"ragged call {i} {lens}: channel {c}")
        assert f.last_kernel_name() == (MULTI if multi else GENERIC)
    _check_end(f, states, hists, "after the ragged calls")
    f.close()


# ---- the two host installs and the queries --------------------------------------------------------------------------------------------
PHASES = (0.0, 1.0, 17.375, 32.999, 33.0)


@pytest.mark.parametrize("types", [(np.complex64, np.float32), (np.complex64, np.float64), (np.complex128, np.complex64)], ids=["c64", "c64-f64", "c128-c64"])
def test_the_two_host_calls_install_the_same_banks_and_the_queries_answer_per_channel(pkg, monkeypatch, torch_cuda, types):
    """set_channel_ctaps_farrow(H) and set_channel_pnfb_ctaps(pnfb() of that filter) give bit-equal filters; bank c is bit for bit the
    bank of the one-channel FIRFilter.complex_taps_farrow(H[c], ...) and of per_channel_complex_taps_farrow(H, ...); tapsforphase gives
    row c from bank c, before any call and after"""
    torch = torch_cuda
    th, tx = types
    rt = _real_of(th)
    Nphi, hLen, P = 32, 250, 4
    H, x = _signal(81, Nphi, hLen, 300, th, tx, 3)
    xd = torch.from_numpy(np.array(x)).cuda()
    bank = pkg.FIRFilter.per_channel_complex_taps_farrow(np.array(H), 1.5, Nphi, P).bind(tx, 3)
    want_pnfb, want_rows = bank.pnfb(), [bank.tapsforphase(p) for p in PHASES]
    assert want_pnfb.shape == (3, 8, P + 1) and want_pnfb.dtype == np.complex128 and want_rows[0].shape == (3, 8) and want_rows[0].dtype == np.dtype(th)
    for c in range(3):                                                      # bank c is bit for bit the bank of mrhip_create_farrow_ctaps(h_c, ...)
        one = pkg.FIRFilter.complex_taps_farrow(np.array(H[c]), 1.5, Nphi, P).bind(tx, 1)
        assert_bit_equal(want_pnfb[c], one.pnfb(), f"bank {c} against the one-channel filter")
        one.close()
    _env(monkeypatch, False)
    placeholder = np.ascontiguousarray(H[0].real)
    by_taps = pkg.FIRFilter.per_channel_rates_farrow(placeholder, R3, Nphi, P).bind(tx, 3)
    assert placeholder.dtype == rt and by_taps.pnfb().shape == (8, P + 1) and by_taps.pnfb().dtype == np.float64 and by_taps.tapsforphase(2.5).shape == (8,)
    by_taps.set_channel_ctaps_farrow(np.array(H))
    assert_bit_equal(by_taps.pnfb(), want_pnfb, "the fit of set_channel_ctaps_farrow against the bank filter's")
    by_pnfb = pkg.FIRFilter.per_channel_rates_farrow(np.ascontiguousarray(H[1].imag), R3, Nphi, P).bind(tx, 3)
    by_pnfb.set_channel_pnfb(np.zeros((3, 8, P + 1)))                       # (real banks first: the complex ones take their place)
    by_pnfb.set_channel_pnfb_ctaps(by_taps.pnfb())
    unbound = pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(np.array(H), R3, Nphi, P).bind(tx, 3)      # (installed at bind)
    outs = []
    for f in (by_taps, by_pnfb, unbound):
        assert f.output_dtype == np.dtype(np.result_type(th, tx))
        for when in ("before any call", "after a call"):
            got = f.pnfb()
            assert got.dtype == np.complex128 and got.shape == (3, 8, P + 1)
            assert_bit_equal(got, want_pnfb, f"pnfb {when}")
            for p, rows in zip(PHASES, want_rows):
                got = f.tapsforphase(p)
                assert got.dtype == rows.dtype and got.shape == (3, 8)
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
    # Float32 taps round every component of a handed-over coefficient to Float32, as mrhip_create_farrow_pnfb_ctaps rounds
    odd = np.array(want_pnfb) * (1.0 + 2.0 ** -30) + 1j * 2.0 ** -40
    by_pnfb.set_channel_pnfb_ctaps(odd)
    got = by_pnfb.pnfb()
    want = odd if rt == np.float64 else (odd.real.astype(np.float32).astype(np.float64) + 1j * odd.imag.astype(np.float32).astype(np.float64))
    assert_bit_equal(got, want.astype(np.complex128), "the rounding of handed-over coefficients")
    for f in (by_taps, by_pnfb, unbound, bank):
        f.close()


# ---- the install from device memory -------------------------------------------------------------------------------------------------
def _queries(f):
    return (f.pnfb(), f.tapsforphase(1.0), f.tapsforphase(2.375))


@pytest.mark.parametrize("th", [np.complex64, np.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("shape", [(4, 4, 1), (3, 40, 2), (32, 1024, 6)], ids=["4x4p1", "3x40p2", "32x1024p6"])
def test_device_install_equals_host_install(pkg, monkeypatch, torch_cuda, shape, th):
    """pnfb() and tapsforphase read back after set_channel_pnfb_ctaps_device, and all outputs, are bit-equal to the host install of the
    same array -- with components that do not fit Float32, so that the rounding on the device is in play"""
    torch = torch_cuda
    Nphi, hLen, P = shape
    rt, tx, nch = _real_of(th), np.float32, 3
    x_len = 300
    H, PN, x = _banks(pkg, 7000 + hLen, Nphi, hLen, P, x_len, th, tx, nch)
    _, PN2, _ = _banks(pkg, 7001 + hLen, Nphi, hLen, P, x_len, th, tx, nch)
    T = -(-hLen // Nphi)
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, False)
    placeholder = np.ascontiguousarray(H[0].real)
    host = pkg.FIRFilter.per_channel_rates_farrow(placeholder, R3, Nphi, P).bind(tx, nch)
    dev = pkg.FIRFilter.per_channel_rates_farrow(placeholder, R3, Nphi, P).bind(tx, nch)
    for k, M in enumerate((PN, PN2)):                                        # the first install allocates, the second reuses the banks
        M = np.array(M) * (1.0 + 2.0 ** -29) + (2.0 ** -45) * (1 + 1j)      # not representable in Float32 (nor, mostly, the products in Float64)
        host.set_channel_pnfb_ctaps(M)
        dev.set_channel_pnfb_ctaps_device(torch.from_numpy(M).cuda())
        assert dev.output_dtype == host.output_dtype == np.dtype(np.result_type(th, tx))
        want = M if rt == np.float64 else (M.real.astype(np.float32).astype(np.float64) + 1j * M.imag.astype(np.float32).astype(np.float64))
        assert_bit_equal(dev.pnfb(), want.astype(np.complex128), f"install {k}: the banks as built")
        for g, w, name in zip(_queries(dev), _queries(host), ("pnfb", "tapsforphase(1.0)", "tapsforphase(2.375)")):
            assert g.dtype == (np.complex128 if name == "pnfb" else np.dtype(th)) and g.shape == w.shape == ((nch, T, P + 1) if name == "pnfb" else (nch, T))
            assert_bit_equal(g, w, f"install {k}: {name}")
        for c in range(nch):                                                 # the queries are those of the one-channel restatement
            r = _restated(want[c], hLen, th, R3[c], Nphi, P, tx)
            assert_bit_equal(host.tapsforphase(2.375)[c], r.tapsforphase(2.375), f"install {k}: tapsforphase of channel {c}")
        a, b = (0, 150) if k == 0 else (150, 300)
        ya, yb = host.filt(xd[:, a:b]), dev.filt(xd[:, a:b])
        for c in range(nch):
            assert_bit_equal(yb[c].cpu().numpy(), ya[c].cpu().numpy(), f"install {k}: outputs of channel {c}")
        assert dev.last_kernel_name() == host.last_kernel_name() == GENERIC
    assert [_state5(s) for s in dev.channel_states] == [_state5(s) for s in host.channel_states]
    assert_bit_equal(dev.history, host.history, "history")
    host.close(), dev.close()


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_a_loop_of_device_installs_that_never_meets_the_host(pkg, monkeypatch, torch_cuda, multi):
    """the tracker's loop: every piece installs new complex banks from device memory and filters, nothing is read back until the loop is
    over (the first install allocates and may wait once; every later one enqueues a kernel and returns) -- then every piece equals the
    twin driven through set_channel_pnfb_ctaps with the same values, and the restatement rebuilt per piece"""
    torch = torch_cuda
    rates, Nphi, hLen, P, th, tx, nch = R4, 32, 250, 4, np.complex64, np.float32, 4
    x_len, piece = 700, 97
    H, PN, x = _banks(pkg, 5150, Nphi, hLen, P, x_len, th, tx, nch)
    pieces = _chunks(x_len, piece)
    xd, base = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(PN)).cuda()
    _env(monkeypatch, multi)
    f = pkg.FIRFilter.per_channel_rates_farrow(np.ascontiguousarray(H[0].real), rates, Nphi, P).bind(tx, nch)
    kept, ys, cnts = [], [], []
    for i, (a, b) in enumerate(pieces):
        PN_d = (base * complex(math.cos(0.3 * i), math.sin(0.3 * i)) + 0.003 * torch.roll(base, shifts=i + 1, dims=1)).contiguous()      # a rotated prototype
        f.set_channel_pnfb_ctaps_device(PN_d)
        y = torch.zeros((nch, f.outputlength_bound(b - a)), dtype=torch.complex64, device="cuda")
        cnt = torch.zeros(nch, dtype=torch.int64, device="cuda")
        f._filt_into_rates(y, xd[:, a:b], counts=cnt)                       # (returns without waiting; the counts stay on the device)
        kept.append(PN_d), ys.append(y), cnts.append(cnt)
    assert f.last_kernel_name() == (MULTI if multi else GENERIC)
    values = [p.cpu().numpy() for p in kept]                                # only now does the host learn anything
    got = [(y.cpu().numpy(), c.cpu().numpy()) for y, c in zip(ys, cnts)]
    assert len({v.tobytes() for v in values}) == len(pieces)
    twin = pkg.FIRFilter.per_channel_rates_farrow(np.ascontiguousarray(H[0].real), rates, Nphi, P).bind(tx, nch)
    refs = [None] * nch
    for i, (a, b) in enumerate(pieces):
        twin.set_channel_pnfb_ctaps(values[i])
        yt = torch.zeros((nch, twin.outputlength_bound(b - a)), dtype=torch.complex64, device="cuda")
        counts = twin.filt_into(yt, xd[:, a:b])
        assert list(got[i][1]) == list(counts), (i, list(got[i][1]), list(counts))
        yth = yt.cpu().numpy()
        for c in range(nch):
            old = refs[c]
            refs[c] = _restated(values[i][c], hLen, th, rates[c], Nphi, P, tx, state=None if old is None else (old.inputDeficit, old.phiAccumulator, old.xIdx),
                                hist=None if old is None else old.history_array())
            want = refs[c].filt(x[c, a:b], scalar=False)
            assert counts[c] == len(want), (i, c)
            assert_bit_equal(got[i][0][c, :counts[c]], yth[c, :counts[c]], f"piece {i}, channel {c}: device installs against host installs")
            assert_bit_equal(got[i][0][c, :counts[c]], want, f"piece {i}, channel {c}: against the restatement")
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [_state5(s) + (s.last_count,) for s in twin.channel_states]
    _check_end(f, [_rstate5(r) for r in refs], [r.history_array() for r in refs], "after the loop")
    for g, w in zip(_queries(f), _queries(twin)):
        assert_bit_equal(g, w, "banks after the loop")
    f.close(), twin.close()


# ---- installs between calls -----------------------------------------------------------------------------------------------------------
def _oracle_prefix(pkg, O, taps_of, rates, Nphi, P, x, tx, pieces):
    """the real-tap filter's outputs over `pieces` (the oracle on the library's fit), and per channel the (inputDeficit, phiAccumulator,
    xIdx) and history reached"""
    from test_gpu_rates_farrow import _oracle
    O.set_fused(False)
    outs, states, hists = [], [], []
    for c, r in enumerate(rates):
        ref = _oracle(pkg, O, taps_of(c), r, Nphi, P, tx)
        outs.append([ref.filt(x[c, a:b]) for a, b in pieces])
        st = ref.state
        states.append((int(st.inputDeficit), float(st.phiAccumulator), int(st.xIdx)))
        hists.append(np.array(ref.history))
    return outs, states, hists


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=["real-x", "complex-x"])
@pytest.mark.parametrize("start", ["shared", "real-banks", "complex", "complex-and-rates"])
def test_installs_between_calls(pkg, O, monkeypatch, torch_cuda, start, tx, multi):
    """700 samples in 97-sample pieces; after the third piece the filter -- on the one shared real bank, on a real bank per channel, or
    on other complex banks (with and without set_channel_rates in the same gap) -- receives complex banks.  The reference behind the
    switch is the restatement given the state and the history reached so far.  Then reset() keeps the complex taps and the rates, and
    set_channel_states, set_channel_rates and set_channel_rates_device work as before."""
    torch = torch_cuda
    rates, Nphi, hLen, P, x_len, rt, ct = R4, 32, 250, 4, 700, np.float32, np.complex64
    rates_after = [1.37, 0.5, 2.123, 3.01] if start == "complex-and-rates" else rates
    H1, PN1, x = _banks(pkg, 61, Nphi, hLen, P, x_len, ct, tx, 4)
    H0c, PN0, _ = _banks(pkg, 62, Nphi, hLen, P, x_len, ct, tx, 4)
    H0 = np.ascontiguousarray(H0c.real + H0c.imag).astype(rt)                # the real taps in force before the switch
    pieces = _chunks(x_len, 97)
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, multi)
    if start.startswith("complex"):
        refs = [_restated(PN0[c], hLen, ct, r, Nphi, P, tx) for c, r in enumerate(rates)]
        before = [[ref.filt(x[c, a:b], scalar=False) for a, b in pieces[:3]] for c, ref in enumerate(refs)]
        reached = [(ref.inputDeficit, ref.phiAccumulator, ref.xIdx) for ref in refs]
        hists = [ref.history_array() for ref in refs]
        f = pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(H0c, rates, Nphi, P, pnfb=PN0).bind(tx, 4)
        name_before = MULTI if multi else GENERIC
    else:
        taps_of = (lambda c: H0[0]) if start == "shared" else (lambda c: H0[c])
        before, reached, hists = _oracle_prefix(pkg, O, taps_of, rates, Nphi, P, x, tx, pieces[:3])
        f = pkg.FIRFilter.per_channel_rates_farrow(np.array(H0[0]), rates, Nphi, P).bind(tx, 4)
        if start == "real-banks":
            f.set_channel_taps_farrow(H0)
        name_before = (REAL if start == "shared" else REAL_BANK)[multi]
        assert f.output_dtype == np.dtype(tx)
    after_refs = [_restated(PN1[c], hLen, ct, r, Nphi, P, tx, state=reached[c], hist=hists[c]) for c, r in enumerate(rates_after)]
    for i, (a, b) in enumerate(pieces):
        if i == 3:
            was = [_state5(s) for s in f.channel_states]
            hist_was = f.history.copy()
            assert [(s[0], s[1], s[4]) for s in was] == reached
            if start == "complex-and-rates":
                f.set_channel_rates(rates_after)
            f.set_channel_pnfb_ctaps(PN1)
            assert [_state5(s) for s in f.channel_states] == was             # accumulator, deficit and history stay
            assert [s.rate for s in f.channel_states] == list(rates_after)
            assert_bit_equal(f.history, hist_was, "history across set_channel_pnfb_ctaps")
            assert f.output_dtype == np.dtype(np.complex64)                  # a real-sample filter's outputs flip to complex
        ys = f.filt(xd[:, a:b])
        for c in range(4):
            want = before[c][i] if i < 3 else after_refs[c].filt(x[c, a:b], scalar=False)
            got = ys[c].cpu().numpy()
            assert got.dtype == want.dtype, (i, c)
            assert_bit_equal(got, want, f"{start}: piece {i}, channel {c}")
        assert f.last_kernel_name() == (name_before if i < 3 else (MULTI if multi else GENERIC))
    _check_end(f, [_rstate5(r) for r in after_refs], [r.history_array() for r in after_refs], f"{start}: after the switch")
    # going back is refused, and leaves everything in place
    for call, arg in ((f.set_channel_taps_farrow, H0), (f.set_channel_pnfb, np.zeros((4, 8, P + 1)))):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call(arg)
        assert e.value.code == 5 and "going back to real taps is left out" in str(e.value)
    assert f._lib.mrhip_set_numerics(f._handle, pkg.NUMERICS_FUSED) == 5     # as on every complex-tap filter
    assert "no FUSED form is defined for complex taps" in f._lib.mrhip_last_error().decode()
    # reset keeps the complex taps and the rates; the states and the rates can be set as before
    f.reset()
    assert [(s.rate,) + _state5(s) + (s.last_count,) for s in f.channel_states] == [(r, 1, 1.0, 1, 0.0, 1, 0) for r in rates_after] and not f.history.any()
    assert_bit_equal(f.pnfb(), np.array(PN1), "the banks after reset")
    new_rates = [1.37, 0.5, 2.123, 3.01]
    deficits, accs = [1, 3, 1, 2], [1.0, 7.25, 32.5, 2.0]
    f.set_channel_states(deficits, accs)
    f.set_channel_rates(new_rates)
    fresh = [_restated(PN1[c], hLen, ct, r, Nphi, P, tx, state=(deficits[c], accs[c])) for c, r in enumerate(new_rates)]
    ys = f.filt(xd[:, :333])
    for c in range(4):
        assert_bit_equal(ys[c].cpu().numpy(), fresh[c].filt(x[c, :333], scalar=False), f"{start}: after reset, states and rates: channel {c}")
    dev_rates = [2.0, 0.75, 1.1, 0.3]
    f.set_channel_rates_device(torch.tensor(dev_rates, dtype=torch.float64, device="cuda"), 0.25, 2.5)
    again = [_restated(PN1[c], hLen, ct, r, Nphi, P, tx, state=(fresh[c].inputDeficit, fresh[c].phiAccumulator, fresh[c].xIdx), hist=fresh[c].history_array())
             for c, r in enumerate(dev_rates)]
    ys = f.filt(xd[:, 333:])
    for c in range(4):
        assert_bit_equal(ys[c].cpu().numpy(), again[c].filt(x[c, 333:], scalar=False), f"{start}: after set_channel_rates_device: channel {c}")
    assert f.last_kernel_name() == (MULTI if multi else GENERIC)
    _check_end(f, [_rstate5(r) for r in again], [r.history_array() for r in again], f"{start}: at the end")
    f.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _poisoned(torch, dtype, nch, cap):
    y = torch.empty((nch, cap), dtype=dtype, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    return y


@pytest.mark.parametrize("installed", ["shared-bank", "real-banks", "complex-banks"])
def test_refusals_leave_the_filter_as_it_was(pkg, monkeypatch, torch_cuda, installed):
    """every refusal of the three calls through the C symbols, in the header's order, and through Python, on a filter that still holds the
    one shared bank, on one with real banks and on one that holds complex banks: state, history, banks and the next call's outputs are the
    untouched twin's"""
    torch = torch_cuda
    lib = pkg.load_library()
    rates, Nphi, hLen, P, n, tx = R3, 32, 250, 4, 300, np.float32
    T = 8
    Hc, PN, x = _banks(pkg, 91, Nphi, hLen, P, 2 * n, np.complex64, tx, 3)
    other_H, other_PN, _ = _banks(pkg, 92, Nphi, hLen, P, 2 * n, np.complex64, tx, 3)
    other_H, other_PN = np.array(other_H), np.array(other_PN)
    Hr = np.ascontiguousarray(Hc.real)
    xd, pd = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(other_PN).cuda()
    _env(monkeypatch, False)

    def make():
        g = pkg.FIRFilter.per_channel_rates_farrow(np.array(Hr[0]), rates, Nphi, P).bind(tx, 3)
        if installed == "real-banks":
            g.set_channel_taps_farrow(Hr)
        elif installed == "complex-banks":
            g.set_channel_pnfb_ctaps(PN)
        return g

    f, twin = make(), make()
    kernel = {"shared-bank": REAL[False], "real-banks": REAL_BANK[False], "complex-banks": GENERIC}[installed]
    firsts = [g.filt(xd[:, :n]) for g in (f, twin)]
    assert f.last_kernel_name() == kernel
    hnd = f._handle
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(rc, code, *texts):
        assert rc == code, (rc, code, texts)
        msg = lib.mrhip_last_error().decode()
        assert all(t in msg for t in texts), msg

    arb = pkg.FIRFilter.per_channel_rates(np.array(Hr[0]), rates, Nphi).bind(tx, 3)
    one = pkg.FIRFilter(np.array(Hr[0]), 2.123, Nphi, P).bind(tx, 3)
    bank = pkg.FIRFilter.per_channel_complex_taps_farrow(other_H, 2.123, Nphi, P).bind(tx, 3)
    fused = pkg.FIRFilter.per_channel_rates_farrow(np.array(Hr[0]), rates, Nphi, P, numerics=pkg.NUMERICS_FUSED).bind(tx, 3)
    takes = " takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb"
    # mrhip_set_channel_ctaps_farrow
    who, call, good = "mrhip_set_channel_ctaps_farrow", lib.mrhip_set_channel_ctaps_farrow, ptr(other_H)
    refused(call(None, good, hLen, 2), 1, who + ": NULL filter")
    refused(call(arb._handle, None, hLen - 1, 0), 1, who + ":", "mrhip_create_arbitrary_rates takes mrhip_set_channel_ctaps")      # the kind goes first
    for g in (one, bank):
        refused(call(g._handle, None, hLen - 1, 0), 1, who + takes)
    refused(call(hnd, None, hLen - 1, 7), 1, who + ": h is NULL")                                       # h before hLen before the dtype
    refused(call(hnd, good, hLen - 1, 7), 1, who + ": hLen")
    refused(call(hnd, good, hLen + 1, 2), 1, who + ": hLen")
    refused(call(hnd, good, hLen, 7), 1, who + ": bad tap dtype")
    refused(call(hnd, good, hLen, -1), 1, who + ": bad tap dtype")
    refused(call(hnd, good, hLen, 0), 1, who + ":", "mrhip_set_channel_taps_farrow")
    refused(call(hnd, good, hLen, 1), 1, who + ":", "mrhip_set_channel_taps_farrow")
    refused(call(hnd, good, hLen, 3), 1, who + ":", "the complex type of the filter's tap precision")
    refused(call(fused._handle, good, hLen, 3), 1, who + ":", "the complex type of the filter's tap precision")      # the dtype before the numerics
    refused(call(fused._handle, good, hLen, 2), 5, who + ":", "FUSED")
    # the two pnfb calls
    host_call = lambda h_, p_, t_, o_: lib.mrhip_set_channel_pnfb_ctaps(h_, p_, t_, o_)
    dev_call = lambda h_, p_, t_, o_: lib.mrhip_set_channel_pnfb_ctaps_device(h_, p_, t_, o_, stream)
    for call, who, good in ((host_call, "mrhip_set_channel_pnfb_ctaps", ptr(other_PN)), (dev_call, "mrhip_set_channel_pnfb_ctaps_device", C.c_void_p(pd.data_ptr()))):
        refused(call(None, good, T, P), 1, who + ": NULL filter")
        refused(call(arb._handle, None, T - 1, P), 1, who + ":", "mrhip_create_arbitrary_rates takes mrhip_set_channel_ctaps")
        for g in (one, bank):
            refused(call(g._handle, None, T - 1, P), 1, who + takes)
        refused(call(hnd, None, T - 1, P), 1, who + ": pnfb is NULL")
        refused(call(hnd, good, T - 1, P), 1, who + ": tapsPerPhi and polyorder")
        refused(call(hnd, good, T, P + 1), 1, who + ": tapsPerPhi and polyorder")
        refused(call(fused._handle, good, T, P - 1), 1, who + ": tapsPerPhi and polyorder")              # the lengths before the numerics
        refused(call(fused._handle, good, T, P), 5, who + ":", "FUSED")
    # a capturing stream: status 5, nothing captured
    gr, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device="cuda")
    with torch.cuda.graph(gr, stream=s):
        scratch.add_(1.0)                                                   # (so that the graph is not empty)
        rc = lib.mrhip_set_channel_pnfb_ctaps_device(hnd, C.c_void_p(pd.data_ptr()), T, P, C.c_void_p(s.cuda_stream))
        msg = lib.mrhip_last_error().decode()
    torch.cuda.synchronize()
    assert rc == 5 and "captur" in msg and "mrhip_set_channel_pnfb_ctaps_device" in msg, (rc, msg)
    # what answered complex taps with "left out" still does, word for word; a filter with complex banks refuses going back
    refused(lib.mrhip_set_channel_ctaps(hnd, ptr(other_H), hLen, 2), 5, "mrhip_set_channel_ctaps: complex taps with per-channel rates for FIRFarrow are left out")
    refused(lib.mrhip_set_channel_ctaps_device(hnd, C.c_void_p(pd.data_ptr()), hLen, 2, stream), 5, "mrhip_set_channel_ctaps_device: complex taps with per-channel rates for FIRFarrow are left out")
    real_pn = np.ascontiguousarray(other_PN.real)
    rd = torch.from_numpy(real_pn).cuda()
    if installed != "complex-banks":
        refused(lib.mrhip_set_channel_taps_farrow(hnd, ptr(other_H), hLen, 2), 5, "mrhip_set_channel_taps_farrow: complex taps with per-channel rates are left out")
    else:
        refused(lib.mrhip_set_channel_taps_farrow(hnd, ptr(Hr), hLen, 0), 5, "mrhip_set_channel_taps_farrow:", "going back to real taps is left out")
        refused(lib.mrhip_set_channel_pnfb(hnd, ptr(real_pn), T, P), 5, "mrhip_set_channel_pnfb:", "going back to real taps is left out")
        refused(lib.mrhip_set_channel_pnfb_device(hnd, C.c_void_p(rd.data_ptr()), T, P, stream), 5, "mrhip_set_channel_pnfb_device:", "going back to real taps is left out")
    # the Python methods: wrong shape / dtype / device class / kind / numerics, and no mirror moved
    mirror = lambda g: (None if g._chan_farrow is None else (g._chan_farrow[0], g._chan_farrow[1].tobytes()), g._farrow_ctaps)
    was = mirror(f)
    bad = [(lambda: f.set_channel_ctaps_farrow(other_H[:2]), 1), (lambda: f.set_channel_ctaps_farrow(other_H[:, :-1]), 1),
           (lambda: f.set_channel_ctaps_farrow(other_H.real.copy()), 1), (lambda: f.set_channel_ctaps_farrow(other_H.astype(np.complex128)), 1),
           (lambda: f.set_channel_pnfb_ctaps(other_PN[:2]), 1), (lambda: f.set_channel_pnfb_ctaps(other_PN[:, :, :-1]), 1), (lambda: f.set_channel_pnfb_ctaps(real_pn), 1),
           (lambda: f.set_channel_pnfb_ctaps_device(pd[:2]), 1), (lambda: f.set_channel_pnfb_ctaps_device(pd[:, :-1]), 1), (lambda: f.set_channel_pnfb_ctaps_device(rd), 1),
           (lambda: f.set_channel_pnfb_ctaps_device(pd.to(torch.complex64)), 1), (lambda: f.set_channel_pnfb_ctaps_device(pd.cpu()), 1),
           (lambda: f.set_channel_pnfb_ctaps_device(other_PN), 1), (lambda: f.set_channel_pnfb_ctaps_device(pd.transpose(1, 2).contiguous().transpose(1, 2)), 1),
           (lambda: one.set_channel_ctaps_farrow(other_H), 1), (lambda: one.set_channel_pnfb_ctaps_device(pd), 1), (lambda: bank.set_channel_pnfb_ctaps(other_PN), 1),
           (lambda: arb.set_channel_ctaps_farrow(other_H), 1), (lambda: arb.set_channel_pnfb_ctaps(other_PN), 1), (lambda: arb.set_channel_pnfb_ctaps_device(pd), 1),
           (lambda: f.set_channel_ctaps(other_H), 5), (lambda: f.set_channel_ctaps_device(pd), 5),
           (lambda: fused.set_channel_ctaps_farrow(other_H), 5), (lambda: fused.set_channel_pnfb_ctaps(other_PN), 5), (lambda: fused.set_channel_pnfb_ctaps_device(pd), 5)]
    for i, (call, code) in enumerate(bad):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == code, i
    assert mirror(f) == was and mirror(fused) == (None, False) and mirror(arb) == (None, False) and arb._chan_ctaps is None
    # nothing moved: kernel, banks, output type, states and the next call's outputs are the untouched twin's
    assert f.output_dtype == twin.output_dtype == np.dtype(np.complex64 if installed == "complex-banks" else np.float32)
    assert [_state5(s_) + (s_.rate, s_.delta, s_.last_count) for s_ in f.channel_states] == [_state5(s_) + (s_.rate, s_.delta, s_.last_count) for s_ in twin.channel_states]
    for g, w in zip(_queries(f), _queries(twin)):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert_bit_equal(g, w, "banks after the refused calls")
    ya, yb = f.filt(xd[:, n:]), twin.filt(xd[:, n:])
    assert f.last_kernel_name() == twin.last_kernel_name() == kernel
    for c in range(3):
        assert_bit_equal(firsts[0][c].cpu().numpy(), firsts[1][c].cpu().numpy(), f"first call, channel {c}")
        assert_bit_equal(ya[c].cpu().numpy(), yb[c].cpu().numpy(), f"the call after the refusals, channel {c}")
    assert_bit_equal(f.history, twin.history, "history after the refusals")
    # a real-sample filter with complex banks refuses a real y, before anything is enqueued
    if installed == "complex-banks":
        y = _poisoned(torch, torch.float32, 3, 2 * f.outputlength_bound(n))
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.filt_into(y, xd[:, :n])
        assert e.value.code == 1 and (y.view(torch.uint8) == POISON).all().item()
    # FUSED is refused before the install (above: the filter `fused`) and after it
    if installed == "complex-banks":
        refused(lib.mrhip_set_numerics(twin._handle, pkg.NUMERICS_FUSED), 5, "no FUSED form is defined for complex taps")
    for g in (arb, one, bank, fused, f, twin):
        g.close()


# ---- write only your own outputs: a checker per row -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "A", "B", "C"])
@pytest.mark.parametrize("types", [(np.complex64, np.float32), (np.complex128, np.complex64)], ids=["c64", "c128"])
@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, monkeypatch, torch_cuda, multi, types, layout):
    torch = torch_cuda
    th, tx = types
    rates, Nphi, hLen, P = R4, 32, 250, 4
    sizes = [257, 5, 40, 300]
    x_len = sum(sizes)
    H, PN, x = _banks(pkg, 31, Nphi, hLen, P, x_len, th, tx, 4)
    pieces = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
    refs = [_restated(PN[c], hLen, th, r, Nphi, P, tx) for c, r in enumerate(rates)]
    f = _filter(pkg, monkeypatch, H, PN, rates, Nphi, P, tx, multi)
    oy, _, ox = LAYOUTS[layout]
    xback = torch.zeros((4, ox + x_len + 3), dtype=_tt(torch, tx), device="cuda")
    xback[:, ox:ox + x_len] = torch.from_numpy(np.array(x)).cuda()
    saw_zero = False
    for i, (a, b) in enumerate(pieces):
        want = [r.filt(x[c, a:b], scalar=False) for c, r in enumerate(refs)]
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
    assert [_state5(s) for s in f.channel_states] == [_rstate5(r) for r in refs]
    f.close()
