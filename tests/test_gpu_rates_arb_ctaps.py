"""GPU tests of COMPLEX per-channel taps on the FIRArbitrary filter with per-channel rates (csrc/kernels_rates_arb_ctaps.hip):
mrhip_set_channel_ctaps and mrhip_set_channel_ctaps_device on a filter of mrhip_create_arbitrary_rates, FIRFilter.set_channel_ctaps(H),
.set_channel_ctaps_device(H) and FIRFilter.per_channel_complex_taps_and_rates(H, rates, Nphi) -- one
FIRFilter(H[c]::Vector{Complex}, rates[c], Nphi) per channel behind one filter object.

Bar (include/multirate_hip.h, "Complex per-channel taps with per-channel rates for FIRArbitrary"): for every channel c the outputs and
the count of every call, the end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx) and the history are BIT FOR BIT those of the
one-channel complex-tap filter fed x[c] -- tests/complex_taps_arb_restatement.py (pinned to the oracle by tests/test_complex_taps_arb_cpu.py),
for real samples also the untouched oracle by components (O.FIRFilter(real(H[c]), ...) and the same over imag, put together), and in one
case per kernel the GPU filters FIRFilter.complex_taps_arbitrary(H[c], rates[c], Nphi) -- on the universal kernel (reported as
arb_rates_ctaps_generic, MRHIP_FORCE_GENERIC=1) and on the tiled one (arb_rates_ctaps_tiled, MRHIP_ARB_RATES_CTAPS_TILED=1).  STRICT only;
no tolerance anywhere.  Row 0 of H is random complex, row 1 a single 1j at tap 0, row 2 -conj(reverse(row 0)), further rows random, and
the rows of x are all different: a swapped bank, a shared bank or an exchanged re / im fails.  The shapes are those of
tests/test_gpu_rates_arb.py, the smallest at which these kernels can go wrong.  The module also holds the write-only-own-outputs cases of
the two kernels (poisoned buffers of tests/output_bounds_cases.py, a checker per row).
"""
import ctypes as C
import math

import numpy as np
import pytest

from complex_taps_arb_restatement import ComplexTapsArbitraryRestated
from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, POISON, make_buffer, row_pad
from test_gpu_rates_arb import BANKS, CHUNKINGS, R1, R3, R4, R67, X_LENS, _assert_rows_only_written, _check_end, _chunks, _state5, _tt

pytestmark = pytest.mark.gpu

GENERIC, TILED = "arb_rates_ctaps_generic", "arb_rates_ctaps_tiled"
REAL = {False: "arb_rates_generic", True: "arb_rates_tiled"}               # the filter's kernels before the install: shared real taps ...
REAL_BANK = {False: "arb_rates_bank_generic", True: "arb_rates_bank_tiled"}  # ... and per-channel real taps
ALL_TYPES = [(th, tx) for th in (np.complex64, np.complex128) for tx in (np.float32, np.float64, np.complex64, np.complex128)]
FEW_TYPES = [(np.complex64, np.float32), (np.complex128, np.complex64)]
CASES = [((32, 250), t) for t in ALL_TYPES] + [(b, t) for b in BANKS if b != (32, 250) for t in FEW_TYPES]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _real_of(th):
    return np.float64 if np.dtype(th) == np.complex128 else np.float32


_SIGNALS = {}


def _signal(seed, Nphi, hLen, x_len, th, tx, nch):
    """tests/test_gpu_arb_bank_ctaps._signal scaled to about unit gain per phase: rows that tell channels and components apart"""
    key = (seed, Nphi, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, nch)
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        H = ((rng.standard_normal((nch, hLen)) + 1j * rng.standard_normal((nch, hLen))) * Nphi / max(hLen, 1)).astype(th)
        if nch > 1:
            H[1] = 0
            H[1, 0] = 1j
        if nch > 2:
            H[2] = -np.conj(H[0][::-1])
        x = rng.random((nch, x_len)) - 0.5
        if np.dtype(tx).kind == "c":
            x = x + 1j * (rng.random((nch, x_len)) - 0.5)
        x = x.astype(tx)
        assert len({x[c].tobytes() for c in range(nch)}) == nch
        H.setflags(write=False), x.setflags(write=False)
        _SIGNALS[key] = (H, x)
    return _SIGNALS[key]


def _restated(h, rate, Nphi, tx, state=None, hist=None):
    """the one-channel complex-tap filter, optionally handed a state (inputDeficit, phiAccumulator and, where it is to be compared
    afterwards, xIdx: a call on the short-input path leaves it where the last walk ended) and a history (samples of tx)"""
    r = ComplexTapsArbitraryRestated(np.array(h), float(rate), Nphi, tx)
    if state is not None:
        r.inputDeficit, r.phiAccumulator = int(state[0]), float(state[1])
        if len(state) > 2:
            r.xIdx = int(state[2])
        r.phiIdx = int(math.floor(r.phiAccumulator))
        r.alpha = r.phiAccumulator - r.phiIdx
    if hist is not None:
        assert len(hist) == r.historyLen
        r.history = [r._widen(v) for v in np.ascontiguousarray(hist, dtype=tx)]
    return r


def _rstate5(r):
    return (r.inputDeficit, r.phiAccumulator, r.phiIdx, r.alpha, r.xIdx)


_REFS = {}


def _reference(seed, rates, Nphi, hLen, x_len, th, tx, how, lengths=None):
    """per channel, the restatement of H[c] at rates[c] fed x[c] in the pieces of `how`: (outputs [c][piece], end states [c],
    histories [c]); computed once per case and shared by the two kernels.  lengths: per piece, the channels' own lengths."""
    key = (seed, tuple(rates), Nphi, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), str(lengths))
    if key not in _REFS:
        H, x = _signal(seed, Nphi, hLen, x_len, th, tx, len(rates))
        refs = [_restated(H[c], r, Nphi, tx) for c, r in enumerate(rates)]
        pieces = _chunks(x_len, how)
        outs = [[r.filt(x[c, a:(b if lengths is None else a + lengths[i][c])], scalar=False) for i, (a, b) in enumerate(pieces)] for c, r in enumerate(refs)]
        _REFS[key] = (outs, [_rstate5(r) for r in refs], [r.history_array() for r in refs])
    return _REFS[key]


def _oracle_by_components(O, H, x, rates, Nphi, tx, pieces):
    """real samples: a complex tap times a real sample is two real products, so channel c is O.FIRFilter(real(H[c]), ...) and the same
    over imag(H[c]), put together -- the untouched oracle"""
    O.set_fused(False)
    outs = []
    for c, r in enumerate(rates):
        fr = O.FIRFilter(np.ascontiguousarray(H[c].real), float(r), Nphi, tx=tx)
        fi = O.FIRFilter(np.ascontiguousarray(H[c].imag), float(r), Nphi, tx=tx)
        row = []
        for a, b in pieces:
            yr, yi = fr.filt(x[c, a:b]), fi.filt(x[c, a:b])
            y = np.empty(len(yr), dtype=np.result_type(yr.dtype, np.complex64))
            y.real, y.imag = yr, yi
            row.append(y)
        outs.append(row)
    return outs


def _env(monkeypatch, tiled, grid=None):
    """the universal kernels (MRHIP_FORCE_GENERIC is read when the device object is created) or the tiled ones wherever their LDS plans
    fit (MRHIP_ARB_RATES_CTAPS_TILED=1; the two older switches for a filter before its complex install)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if tiled else "1")
    monkeypatch.setenv("MRHIP_ARB_RATES_CTAPS_TILED", "1")
    monkeypatch.setenv("MRHIP_ARB_RATES_BANK_TILED", "1")
    monkeypatch.setenv("MRHIP_ARB_RATES_TILED", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_ARB_RATES_CTAPS_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_ARB_RATES_CTAPS_GRID", str(grid))


def _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled, grid=None):
    _env(monkeypatch, tiled, grid)
    return pkg.FIRFilter.per_channel_complex_taps_and_rates(H, rates, Nphi).bind(tx, len(rates))


def _run_case(pkg, O, monkeypatch, torch, rates, Nphi, hLen, x_len, th, tx, tiled, chunkings=CHUNKINGS, grid=None, against_gpu=False):
    seed = 1000 * Nphi + hLen + x_len
    nch = len(rates)
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, nch)
    xd = torch.from_numpy(np.array(x)).cuda()
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        outs, states, hists = _reference(seed, rates, Nphi, hLen, x_len, th, tx, how)
        by_components = _oracle_by_components(O, H, x, rates, Nphi, tx, pieces) if np.dtype(tx).kind != "c" else None
        ones = [pkg.FIRFilter.complex_taps_arbitrary(np.array(H[c]), float(r), Nphi).bind(tx, 1) for c, r in enumerate(rates)] if against_gpu else None
        f = _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled, grid)
        want_dtype = outs[0][0].dtype
        assert want_dtype.kind == "c" and f.output_dtype == want_dtype
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
                if by_components is not None:
                    assert_bit_equal(yh[c, :want[c]], by_components[c][i], f"{what}: channel {c} against the oracle by components")
                if ones is not None:
                    assert_bit_equal(yh[c, :want[c]], np.atleast_1d(ones[c].filt(x[c, a:b])), f"{what}: channel {c} against the GPU one-channel filter")
            if b > a:
                assert f.last_kernel_name() == (TILED if tiled else GENERIC), what
            some_zero_beside_outputs = some_zero_beside_outputs or (min(want) == 0 < max(want))
        _check_end(f, states, hists, f"{name} x_len {x_len}")
        if rates is R4 and name == "prime" and x_len == 1500:
            assert some_zero_beside_outputs       # the short-input path of one channel while its neighbours produce outputs
        f.close()
        for g in ones or ():
            g.close()


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("bank,types", CASES, ids=[f"{b[0]}x{b[1]}-{np.dtype(t[0]).name}-{np.dtype(t[1]).name}" for b, t in CASES])
def test_every_channel_is_its_one_channel_filter(pkg, O, monkeypatch, torch_cuda, bank, types, tiled):
    (Nphi, hLen), (th, tx) = bank, types
    for rates in (R3, R4):
        for x_len in X_LENS:
            _run_case(pkg, O, monkeypatch, torch_cuda, rates, Nphi, hLen, x_len, th, tx, tiled)


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_every_channel_is_the_gpu_one_channel_filter(pkg, O, monkeypatch, torch_cuda, tiled):
    _run_case(pkg, O, monkeypatch, torch_cuda, R4, 32, 250, 1500, np.complex64, np.complex64, tiled, chunkings={"prime": 97}, against_gpu=True)


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("rates", [R67, R1], ids=["nch67", "nch1"])
def test_a_second_wave_of_the_schedule_kernel_and_one_channel(pkg, O, monkeypatch, torch_cuda, rates, tiled):
    for x_len in X_LENS:
        _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, x_len, np.complex64, np.float32, tiled)
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 3, 40, 1500, np.complex128, np.complex64, tiled, chunkings={"prime": 97})


@pytest.mark.parametrize("rates", [R4, R67], ids=["R4", "R67"])
@pytest.mark.parametrize("grid", [1, 2, 3, 2000])
def test_tiled_kernel_on_any_grid(pkg, O, monkeypatch, torch_cuda, grid, rates):
    """one workgroup for every tile, a few, and more workgroups than tiles (R4 at 1500 samples: 4 x 63 = 252 tiles, R67: 67 x 22 = 1474): a
    workgroup's run crosses several channels, in the 97-sample pieces also one whose count is 0 in that call"""
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, 1500, np.complex64, np.float32, True, chunkings={"whole": None, "prime": 97}, grid=grid)


RAGGED = [[1500, 0, 257, 1499], [1500, 1, 257, 1499], [0, 0, 0, 5], [3, 1500, 1500, 0]]      # (the second differs from the first in the zero-length channel only)


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=["real-x", "complex-x"])
def test_ragged_calls(pkg, monkeypatch, torch_cuda, tx, tiled):
    """mrhip_filt_device_rates_ragged: every channel against the restatement fed its own samples, a channel of length 0 among them"""
    torch = torch_cuda
    rates, Nphi, hLen, th = R4, 32, 250, np.complex64
    x_len, seed = 1500 * len(RAGGED), 4242
    H, x = _signal(seed, Nphi, hLen, x_len, th, tx, 4)
    xd = torch.from_numpy(np.array(x)).cuda()
    outs, states, hists = _reference(seed, rates, Nphi, hLen, x_len, th, tx, 1500, lengths=RAGGED)
    f = _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled)
    for i, lens in enumerate(RAGGED):
        bound = f.outputlength_bound(max(lens))
        y = torch.zeros((4, bound), dtype=torch.complex64, device="cuda")
        counts = f.filt_into(y, xd[:, 1500 * i:1500 * (i + 1)], lengths=lens)
        want = [len(outs[c][i]) for c in range(4)]
        assert list(counts) == want, (i, list(counts), want)
        yh = y.cpu().numpy()
        for c in range(4):
            assert_bit_equal(yh[c, :want[c]], outs[c][i], f"ragged call {i} {lens}: channel {c}")
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    _check_end(f, states, hists, "after the ragged calls")
    f.close()


# ---- switching mid-stream -----------------------------------------------------------------------------------------------------------
def _oracle_prefix(O, taps_of, rates, Nphi, x, tx, pieces):
    """the real-tap filter's outputs over `pieces` (the oracle), and per channel the (inputDeficit, phiAccumulator) and history reached"""
    O.set_fused(False)
    outs, states, hists = [], [], []
    for c, r in enumerate(rates):
        ref = O.FIRFilter(taps_of(c), float(r), Nphi, tx=tx)
        outs.append([ref.filt(x[c, a:b]) for a, b in pieces])
        st = ref.state
        states.append((int(st.inputDeficit), float(st.phiAccumulator), int(st.xIdx)))
        hists.append(np.array(ref.history))
    return outs, states, hists


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=["real-x", "complex-x"])
@pytest.mark.parametrize("start", ["shared", "host-taps", "device-taps", "complex"])
def test_switching_to_complex_taps_mid_stream(pkg, O, monkeypatch, torch_cuda, start, tx, tiled):
    """700 samples in 97-sample pieces; after the third piece the filter -- on shared real taps, on per-channel real taps installed from
    the host or from the device, or on other complex taps -- receives complex taps.  The reference behind the switch is the restatement
    given the state and the history reached so far.  Then reset() keeps the complex taps, and set_channel_states, set_channel_rates and
    set_channel_rates_device work as before."""
    torch = torch_cuda
    rates, Nphi, hLen, x_len, rt, ct = R4, 32, 250, 700, np.float32, np.complex64
    H1, x = _signal(61, Nphi, hLen, x_len, ct, tx, 4)
    H0c, _ = _signal(62, Nphi, hLen, x_len, ct, tx, 4)
    H0 = np.ascontiguousarray(H0c.real + H0c.imag).astype(rt)                # the real taps in force before the switch
    pieces = _chunks(x_len, 97)
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, tiled)
    # the reference in front of the switch and the state it reaches
    if start == "complex":
        refs = [_restated(H0c[c], r, Nphi, tx) for c, r in enumerate(rates)]
        before = [[ref.filt(x[c, a:b], scalar=False) for a, b in pieces[:3]] for c, ref in enumerate(refs)]
        reached = [(ref.inputDeficit, ref.phiAccumulator, ref.xIdx) for ref in refs]
        hists = [ref.history_array() for ref in refs]
        f = pkg.FIRFilter.per_channel_complex_taps_and_rates(H0c, rates, Nphi).bind(tx, 4)
        name_before = TILED if tiled else GENERIC
    else:
        taps_of = (lambda c: H0[0]) if start == "shared" else (lambda c: H0[c])
        before, reached, hists = _oracle_prefix(O, taps_of, rates, Nphi, x, tx, pieces[:3])
        f = pkg.FIRFilter.per_channel_rates(np.array(H0[0]), rates, Nphi).bind(tx, 4)
        if start == "host-taps":
            f.set_channel_taps(H0)
        elif start == "device-taps":
            f.set_channel_taps_device(torch.from_numpy(H0).cuda())
        name_before = (REAL if start == "shared" else REAL_BANK)[tiled]
        assert f.output_dtype == np.dtype(tx)
    after_refs = [_restated(H1[c], r, Nphi, tx, state=reached[c], hist=hists[c]) for c, r in enumerate(rates)]
    for i, (a, b) in enumerate(pieces):
        if i == 3:
            was = [_state5(s) for s in f.channel_states]
            hist_was = f.history.copy()
            assert [(s[0], s[1], s[4]) for s in was] == reached
            f.set_channel_ctaps(H1)
            assert [_state5(s) for s in f.channel_states] == was             # accumulator, deficit and history stay
            assert_bit_equal(f.history, hist_was, "history across set_channel_ctaps")
            assert f.output_dtype == np.dtype(np.complex64)                  # a real-sample filter's outputs flip to complex
        ys = f.filt(xd[:, a:b])
        for c in range(4):
            want = before[c][i] if i < 3 else after_refs[c].filt(x[c, a:b], scalar=False)
            got = ys[c].cpu().numpy()
            assert got.dtype == want.dtype, (i, c)
            assert_bit_equal(got, want, f"{start}: piece {i}, channel {c}")
        assert f.last_kernel_name() == (name_before if i < 3 else (TILED if tiled else GENERIC))
    _check_end(f, [_rstate5(r) for r in after_refs], [r.history_array() for r in after_refs], f"{start}: after the switch")
    # going back is refused, and leaves everything in place
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.set_channel_taps(H0)
    assert e.value.code == 5 and "going back to real taps is left out" in str(e.value)
    assert f._lib.mrhip_set_numerics(f._handle, pkg.NUMERICS_FUSED) == 5     # as on every complex-tap filter
    assert "no FUSED form is defined for complex taps" in f._lib.mrhip_last_error().decode()
    # reset keeps the complex taps; the states and the rates can be set as before
    f.reset()
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [(1, 1.0, 1, 0.0, 1, 0)] * 4 and not f.history.any()
    new_rates = [1.37, 0.5, 2.123, 3.01]
    deficits, accs = [1, 3, 1, 2], [1.0, 7.25, 32.5, 2.0]
    f.set_channel_states(deficits, accs)
    f.set_channel_rates(new_rates)
    fresh = [_restated(H1[c], r, Nphi, tx, state=(deficits[c], accs[c])) for c, r in enumerate(new_rates)]
    ys = f.filt(xd[:, :333])
    for c in range(4):
        assert_bit_equal(ys[c].cpu().numpy(), fresh[c].filt(x[c, :333], scalar=False), f"{start}: after reset, states and rates: channel {c}")
    dev_rates = [2.0, 0.75, 1.1, 0.3]
    f.set_channel_rates_device(torch.tensor(dev_rates, dtype=torch.float64, device="cuda"), 0.25, 2.5)
    again = [_restated(H1[c], r, Nphi, tx, state=(fresh[c].inputDeficit, fresh[c].phiAccumulator, fresh[c].xIdx), hist=fresh[c].history_array()) for c, r in enumerate(dev_rates)]
    ys = f.filt(xd[:, 333:])
    for c in range(4):
        assert_bit_equal(ys[c].cpu().numpy(), again[c].filt(x[c, 333:], scalar=False), f"{start}: after set_channel_rates_device: channel {c}")
    assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    _check_end(f, [_rstate5(r) for r in again], [r.history_array() for r in again], f"{start}: at the end")
    f.close()


# ---- the install from device memory -------------------------------------------------------------------------------------------------
def _queries(f):
    return (f.taps(0), f.taps(1), f.tapsforphase(1.0), f.tapsforphase(2.375))


@pytest.mark.parametrize("th", [np.complex64, np.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("bank", [(4, 4), (3, 40), (32, 1024), (4, 5000)], ids=["4x4", "3x40", "32x1024", "row-beyond-lds"])
def test_device_install_equals_host_install(pkg, monkeypatch, torch_cuda, bank, th):
    """taps() and tapsforphase read back after set_channel_ctaps_device, and all outputs, are bit-equal to the host install of the same
    matrix; (4, 5000): a row of 5000 pairs, 40 000 or 80 000 bytes, is longer than the 32 KiB the build kernel stages in LDS"""
    torch = torch_cuda
    Nphi, hLen = bank
    rt, tx, nch = _real_of(th), np.float32, 3
    x_len = 300
    H, x = _signal(7000 + hLen, Nphi, hLen, x_len, th, tx, nch)
    H2, _ = _signal(7001 + hLen, Nphi, hLen, x_len, th, tx, nch)
    T = -(-hLen // Nphi)
    xd = torch.from_numpy(np.array(x)).cuda()
    _env(monkeypatch, False)
    placeholder = np.ascontiguousarray(H[0].real)
    host = pkg.FIRFilter.per_channel_rates(placeholder, R3, Nphi).bind(tx, nch)
    dev = pkg.FIRFilter.per_channel_rates(placeholder, R3, Nphi).bind(tx, nch)
    assert placeholder.dtype == rt and host.taps(0).shape == (T, Nphi)
    for k, M in enumerate((H, H2)):                                          # the first install allocates, the second reuses the banks
        host.set_channel_ctaps(M)
        dev.set_channel_ctaps_device(torch.from_numpy(np.array(M)).cuda())
        assert dev.output_dtype == host.output_dtype == np.dtype(np.result_type(th, tx))
        for g, w, name in zip(_queries(dev), _queries(host), ("pfb", "dpfb", "tapsforphase(1.0)", "tapsforphase(2.375)")):
            assert g.dtype == np.dtype(th) and g.shape == w.shape == ((nch, T, Nphi) if name.endswith("pfb") else (nch, T))
            assert_bit_equal(g, w, f"install {k}: {name}")
        # the host banks are those of the one-channel restatement: pfb[i, phi] of channel c
        for c in range(nch):
            r = ComplexTapsArbitraryRestated(np.array(M[c]), R3[c], Nphi, tx)
            assert_bit_equal(host.taps(0)[c], r.pfb, f"install {k}: pfb of channel {c}")
            assert_bit_equal(host.taps(1)[c], r.dpfb, f"install {k}: dpfb of channel {c}")
            assert_bit_equal(host.tapsforphase(2.375)[c], r.tapsforphase(2.375), f"install {k}: tapsforphase of channel {c}")
        a, b = (0, 150) if k == 0 else (150, 300)
        ya, yb = host.filt(xd[:, a:b]), dev.filt(xd[:, a:b])
        for c in range(nch):
            assert_bit_equal(yb[c].cpu().numpy(), ya[c].cpu().numpy(), f"install {k}: outputs of channel {c}")
        assert dev.last_kernel_name() == host.last_kernel_name() == GENERIC
    assert [_state5(s) for s in dev.channel_states] == [_state5(s) for s in host.channel_states]
    assert_bit_equal(dev.history, host.history, "history")
    host.close(), dev.close()


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_a_loop_of_device_installs_that_never_meets_the_host(pkg, monkeypatch, torch_cuda, tiled):
    """the tracker's loop: every piece installs new complex taps from device memory and filters, nothing is read back until the loop is
    over (the first install allocates and may wait once; every later one enqueues a kernel and returns) -- then every piece equals the
    twin driven through set_channel_ctaps with the same values, and the restatement rebuilt per piece"""
    torch = torch_cuda
    rates, Nphi, hLen, th, tx, nch = R4, 32, 250, np.complex64, np.float32, 4
    x_len, piece = 700, 97
    H0, x = _signal(5150, Nphi, hLen, x_len, th, tx, nch)
    pieces = _chunks(x_len, piece)
    xd, base = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(H0)).cuda()
    _env(monkeypatch, tiled)
    f = pkg.FIRFilter.per_channel_rates(np.ascontiguousarray(H0[0].real), rates, Nphi).bind(tx, nch)
    kept, ys, cnts = [], [], []
    for i, (a, b) in enumerate(pieces):
        H_d = (base * complex(math.cos(0.3 * i), math.sin(0.3 * i)) + 0.003 * torch.roll(base, shifts=i + 1, dims=-1)).contiguous()      # a rotated prototype
        f.set_channel_ctaps_device(H_d)
        y = torch.zeros((nch, f.outputlength_bound(b - a)), dtype=torch.complex64, device="cuda")
        cnt = torch.zeros(nch, dtype=torch.int64, device="cuda")
        f._filt_into_rates(y, xd[:, a:b], counts=cnt)                       # (returns without waiting; the counts stay on the device)
        kept.append(H_d), ys.append(y), cnts.append(cnt)
    assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    values = [h.cpu().numpy() for h in kept]                                # only now does the host learn anything
    got = [(y.cpu().numpy(), c.cpu().numpy()) for y, c in zip(ys, cnts)]
    assert len({h.tobytes() for h in values}) == len(pieces)
    twin = pkg.FIRFilter.per_channel_rates(np.ascontiguousarray(H0[0].real), rates, Nphi).bind(tx, nch)
    refs = [None] * nch
    for i, (a, b) in enumerate(pieces):
        twin.set_channel_ctaps(values[i])
        yt = torch.zeros((nch, twin.outputlength_bound(b - a)), dtype=torch.complex64, device="cuda")
        counts = twin.filt_into(yt, xd[:, a:b])
        assert list(got[i][1]) == list(counts), (i, list(got[i][1]), list(counts))
        yth = yt.cpu().numpy()
        for c in range(nch):
            old = refs[c]
            refs[c] = _restated(values[i][c], rates[c], Nphi, tx, state=None if old is None else (old.inputDeficit, old.phiAccumulator, old.xIdx),
                                hist=None if old is None else old.history_array())
            want = refs[c].filt(x[c, a:b], scalar=False)
            assert counts[c] == len(want), (i, c)
            assert_bit_equal(got[i][0][c, :counts[c]], yth[c, :counts[c]], f"piece {i}, channel {c}: device installs against host installs")
            assert_bit_equal(got[i][0][c, :counts[c]], want, f"piece {i}, channel {c}: against the restatement")
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [_state5(s) + (s.last_count,) for s in twin.channel_states]
    _check_end(f, [_rstate5(r) for r in refs], [r.history_array() for r in refs], "after the loop")
    for g, w in zip(_queries(f), _queries(twin)):
        assert_bit_equal(g, w, "taps after the loop")
    f.close(), twin.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _poisoned(torch, dtype, nch, cap):
    y = torch.empty((nch, cap), dtype=dtype, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    return y


@pytest.mark.parametrize("installed", ["shared-taps", "real-banks", "complex-banks"])
def test_refusals_leave_the_filter_as_it_was(pkg, monkeypatch, torch_cuda, installed):
    """every refusal of the two calls through the C symbols, in the header's order, and through Python, on a filter whose taps are still
    shared, on one with real banks and on one that holds complex banks: state, history, taps and the next call's outputs are the
    untouched twin's"""
    torch = torch_cuda
    lib = pkg.load_library()
    rates, Nphi, hLen, n, tx = R3, 32, 250, 300, np.float32
    Hc, x = _signal(91, Nphi, hLen, 2 * n, np.complex64, tx, 3)
    other = np.array(_signal(92, Nphi, hLen, 2 * n, np.complex64, tx, 3)[0])
    Hr = np.ascontiguousarray(Hc.real)
    xd, od = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(other).cuda()
    _env(monkeypatch, False)

    def make():
        g = pkg.FIRFilter.per_channel_rates(np.array(Hr[0]), rates, Nphi).bind(tx, 3)
        if installed == "real-banks":
            g.set_channel_taps(Hr)
        elif installed == "complex-banks":
            g.set_channel_ctaps(Hc)
        return g

    f, twin = make(), make()
    kernel = {"shared-taps": REAL[False], "real-banks": REAL_BANK[False], "complex-banks": GENERIC}[installed]
    firsts = [g.filt(xd[:, :n]) for g in (f, twin)]
    assert f.last_kernel_name() == kernel
    hnd = f._handle
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    host_call = lambda h_, p_, n_, t_: lib.mrhip_set_channel_ctaps(h_, p_, n_, t_)
    dev_call = lambda h_, p_, n_, t_: lib.mrhip_set_channel_ctaps_device(h_, p_, n_, t_, stream)

    def refused(rc, code, *texts):
        assert rc == code, (rc, code, texts)
        msg = lib.mrhip_last_error().decode()
        assert all(t in msg for t in texts), msg

    farrow = pkg.FIRFilter.per_channel_rates_farrow(np.array(Hr[0]), rates, Nphi, 4).bind(tx, 3)
    one = pkg.FIRFilter(np.array(Hr[0]), 2.123, Nphi).bind(tx, 3)
    bank = pkg.FIRFilter.per_channel_complex_taps_arbitrary(other, 2.123, Nphi).bind(tx, 3)
    fused = pkg.FIRFilter.per_channel_rates(np.array(Hr[0]), rates, Nphi, numerics=pkg.NUMERICS_FUSED).bind(tx, 3)
    for call, who, good in ((host_call, "mrhip_set_channel_ctaps", ptr(other)), (dev_call, "mrhip_set_channel_ctaps_device", C.c_void_p(od.data_ptr()))):
        refused(call(None, good, hLen, 2), 1, who + ": NULL filter")
        refused(call(farrow._handle, None, hLen - 1, 0), 5, who + ":", "complex taps with per-channel rates for FIRFarrow are left out")      # the kind goes first
        for g in (one, bank):
            refused(call(g._handle, None, hLen - 1, 0), 1, who + " takes a filter of mrhip_create_arbitrary_rates")
        refused(call(hnd, None, hLen - 1, 7), 1, who + ": h is NULL")                                   # h before hLen before the dtype
        refused(call(hnd, good, hLen - 1, 7), 1, who + ": hLen")
        refused(call(hnd, good, hLen + 1, 2), 1, who + ": hLen")
        refused(call(hnd, good, hLen, 7), 1, who + ": bad tap dtype")
        refused(call(hnd, good, hLen, -1), 1, who + ": bad tap dtype")
        refused(call(hnd, good, hLen, 0), 1, who + ":", "mrhip_set_channel_taps")
        refused(call(hnd, good, hLen, 1), 1, who + ":", "mrhip_set_channel_taps")
        refused(call(hnd, good, hLen, 3), 1, who + ":", "the complex type of the filter's tap precision")
        refused(call(fused._handle, good, hLen, 3), 1, who + ":", "the complex type of the filter's tap precision")      # the dtype before the numerics
        refused(call(fused._handle, good, hLen, 2), 5, who + ":", "FUSED")
    # a capturing stream: status 5, nothing captured
    gr, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device="cuda")
    with torch.cuda.graph(gr, stream=s):
        scratch.add_(1.0)                                                   # (so that the graph is not empty)
        rc = lib.mrhip_set_channel_ctaps_device(hnd, C.c_void_p(od.data_ptr()), hLen, 2, C.c_void_p(s.cuda_stream))
        msg = lib.mrhip_last_error().decode()
    torch.cuda.synchronize()
    assert rc == 5 and "captur" in msg and "mrhip_set_channel_ctaps_device" in msg, (rc, msg)
    # what answered a complex tap dtype with "left out" still does
    if installed != "complex-banks":
        refused(lib.mrhip_set_channel_taps(hnd, ptr(other), hLen, 2), 5, "complex taps with per-channel rates are left out")
        refused(lib.mrhip_set_channel_taps_device(hnd, C.c_void_p(od.data_ptr()), hLen, 2, stream), 5, "complex taps with per-channel rates are left out")
    else:
        refused(lib.mrhip_set_channel_taps(hnd, ptr(Hr), hLen, 0), 5, "mrhip_set_channel_taps:", "going back to real taps is left out")
        refused(lib.mrhip_set_channel_taps_device(hnd, C.c_void_p(od.data_ptr()), hLen, 0, stream), 5, "mrhip_set_channel_taps_device:", "going back to real taps is left out")
    refused(lib.mrhip_set_channel_taps_farrow(farrow._handle, ptr(other), hLen, 2), 5, "complex taps with per-channel rates are left out")
    # the Python methods: wrong shape / dtype / device class / kind / numerics, and no mirror moved
    mirror = None if f._chan_ctaps is None else f._chan_ctaps.tobytes()
    bad = [(lambda: f.set_channel_ctaps(other[:2]), 1), (lambda: f.set_channel_ctaps(other[:, :-1]), 1), (lambda: f.set_channel_ctaps(other.real.copy()), 1),
           (lambda: f.set_channel_ctaps(other.astype(np.complex128)), 1), (lambda: f.set_channel_ctaps_device(od[:2]), 1),
           (lambda: f.set_channel_ctaps_device(od[:, :-1]), 1), (lambda: f.set_channel_ctaps_device(od.real.contiguous()), 1),
           (lambda: f.set_channel_ctaps_device(od.to(torch.complex128)), 1), (lambda: f.set_channel_ctaps_device(od.cpu()), 1),
           (lambda: f.set_channel_ctaps_device(other), 1), (lambda: f.set_channel_ctaps_device(od.t().contiguous().t()), 1),
           (lambda: one.set_channel_ctaps(other), 1), (lambda: one.set_channel_ctaps_device(od), 1), (lambda: bank.set_channel_ctaps(other), 1),
           (lambda: farrow.set_channel_ctaps(other), 5), (lambda: farrow.set_channel_ctaps_device(od), 5),
           (lambda: fused.set_channel_ctaps(other), 5), (lambda: fused.set_channel_ctaps_device(od), 5)]
    for i, (call, code) in enumerate(bad):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == code, i
    assert (None if f._chan_ctaps is None else f._chan_ctaps.tobytes()) == mirror and fused._chan_ctaps is None and farrow._chan_ctaps is None
    # nothing moved: kernel, taps, output type, states and the next call's outputs are the untouched twin's
    assert f.output_dtype == twin.output_dtype == np.dtype(np.complex64 if installed == "complex-banks" else np.float32)
    assert [_state5(s_) + (s_.rate, s_.delta, s_.last_count) for s_ in f.channel_states] == [_state5(s_) + (s_.rate, s_.delta, s_.last_count) for s_ in twin.channel_states]
    for g, w in zip(_queries(f), _queries(twin)):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert_bit_equal(g, w, "taps after the refused calls")
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
    for g in (farrow, one, bank, fused, f, twin):
        g.close()


# ---- write only your own outputs: a checker per row -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "A", "B", "C"])
@pytest.mark.parametrize("types", [(np.complex64, np.float32), (np.complex128, np.complex64)], ids=["c64", "c128"])
@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, monkeypatch, torch_cuda, tiled, types, layout):
    torch = torch_cuda
    th, tx = types
    rates, Nphi, hLen = R4, 32, 250
    sizes = [257, 5, 40, 300]
    x_len = sum(sizes)
    H, x = _signal(31, Nphi, hLen, x_len, th, tx, 4)
    pieces = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
    refs = [_restated(H[c], r, Nphi, tx) for c, r in enumerate(rates)]
    f = _filter(pkg, monkeypatch, H, rates, Nphi, tx, tiled)
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
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        _assert_rows_only_written(backing, 4, cap, oy, pad, counts, want, f"{layout} piece {i} [{a}, {b})")
        saw_zero = saw_zero or (min(counts) == 0 < max(counts))
    assert saw_zero                                                         # a call in which one channel's count is 0
    assert [_state5(s) for s in f.channel_states] == [_rstate5(r) for r in refs]
    f.close()
