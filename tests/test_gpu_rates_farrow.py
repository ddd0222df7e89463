"""GPU tests of per-channel rates for FIRFarrow (csrc/kernels_rates_farrow.hip): FIRFilter.per_channel_rates_farrow(h, rates, Nphi,
polyorder), one FIRFilter(h, rates[c], Nphi, polyorder) per channel behind one filter object (mrhip_create_farrow_rates,
mrhip_create_farrow_rates_pnfb), and of rates that change between calls (mrhip_set_channel_rates) on both filters with per-channel
rates.

Bar (include/multirate_hip.h, "Per-channel rates for FIRFarrow"): for every channel c the outputs and the count of every call, the
end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx) and the history are BIT FOR BIT those of the oracle's
O.FIRFilter(h, rates[c], Nphi, tx=tx, polyorder=P, pnfb=fit) fed x[c] -- under STRICT and FUSED, on the universal kernel (reported as
farrow_rates_generic, MRHIP_FORCE_GENERIC=1) and on the multi kernel (farrow_rates_multi, MRHIP_FARROW_RATES_MULTI=1).  No tolerance
anywhere.  `fit` is the library's own per-row fit (mrhip_polyfit per row of taps2pfb(h, Nphi), rounded to the tap type), as in
tests/test_gpu_farrow_bank.py: the reference pins no bits of the fit, oracle and library must evaluate the same coefficients.  The
module also holds the write-only-own-outputs cases of the two kernels (poisoned buffers of tests/output_bounds_cases.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, POISON, backing_bytes, first_stray, make_buffer, row_pad

pytestmark = pytest.mark.gpu

R3 = [0.47, 1.0, 2.123]
R4 = [0.01, 32.0 / 3, 2.123, 2.123]      # a channel that writes nothing in most chunks; an exactly cycling rate; two equal rates
R67 = [0.3 + 0.05 * c for c in range(67)]  # a second wave of the schedule kernel, with idle lanes
R1 = [math.pi / 3]
X_LENS = [1, 5, 257, 1500]
# the multi kernel: a lane's four runs span 1024 outputs.  1030 samples at rate 1.0 end a channel's count just inside a second span;
# 2100 at 0.47 (988 outputs) leaves lanes with three live outputs of four, at 2.123 (4459: 363 in the fifth span) with two and one
X_LENS_MULTI = [1030, 2100]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
ALL_TYPES = [(th, tx) for th in (np.float32, np.float64) for tx in (np.float32, np.float64, np.complex64, np.complex128)]
FEW_TYPES = [(np.float32, np.float32), (np.float64, np.complex64)]
# (Nphi, hLen, polyorder): T = 1 (no history); 8; a non-power-of-two Nphi (T = 14); 8; 32.  polyorder 4 is the unrolled chain, every
# other one the runtime loop (polyorder + 1 <= Nphi: the banks of 3 and 4 phases take 1, 2 and 3)
SHAPES = [(4, 4, 1), (4, 30, 1), (4, 30, 3), (3, 40, 1), (3, 40, 2), (32, 250, 1), (32, 250, 6), (32, 1024, 4), (32, 1024, 6)]
CASES = [((32, 250, 4), t) for t in ALL_TYPES] + [(s, t) for s in SHAPES for t in FEW_TYPES]
GENERIC, MULTI = "farrow_rates_generic", "farrow_rates_multi"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _chunks(n, how):
    if how is None:
        return [(0, n)]
    if isinstance(how, int):
        return [(a, min(a + how, n)) for a in range(0, n, how)]
    out, pos = [], 0
    for c in how:
        if pos + c > n:
            break
        out.append((pos, pos + c))
        pos += c
    out.append((pos, n))
    return out


_SIGNALS = {}


def _signal(seed, Nphi, hLen, x_len, th, tx, rates):
    """one tap vector (about unit gain per phase) and one row of samples per channel; channels of EQUAL rate get equal rows, so their
    outputs must be bit-equal rows"""
    key = (seed, Nphi, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, tuple(rates))
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        h = (rng.standard_normal(hLen) * Nphi / max(hLen, 1)).astype(th)
        nch = len(rates)
        x = rng.random((nch, x_len)) - 0.5
        if np.dtype(tx).kind == "c":
            x = x + 1j * (rng.random((nch, x_len)) - 0.5)
        for c in range(nch):
            first = rates.index(rates[c])
            if first != c:
                x[c] = x[first]
        x = x.astype(tx)
        h.setflags(write=False), x.setflags(write=False)
        _SIGNALS[key] = (h, x)
    return _SIGNALS[key]


_FITS = {}


def _fit(pkg, O, h, Nphi, P):
    """pfb2pnfb (src/Filters.jl:311-321) with the library's per-row fit: one polynomial per row of taps2pfb(h, Nphi), ascending powers,
    stored in the tap type (values representable in it, held as Float64).  Computed once per tap vector."""
    key = (h.tobytes(), h.dtype.name, Nphi, P)
    if key not in _FITS:
        pfb = O.taps2pfb(h, Nphi)
        _FITS[key] = np.stack([pkg.polyfit(pfb[i].astype(np.float64), P).astype(h.dtype).astype(np.float64) for i in range(pfb.shape[0])])
    return _FITS[key]


def _oracle(pkg, O, h, rate, Nphi, P, tx):
    """the reference of one channel: the oracle's FIRFilter(h, rate, Nphi, polyorder = P) on the library's fit of h; P None: FIRArbitrary"""
    if P is None:
        return O.FIRFilter(h, float(rate), Nphi, tx=tx)
    return O.FIRFilter(h, float(rate), Nphi, tx=tx, polyorder=P, pnfb=_fit(pkg, O, h, Nphi, P))


def _state5(st):
    return (st.inputDeficit, st.phiAccumulator, st.phiIdx, st.alpha, st.xIdx)


_REFS = {}


def _reference(pkg, O, seed, rates, Nphi, hLen, P, x_len, th, tx, how, fused, start=None):
    """per channel, the oracle's filter fed x[c] in the pieces of `how`: (outputs [c][piece], end states [c], histories [c]); computed
    once per case and shared by the two kernels.  start: per-channel (inputDeficit, phiAccumulator)."""
    key = (seed, tuple(rates), Nphi, hLen, P, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), fused, str(start))
    if key not in _REFS:
        h, x = _signal(seed, Nphi, hLen, x_len, th, tx, rates)
        O.set_fused(fused)
        try:
            refs = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in rates]
            if start is not None:
                for r, (d, a) in zip(refs, start):
                    r.set_state(int(math.floor(a)), int(d), float(a))
            outs = [[r.filt(x[c, a:b]) for a, b in _chunks(x_len, how)] for c, r in enumerate(refs)]
        finally:
            O.set_fused(False)
        _REFS[key] = (outs, [_state5(r.state) for r in refs], [r.history for r in refs])
    return _REFS[key]


def _filter(pkg, monkeypatch, h, rates, Nphi, P, tx, multi, fused=False, grid=None, pnfb=None):
    """a bound filter on the universal kernel (MRHIP_FORCE_GENERIC is read when the device object is created) or on the multi kernel
    (MRHIP_FARROW_RATES_MULTI=1).  P None: the FIRArbitrary filter with per-channel rates (multi: its tiled kernel)."""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if multi else "1")
    monkeypatch.setenv("MRHIP_FARROW_RATES_MULTI", "1")
    monkeypatch.setenv("MRHIP_ARB_RATES_TILED", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_FARROW_RATES_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_FARROW_RATES_GRID", str(grid))
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    if P is None:
        return pkg.FIRFilter.per_channel_rates(h, rates, Nphi, numerics=numerics).bind(tx, len(rates))
    return pkg.FIRFilter.per_channel_rates_farrow(h, rates, Nphi, P, numerics=numerics, pnfb=pnfb).bind(tx, len(rates))


def _tt(torch, dt):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.complex64): torch.complex64,
            np.dtype(np.complex128): torch.complex128}[np.dtype(dt)]


def _check_end(f, states, hists, what):
    got = f.channel_states
    assert [_state5(s) for s in got] == states, what                                    # the end state, in every bit (== on floats)
    hist = np.atleast_2d(f.history)                                                     # (one channel: a vector)
    for c, hr in enumerate(hists):
        assert_bit_equal(hist[c], hr, f"{what}: history of channel {c}")


def _run_case(pkg, O, monkeypatch, torch, rates, Nphi, hLen, P, x_len, th, tx, multi, fused, chunkings=CHUNKINGS, grid=None):
    seed = 1000 * Nphi + hLen + x_len
    h, x = _signal(seed, Nphi, hLen, x_len, th, tx, rates)
    nch = len(rates)
    xd = torch.from_numpy(np.array(x)).cuda()
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        outs, states, hists = _reference(pkg, O, seed, rates, Nphi, hLen, P, x_len, th, tx, how, fused)
        f = _filter(pkg, monkeypatch, h, rates, Nphi, P, tx, multi, fused, grid)
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
            for c in range(nch):                                                                      # equal rates, equal inputs: bit-equal rows
                first = rates.index(rates[c])
                if first != c:
                    assert want[c] == want[first] and np.array_equal(yh[c, :want[c]].view(np.uint8), yh[first, :want[first]].view(np.uint8)), what
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
        for x_len in X_LENS:
            _run_case(pkg, O, monkeypatch, torch_cuda, rates, Nphi, hLen, P, x_len, th, tx, multi, fused)


@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("P", [4, 1], ids=["p4", "p1"])
@pytest.mark.parametrize("x_len", X_LENS_MULTI)
def test_a_count_that_ends_inside_a_lanes_runs(pkg, O, monkeypatch, torch_cuda, x_len, P, fused):
    """the multi kernel's sizes: lanes with four, three, two and one live outputs, a tile behind a channel's count; the universal kernel
    at the same sizes shares the references"""
    for multi in (True, False):
        _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, P, x_len, np.float32, np.float32, multi, fused, chunkings={"whole": None})
    _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, P, x_len, np.float64, np.complex128, True, fused, chunkings={"whole": None})
    # the sizes are what the docstring says they are
    outs, _, _ = _reference(pkg, O, 1000 * 32 + 250 + x_len, R3, 32, 250, P, x_len, np.float32, np.float32, None, fused)
    tails = sorted(len(outs[c][0]) % 1024 for c in range(3))
    assert tails == ([6, 139, 485] if x_len == 1030 else [52, 363, 988]), tails


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("rates", [R67, R1], ids=["nch67", "nch1"])
def test_a_second_wave_of_the_schedule_kernel_and_one_channel(pkg, O, monkeypatch, torch_cuda, rates, fused, multi):
    for x_len in X_LENS:
        _run_case(pkg, O, monkeypatch, torch_cuda, rates, 32, 250, 4, x_len, np.float32, np.float32, multi, fused)
    _run_case(pkg, O, monkeypatch, torch_cuda, rates, 3, 40, 2, 1500, np.float64, np.complex64, multi, fused, chunkings={"prime": 97})


@pytest.mark.parametrize("grid", [1, 3, 1000])
def test_multi_kernel_on_any_grid(pkg, O, monkeypatch, torch_cuda, grid):
    """one workgroup for every tile, a few, and more workgroups than tiles"""
    _run_case(pkg, O, monkeypatch, torch_cuda, R4, 32, 250, 4, 1500, np.float32, np.float32, True, False, chunkings={"whole": None, "prime": 97}, grid=grid)
    _run_case(pkg, O, monkeypatch, torch_cuda, R3, 32, 250, 4, 2100, np.float32, np.float32, True, False, chunkings={"whole": None}, grid=grid)


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_set_channel_states_and_reset(pkg, O, monkeypatch, torch_cuda, multi):
    torch = torch_cuda
    rates, Nphi, hLen, P, x_len, th, tx = R4, 32, 250, 4, 700, np.float32, np.float32
    seed = 77
    h, x = _signal(seed, Nphi, hLen, x_len, th, tx, rates)
    xd = torch.from_numpy(np.array(x)).cuda()
    start = [(3, 1.0), (1, 17.625), (120, 32.99999), (2, 5.5)]             # per-channel (inputDeficit, phiAccumulator)
    f = _filter(pkg, monkeypatch, h, rates, Nphi, P, tx, multi)
    for bad_d, bad_a in (([0, 1, 1, 1], [1.0] * 4), ([1] * 4, [0.5, 1.0, 1.0, 1.0]), ([1] * 4, [1.0, 1.0, 33.0, 1.0])):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_states(bad_d, bad_a)
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError):
        f.set_channel_states([1, 1], [1.0, 1.0])
    f.set_channel_states([d for d, _ in start], [a for _, a in start])
    got = f.channel_states
    assert [(s.inputDeficit, s.phiAccumulator, s.phiIdx, s.alpha) for s in got] == [(d, a, math.floor(a), a - math.floor(a)) for d, a in start]
    outs, states, hists = _reference(pkg, O, seed, rates, Nphi, hLen, P, x_len, th, tx, 97, False, start=start)
    ys = f.filt(xd[:, :0])                                                  # (an empty call changes nothing)
    assert [len(v) for v in ys] == [0] * 4
    for i, (a, b) in enumerate(_chunks(x_len, 97)):
        ys = f.filt(xd[:, a:b])
        for c in range(4):
            assert_bit_equal(ys[c].cpu().numpy(), outs[c][i], f"after set_channel_states: piece {i}, channel {c}")
    _check_end(f, states, hists, "after set_channel_states")
    # reset(): the constructor state and a history of zeros, for every channel
    f.reset()
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [(1, 1.0, 1, 0.0, 1, 0)] * 4
    assert not f.history.any()
    outs, states, hists = _reference(pkg, O, seed, rates, Nphi, hLen, P, x_len, th, tx, None, False)
    ys = f.filt(xd)
    for c in range(4):
        assert_bit_equal(ys[c].cpu().numpy(), outs[c][0], f"after reset: channel {c}")
    _check_end(f, states, hists, "after reset")
    # numpy in, numpy out: the same list
    f.reset()
    for c, v in enumerate(f.filt(np.array(x))):
        assert isinstance(v, np.ndarray)
        assert_bit_equal(v, outs[c][0], f"numpy signal: channel {c}")
    f.close()


def test_the_bank_the_history_and_the_mod_form(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    h, x = _signal(5, 32, 250, 300, np.float32, np.float32, R3)
    f = _filter(pkg, monkeypatch, h, R3, 32, 4, np.float32, False)
    fit = _fit(pkg, O, h, 32, 4)
    one = pkg.FIRFilter(h, 2.123, 32, 4).bind(np.float32, 1)
    # ONE bank, fitted once by the fit of mrhip_create_farrow: pnfb and tapsforphase answer as on a one-channel FIRFarrow filter of h
    assert f.pnfb().shape == (8, 5)
    assert_bit_equal(f.pnfb(), fit, "pnfb against the per-row fit")
    assert_bit_equal(f.pnfb(), one.pnfb(), "pnfb against the one-channel filter")
    for phase in (0.0, 1.0, 2.5, 17.03125, 33.0):
        assert_bit_equal(f.tapsforphase(phase), one.tapsforphase(phase), f"tapsforphase({phase})")
    with pytest.raises(pkg.MultirateHIPError):
        f.tapsforphase(33.5)
    one.close()
    # a caller-fitted bank (mrhip_create_farrow_rates_pnfb): a bank that no fit of h gives
    own = (fit * 0.75).astype(np.float32).astype(np.float64)
    g = _filter(pkg, monkeypatch, h, R3, 32, 4, np.float32, True, pnfb=own)
    assert_bit_equal(g.pnfb(), own, "the handed-over bank")
    refs = [O.FIRFilter(h, float(r), 32, tx=np.float32, polyorder=4, pnfb=own) for r in R3]
    ys = g.filt(torch.from_numpy(np.array(x)).cuda())
    for c, r in enumerate(refs):
        assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c]), f"a handed-over bank: channel {c}")
    assert g.last_kernel_name() == MULTI
    g.close()
    f.set_mod_form(True)                                                    # N𝜙 a power of two: the two forms agree in every bit
    f.set_mod_form(False)
    f3 = _filter(pkg, monkeypatch, _signal(5, 3, 40, 300, np.float32, np.float32, R3)[0], R3, 3, 2, np.float32, False)
    with pytest.raises(pkg.MultirateHIPError) as e:
        f3.set_mod_form(True)
    assert e.value.code == 5
    f3.set_mod_form(False)
    f3.close()
    # set_history / set_history_device
    hist = np.random.default_rng(3).random((3, 7)).astype(np.float32)
    refs = [_oracle(pkg, O, h, r, 32, 4, np.float32) for r in R3]
    for c, r in enumerate(refs):
        r.set_history(hist[c])
    f.set_history(hist)
    assert_bit_equal(f.history, hist, "set_history")
    ys = f.filt(torch.from_numpy(np.array(x)).cuda())
    for c, r in enumerate(refs):
        assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c]), f"after set_history: channel {c}")
    f.set_history_device(torch.from_numpy(hist).cuda())
    torch.cuda.synchronize()
    assert_bit_equal(f.history, hist, "set_history_device")
    f.set_timing(True)                                                      # one bracket a call, round the walk AND the filter kernel
    f.filt(torch.from_numpy(np.array(x)).cuda())
    n, ms = f.timing_read()
    assert n == 1 and ms > 0.0
    f.close()


def _poisoned(torch, dtype, nch, cap):
    y = torch.empty((nch, cap), dtype=dtype, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    return y


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_refusals_leave_state_and_y_untouched(pkg, O, monkeypatch, torch_cuda, multi):
    torch = torch_cuda
    lib = pkg.load_library()
    rates, Nphi, hLen, P, n = R3, 32, 250, 4, 300
    h, x = _signal(9, Nphi, hLen, 2 * n, np.float32, np.float32, rates)
    xd = torch.from_numpy(np.array(x)).cuda()
    f = _filter(pkg, monkeypatch, h, rates, Nphi, P, np.float32, multi)
    first = f.filt(xd[:, :n])                                               # (a stream in progress)
    before = [_state5(s) + (s.last_count,) for s in f.channel_states]
    hist_before = f.history.copy()
    bound = f.outputlength_bound(n)
    assert bound == math.ceil(n * max(rates)) + 2                           # the largest of the channels' bounds
    y = _poisoned(torch, torch.float32, 3, bound)
    xs = xd[:, n:]
    hnd, stream = f._handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, yp = C.c_void_p(xs.data_ptr()), C.c_void_p(y.data_ptr())
    nw = C.c_int64(-7)

    def refused(rc, code=5, named=None):
        assert rc == code, rc
        msg = lib.mrhip_last_error().decode()
        if code == 5 if named is None else named:                           # the message names both constructors and the calls that serve them
            assert "mrhip_create_arbitrary_rates" in msg and "mrhip_create_farrow_rates" in msg, msg
            assert "mrhip_filt_device_rates" in msg and "mrhip_get_channel_states" in msg and "mrhip_set_channel_states" in msg, msg

    # every entry point that carries ONE state or ONE count
    refused(lib.mrhip_filt_device(hnd, xp, n, 2 * n, yp, bound, bound, C.byref(nw), stream))
    refused(lib.mrhip_filt_device_async(hnd, xp, n, 2 * n, yp, bound, bound, None, stream))
    refused(lib.mrhip_filt_device_chunked(hnd, xp, n, 2 * n, 64, yp, bound, bound, C.byref(nw), stream))
    refused(lib.mrhip_filt_host(hnd, C.c_void_p(x.ctypes.data), n, 2 * n, C.c_void_p(np.empty((3, bound), np.float32).ctypes.data), bound, bound, C.byref(nw)))
    other = pkg.FIRFilter(h, 2.123, Nphi, P).bind(np.float32, 3)
    refused(lib.mrhip_filt_device_chained(hnd, other._handle, xp, n, 2 * n, yp, bound, bound, None, stream))
    refused(lib.mrhip_filt_device_chained(other._handle, hnd, xp, n, 2 * n, yp, bound, bound, None, stream))
    arr = lambda t, v: (t * len(v))(*v)
    refused(lib.mrhip_filt_device_multi(arr(C.c_void_p, [other._handle.value, hnd.value]), 2, arr(C.c_void_p, [xs.data_ptr(), xs.data_ptr()]),
                                        arr(C.c_int64, [n, n]), arr(C.c_void_p, [y.data_ptr(), y.data_ptr()]), arr(C.c_int64, [bound, bound]), None, stream))
    ring = C.c_void_p()
    refused(lib.mrhip_ring_open(hnd, C.byref(ring)))
    assert not ring.value
    casc = C.c_void_p()
    rc = lib.mrhip_cascade_create(arr(C.c_void_p, [hnd.value]), 1, C.byref(casc))
    assert rc == 5 and not casc.value and "mrhip_filt_device_rates" in lib.mrhip_last_error().decode()
    st = pkg.host._State()
    refused(lib.mrhip_get_state(hnd, C.byref(st)))
    refused(lib.mrhip_set_state(hnd, 1, 1, 1.0))
    refused(lib.mrhip_sync_state(hnd, C.byref(nw)))
    for fn in (lib.mrhip_outputlength, lib.mrhip_inputlength, lib.mrhip_next_output_count, lib.mrhip_advance_state):
        assert fn(hnd, n) == -1
        assert "mrhip_create_farrow_rates" in lib.mrhip_last_error().decode()
    for call in (lambda: f.state, lambda: f.set_state(1, 1, 1.0), lambda: f.filt_into_async(y, xs), lambda: f.sync_state(), lambda: f.open_ring(),
                 lambda: f.advance_state(n)):
        with pytest.raises(pkg.MultirateHIPError):
            call()
    assert f.next_output_count(n) == -1 and f.outputlength(n) == -1 and nw.value in (-7, 0)
    # the call's own refusals: a buffer one element short (capacity, then stride), a call past 2^24 entries, a capturing stream, a filter
    # of another constructor
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    cp = C.c_void_p(cnt.data_ptr())
    refused(lib.mrhip_filt_device_rates(hnd, xp, n, 2 * n, yp, bound - 1, bound, cp, stream), 2)
    refused(lib.mrhip_filt_device_rates(hnd, xp, n, 2 * n, yp, bound, bound - 1, cp, stream), 2)
    refused(lib.mrhip_filt_device_rates(hnd, xp, n, n - 1, yp, bound, bound, cp, stream), 1)
    refused(lib.mrhip_filt_device_rates(hnd, xp, -1, 2 * n, yp, bound, bound, cp, stream), 1)
    refused(lib.mrhip_filt_device_rates(other._handle, xp, n, 2 * n, yp, bound, bound, cp, stream), 1)
    states1 = (pkg.ChannelState * 3)()
    refused(lib.mrhip_get_channel_states(other._handle, C.cast(states1, C.c_void_p)), 1)
    refused(lib.mrhip_set_channel_states(other._handle, C.cast(arr(C.c_int64, [1, 1, 1]), C.c_void_p), C.cast(arr(C.c_double, [1.0] * 3), C.c_void_p)), 1)
    refused(lib.mrhip_set_channel_rates(other._handle, C.cast(arr(C.c_double, [1.0] * 3), C.c_void_p)), 1)
    long_n = (1 << 24) // 2                                                 # ceil(n * 2.123) + 2 > 2^24 entries a channel
    refused(lib.mrhip_filt_device_rates(hnd, xp, long_n, long_n, yp, 1 << 26, 1 << 26, cp, stream), 5, named=False)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        scratch.add_(1.0)                                                   # (so that the graph is not empty)
        rc = lib.mrhip_filt_device_rates(hnd, xp, n, 2 * n, yp, bound, bound, cp, C.c_void_p(s.cuda_stream))
    assert rc == 5 and "captur" in lib.mrhip_last_error().decode()
    torch.cuda.synchronize()
    # nothing was enqueued, nothing written, the state is where it was
    assert (y.view(torch.uint8) == POISON).all().item() and not cnt.any().item()
    assert [_state5(s_) + (s_.last_count,) for s_ in f.channel_states] == before
    assert_bit_equal(f.history, hist_before, "history after the refused calls")
    # and the stream goes on as if nothing had happened
    outs, states, hists = _reference(pkg, O, 9, rates, Nphi, hLen, P, 2 * n, np.float32, np.float32, n, False)
    second = f.filt(xs)
    for c in range(3):
        assert_bit_equal(first[c].cpu().numpy(), outs[c][0], f"first call, channel {c}")
        assert_bit_equal(second[c].cpu().numpy(), outs[c][1], f"the call after the refusals, channel {c}")
    _check_end(f, states, hists, "after the refusals")
    assert lib.mrhip_synchronize(hnd, stream) == 0
    other.close()
    f.close()


def test_constructor_refusals_of_the_library(pkg, torch_cuda):
    lib = pkg.load_library()
    h = np.ones(64, dtype=np.float32) + np.arange(64, dtype=np.float32) ** 2
    out = C.c_void_p()

    def mk(th, rates, taps=h, Nphi=32, P=4):
        r = np.asarray(rates, dtype=np.float64)
        return lib.mrhip_create_farrow_rates(C.c_void_p(taps.ctypes.data), len(taps), th, C.c_void_p(r.ctypes.data), Nphi, P, 0, len(r), 0, C.byref(out))

    def mk_pnfb(th, rates, P=4, Nphi=32):
        r = np.asarray(rates, dtype=np.float64)
        pn = np.ones((2, P + 1), dtype=np.float64)
        return lib.mrhip_create_farrow_rates_pnfb(C.c_void_p(pn.ctypes.data), 64, th, C.c_void_p(r.ctypes.data), Nphi, P, 0, len(r), 0, C.byref(out))

    for make in (mk, mk_pnfb):
        for rates in ([0.0, 1.0], [1.0, -1.0], [1.0, float("nan")], [float("inf")]):
            assert make(0, rates) == 1 and not out.value                    # MRHIP_ERR_INVALID_ARG
        assert make(0, [1.0, 2.0 ** -31]) == 5 and not out.value            # a rate below 2^-30
        for th in (2, 3):
            assert make(th, [1.0]) == 5 and not out.value                   # complex taps: left out
    assert lib.mrhip_create_farrow_rates(C.c_void_p(h.ctypes.data), 64, 0, None, 32, 4, 0, 1, 0, C.byref(out)) == 1
    for P, Nphi in ((-1, 32), (33, 64), (4, 4)):                            # polyorder: the checks of mrhip_create_farrow
        assert mk(0, [1.0], Nphi=Nphi, P=P) == 1 and not out.value
    assert mk(0, [1.0], Nphi=0) == 1 and not out.value
    assert mk_pnfb(0, [1.0], P=33) == 1 and not out.value
    assert mk(0, [1.0, 2.0]) == 0 and out.value
    st = (pkg.ChannelState * 2)()
    assert lib.mrhip_get_channel_states(out, C.cast(st, C.c_void_p)) == 0
    assert [(s.rate, s.delta, s.phiAccumulator, s.inputDeficit, s.xIdx) for s in st] == [(1.0, 32.0, 1.0, 1, 1), (2.0, 16.0, 1.0, 1, 1)]
    for bad, code in (([1.0, 0.0], 1), ([float("nan"), 1.0], 1), ([1.0, 2.0 ** -31], 5)):   # mrhip_set_channel_rates: the constructors' checks
        r = np.asarray(bad, dtype=np.float64)
        assert lib.mrhip_set_channel_rates(out, C.c_void_p(r.ctypes.data)) == code
    assert lib.mrhip_set_channel_rates(out, None) == 1
    assert lib.mrhip_get_channel_states(out, C.cast(st, C.c_void_p)) == 0 and [s.rate for s in st] == [1.0, 2.0]      # nothing changed
    lib.mrhip_destroy(out)
    assert mk_pnfb(0, [0.5]) == 0 and out.value
    lib.mrhip_destroy(out)
    # the older constructors answer as before
    assert lib.mrhip_create_farrow(C.c_void_p(h.ctypes.data), 64, 0, 0.0, 32, 4, 0, 1, 0, C.byref(out)) == 1
    assert lib.mrhip_create_farrow(C.c_void_p(h.ctypes.data), 64, 2, 1.5, 32, 4, 0, 1, 0, C.byref(out)) == 5
    assert lib.mrhip_create_farrow(C.c_void_p(h.ctypes.data), 64, 0, 1.5, 32, 4, 0, 1, 0, C.byref(out)) == 0 and out.value
    assert lib.mrhip_set_channel_rates(out, C.c_void_p(np.ones(1).ctypes.data)) == 1          # a filter without per-channel rates
    lib.mrhip_destroy(out)


# ---- rates that change between calls ------------------------------------------------------------------------------------------------
NEW_R4 = [32.0 / 3, 0.01, 0.01, 2.123]       # against R4: channels 0 and 1 swap, channel 2 goes from 2.123 to 0.01, channel 3 stays


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("P", [None, 4], ids=["arbitrary", "farrow"])
def test_set_channel_rates_between_calls(pkg, O, monkeypatch, torch_cuda, P, multi):
    """700 samples in 97-sample pieces, new rates after the third piece.  The reference of channel c: the oracle's filter at the old
    rate for three pieces, then a filter REBUILT at the new rate that is given the old one's (inputDeficit, phiAccumulator) through
    set_state and its history through set_history."""
    torch = torch_cuda
    Nphi, hLen, x_len, th, tx = 32, 250, 700, np.float32, np.float32
    h, x = _signal(123, Nphi, hLen, x_len, th, tx, R4)
    xd = torch.from_numpy(np.array(x)).cuda()
    pieces = _chunks(x_len, 97)
    refs = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in R4]
    never = _oracle(pkg, O, h, R4[3], Nphi, P, tx)                          # channel 3 of a run that never changes a rate
    f = _filter(pkg, monkeypatch, h, R4, Nphi, P, tx, multi)
    plain = _filter(pkg, monkeypatch, h, R4, Nphi, P, tx, multi)            # the library's run that never calls set_channel_rates
    with pytest.raises(pkg.MultirateHIPError):
        f.set_channel_rates([1.0, 2.0])                                     # one rate per channel
    for bad in ([1.0, 0.0, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0]):
        with pytest.raises(pkg.MultirateHIPError):
            f.set_channel_rates(bad)
    assert [s.rate for s in f.channel_states] == R4
    for i, (a, b) in enumerate(pieces):
        if i == 3:
            before = [_state5(s) for s in f.channel_states]
            hist_before = np.array(f.history)
            f.set_channel_rates(NEW_R4)
            got = f.channel_states
            assert [(s.rate, s.delta) for s in got] == [(r, Nphi / r) for r in NEW_R4]
            assert [_state5(s) for s in got] == before                      # accumulator, deficit (and xIdx) stay
            assert_bit_equal(np.array(f.history), hist_before, "the history stays")
            assert f.outputlength_bound(97) == math.ceil(97 * max(NEW_R4)) + 2
            rebuilt = []
            for c, old in enumerate(refs):
                st = old.state
                new = _oracle(pkg, O, h, NEW_R4[c], Nphi, P, tx)
                new.set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
                if old.state.historyLen:
                    new.set_history(old.history)
                rebuilt.append(new)
            refs = rebuilt
        ys, yp = f.filt(xd[:, a:b]), plain.filt(xd[:, a:b])
        want3 = never.filt(x[3, a:b])
        for c, r in enumerate(refs):
            assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c, a:b]), f"piece {i}, channel {c}")
        assert_bit_equal(ys[3].cpu().numpy(), want3, f"piece {i}: the unchanged channel against the run that never changed a rate")
        assert_bit_equal(ys[3].cpu().numpy(), yp[3].cpu().numpy(), f"piece {i}: the unchanged channel against the library's plain run")
    _check_end(f, [_state5(r.state) for r in refs], [r.history for r in refs], "after set_channel_rates")
    # reset() restores the constructor state and KEEPS the current rates
    f.reset()
    assert [(s.rate,) + _state5(s) for s in f.channel_states] == [(r, 1, 1.0, 1, 0.0, 1) for r in NEW_R4]
    fresh = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in NEW_R4]
    ys = f.filt(xd)
    for c, r in enumerate(fresh):
        assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c]), f"after reset at the new rates: channel {c}")
    plain.close()
    f.close()


@pytest.mark.parametrize("P", [None, 4], ids=["arbitrary", "farrow"])
def test_a_raised_rate_outgrows_the_schedule_buffers(pkg, O, monkeypatch, torch_cuda, P):
    """two channels at 0.5 and 300-sample calls: 2 x 152 entries, buffers of 4096; at rate 8 the same call needs 2 x 2402: the
    reallocation path of mrhip_filt_device_rates, in the middle of a stream"""
    torch = torch_cuda
    Nphi, hLen, n, tx = 32, 250, 300, np.float32
    old, new = [0.5, 0.5], [8.0, 0.5]
    h, x = _signal(321, Nphi, hLen, 3 * n, np.float32, tx, [0.5, 0.25])     # (two different rows)
    xd = torch.from_numpy(np.array(x)).cuda()
    f = _filter(pkg, monkeypatch, h, old, Nphi, P, tx, False)
    refs = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in old]
    assert f.outputlength_bound(n) == 152 and 2 * 152 <= 4096
    ys = f.filt(xd[:, :n])
    for c, r in enumerate(refs):
        assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c, :n]), f"before: channel {c}")
    f.set_channel_rates(new)
    assert f.outputlength_bound(n) == 2402 and 2 * 2402 > 4096              # follows the new largest rate; the next call reallocates
    st = refs[0].state
    r0 = _oracle(pkg, O, h, 8.0, Nphi, P, tx)
    r0.set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
    r0.set_history(refs[0].history)
    refs[0] = r0
    for a in (n, 2 * n):
        ys = f.filt(xd[:, a:a + n])
        for c, r in enumerate(refs):
            assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c, a:a + n]), f"after the raise, from sample {a}: channel {c}")
    _check_end(f, [_state5(r.state) for r in refs], [r.history for r in refs], "after the raise")
    shared = pkg.FIRFilter(h, 2.123, Nphi, P).bind(tx, 2)                   # a shared-rate filter: INVALID_ARG
    with pytest.raises(pkg.MultirateHIPError) as e:
        shared.set_channel_rates([1.0, 1.0])
    assert e.value.code == 1
    lib = pkg.load_library()
    assert lib.mrhip_set_channel_rates(shared._handle, C.c_void_p(np.ones(2).ctypes.data)) == 1
    shared.close()
    f.close()


# ---- write only your own outputs: a checker per row -------------------------------------------------------------------------------
def _assert_rows_only_written(backing, nch, cap, oy, pad, counts, want, what):
    """row c's [0, counts[c]) holds the oracle's outputs and every other byte of the backing store is still poison"""
    by, es = backing_bytes(backing)
    assert by.shape == (nch + 2, (oy + cap + pad) * es), (what, by.shape)
    allowed = np.zeros(by.shape, dtype=bool)
    for c in range(nch):
        assert 0 <= counts[c] <= cap, (what, c, counts[c], cap)
        allowed[1 + c, oy * es:(oy + counts[c]) * es] = True
        got = by[1 + c, oy * es:(oy + counts[c]) * es]
        assert np.array_equal(got, np.ascontiguousarray(want[c]).view(np.uint8)), f"{what}: channel {c} differs from the oracle"
    hit = first_stray(by, allowed)
    if hit is not None:
        r, b = hit
        raise AssertionError(f"{what}: wrote outside its outputs: first stray element at row {r - 1}, column {b // es - oy} of the view "
                             f"(counts {list(counts)}, capacity {cap}, guards {oy} in front / {pad} behind)")


@pytest.mark.parametrize("layout", ["tight", "A", "B", "C"])
@pytest.mark.parametrize("types", [(np.float32, np.float32), (np.float64, np.complex64)], ids=["f32", "c128"])
@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, O, monkeypatch, torch_cuda, multi, types, layout):
    torch = torch_cuda
    th, tx = types
    rates, Nphi, hLen, P = R4, 32, 250, 4
    sizes = [257, 5, 40, 300, 500]             # (500 at 2.123: 1062 outputs, a lane of the multi kernel with one live slot of four)
    x_len = sum(sizes)
    h, x = _signal(31, Nphi, hLen, x_len, th, tx, rates)
    pieces = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
    O.set_fused(False)
    refs = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in rates]
    f = _filter(pkg, monkeypatch, h, rates, Nphi, P, tx, multi)
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
