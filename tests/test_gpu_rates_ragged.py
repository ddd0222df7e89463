"""GPU tests of per-channel input lengths for the filters with per-channel rates: FIRFilter.per_channel_rates(...) and
FIRFilter.per_channel_rates_farrow(...) called as filt_into(buffer, x, lengths) / filt(x, lengths) (mrhip_filt_device_rates_ragged).

Bar (include/multirate_hip.h at mrhip_filt_device_rates_ragged): for every channel c the outputs and the count of every call, the end
state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx) and the history are BIT FOR BIT those of the oracle's one-channel filter
O.FIRFilter(h, rates[c], Nphi[, polyorder], tx=tx) fed x[c, :lengths[c]] call after call -- for both families, on both kernels of each
(MRHIP_FORCE_GENERIC; MRHIP_ARB_RATES_TILED=1, MRHIP_FARROW_RATES_MULTI=1; the *_GRID switches for other grids), under STRICT and
FUSED.  No tolerance anywhere.  A channel of length 0 keeps its state and its history.
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, POISON, make_buffer, row_pad
from test_gpu_rates_arb import _assert_rows_only_written

pytestmark = pytest.mark.gpu

NAME = "mrhip_filt_device_rates_ragged"
R4 = [0.01, 32.0 / 3, 2.123, 2.123]      # a channel that writes nothing in most calls; an exactly cycling rate; two equal rates
NEW_R4 = [0.02, 32.0 / 3, 1.37, 2.123]
CALLS = [[257, 0, 5, 257], [3, 300, 0, 7], [1500, 1, 257, 2], [0, 0, 0, 0], [100, 100, 100, 100]]
COUNTS = [[3, 0, 11, 546], [0, 3200, 0, 15], [15, 11, 546, 4], [0, 0, 0, 0], [1, 1067, 212, 213]]      # at N𝜙 32: the oracle's, checked on the CPU
R67 = [0.3 + 0.05 * c for c in range(67)]
L67 = [(37 * c) % 301 for c in range(67)]
CALLS67 = [L67[5 * i:] + L67[:5 * i] for i in range(3)]                      # the lengths rotate by 5 channels a call
ALL_TYPES = [(th, tx) for th in (np.float32, np.float64) for tx in (np.float32, np.float64, np.complex64, np.complex128)]
FEW_TYPES = [(np.float32, np.float32), (np.float64, np.complex64)]
# (Nphi, hLen): T = 8, H = 7 with all eight type pairs; T = 1 (no history); the division path (T = 14); T = 32
CASES = [((32, 250), t) for t in ALL_TYPES] + [(b, t) for b in ((4, 4), (3, 40), (32, 1024)) for t in FEW_TYPES]
FAMILIES = ["arbitrary", "farrow"]
KERNELS = {("arbitrary", False): "arb_rates_generic", ("arbitrary", True): "arb_rates_tiled",
           ("farrow", False): "farrow_rates_generic", ("farrow", True): "farrow_rates_multi"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _poly(family, Nphi):
    """the polyorder of a family's filters: None for FIRArbitrary; FIRFarrow: 4, the unrolled chain (banks of 3 and 4 phases: 2, the loop)"""
    return None if family == "arbitrary" else (4 if Nphi > 4 else 2)


_SIGNALS = {}


def _signal(seed, Nphi, hLen, calls, th, tx, rates):
    """one tap vector (about unit gain per phase) and, per call, the (nch, max length) matrix of samples; channels of EQUAL rate get
    equal rows"""
    key = (seed, Nphi, hLen, str(calls), np.dtype(th).name, np.dtype(tx).name, tuple(rates))
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        h = (rng.standard_normal(hLen) * Nphi / max(hLen, 1)).astype(th)
        nch = len(rates)
        xs = []
        for lens in calls:
            n = max(lens)
            x = rng.random((nch, n)) - 0.5
            if np.dtype(tx).kind == "c":
                x = x + 1j * (rng.random((nch, n)) - 0.5)
            for c in range(nch):
                first = rates.index(rates[c])
                if first != c:
                    x[c] = x[first]
            x = x.astype(tx)
            x.setflags(write=False)
            xs.append(x)
        h.setflags(write=False)
        _SIGNALS[key] = (h, xs)
    return _SIGNALS[key]


_FITS = {}


def _oracle(pkg, O, h, rate, Nphi, P, tx):
    """the reference of one channel: the oracle's FIRFilter(h, rate, Nphi) -- P None -- or FIRFilter(h, rate, Nphi, polyorder = P) on the
    library's per-row fit of h (as tests/test_gpu_rates_farrow.py)"""
    if P is None:
        return O.FIRFilter(h, float(rate), Nphi, tx=tx)
    key = (h.tobytes(), h.dtype.name, Nphi, P)
    if key not in _FITS:
        pfb = O.taps2pfb(h, Nphi)
        _FITS[key] = np.stack([pkg.polyfit(pfb[i].astype(np.float64), P).astype(h.dtype).astype(np.float64) for i in range(pfb.shape[0])])
    return O.FIRFilter(h, float(rate), Nphi, tx=tx, polyorder=P, pnfb=_FITS[key])


def _state5(st):
    return (st.inputDeficit, st.phiAccumulator, st.phiIdx, st.alpha, st.xIdx)


def _feed(refs, x, lens):
    """one ragged call of the references: channel c is fed x[c, :lens[c]]"""
    return [r.filt(x[c, :lens[c]]) for c, r in enumerate(refs)]


_REFS = {}


def _reference(pkg, O, seed, rates, Nphi, hLen, P, calls, th, tx, fused):
    """(outputs [call][c], states [call][c], histories [call][c]) of the one-channel references over the sequence of calls; computed once
    per case and shared by the kernels"""
    key = (seed, tuple(rates), Nphi, hLen, P, str(calls), np.dtype(th).name, np.dtype(tx).name, fused)
    if key not in _REFS:
        h, xs = _signal(seed, Nphi, hLen, calls, th, tx, rates)
        O.set_fused(fused)
        try:
            refs = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in rates]
            outs, states, hists = [], [], []
            for x, lens in zip(xs, calls):
                outs.append(_feed(refs, x, lens))
                states.append([_state5(r.state) for r in refs])
                hists.append([np.array(r.history) for r in refs])
        finally:
            O.set_fused(False)
        _REFS[key] = (outs, states, hists)
    return _REFS[key]


def _filter(pkg, monkeypatch, family, h, rates, Nphi, tx, fast, fused=False, grid=None):
    """a bound filter on its family's universal kernel (MRHIP_FORCE_GENERIC is read when the device object is created) or on the tiled /
    multi kernel; grid: the *_GRID switch of that kernel"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if fast else "1")
    monkeypatch.setenv("MRHIP_FARROW_RATES_MULTI", "1")
    monkeypatch.setenv("MRHIP_ARB_RATES_TILED", "1")
    for name in ("MRHIP_ARB_RATES_GRID", "MRHIP_FARROW_RATES_GRID"):
        if grid is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(grid))
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    if family == "arbitrary":
        return pkg.FIRFilter.per_channel_rates(h, rates, Nphi, numerics=numerics).bind(tx, len(rates))
    return pkg.FIRFilter.per_channel_rates_farrow(h, rates, Nphi, _poly(family, Nphi), numerics=numerics).bind(tx, len(rates))


def _tt(torch, dt):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.complex64): torch.complex64,
            np.dtype(np.complex128): torch.complex128}[np.dtype(dt)]


def _check_state(f, states, hists, what):
    assert [_state5(s) for s in f.channel_states] == states, what                       # the end state, in every bit (== on floats)
    hist = np.atleast_2d(f.history)
    for c, hr in enumerate(hists):
        assert_bit_equal(hist[c], hr, f"{what}: history of channel {c}")


def _ragged_call(torch, f, x, lens, out_dtype):
    """one ragged call into a zeroed buffer of the call's bound: (counts, the buffer on the host)"""
    nch = len(lens)
    bound = f.outputlength_bound(max(lens))
    assert bound == (math.ceil(max(lens) * f.rate) + 2 if max(lens) else 0)
    y = torch.zeros((nch, bound), dtype=_tt(torch, out_dtype), device="cuda")
    xd = torch.from_numpy(np.array(x)).cuda()
    counts = f.filt_into(y, xd, lengths=lens)
    assert counts.dtype == np.int64 and counts.shape == (nch,)
    return counts, y.cpu().numpy()


def _run_sequence(pkg, O, monkeypatch, torch, family, rates, Nphi, hLen, calls, th, tx, fast, fused, grid=None, seed=None):
    P = _poly(family, Nphi)
    seed = 5000 + 10 * Nphi + hLen if seed is None else seed
    h, xs = _signal(seed, Nphi, hLen, calls, th, tx, rates)
    outs, states, hists = _reference(pkg, O, seed, rates, Nphi, hLen, P, calls, th, tx, fused)
    f = _filter(pkg, monkeypatch, family, h, rates, Nphi, tx, fast, fused, grid)
    nch = len(rates)
    for i, (x, lens) in enumerate(zip(xs, calls)):
        what = f"{family} Nphi {Nphi} hLen {hLen} {np.dtype(th).name}/{np.dtype(tx).name} call {i} lengths {lens[:6]}"
        want = [len(o) for o in outs[i]]
        counts, yh = _ragged_call(torch, f, x, lens, outs[0][0].dtype)
        assert list(counts) == want, (what, list(counts), want)                             # counts_out
        assert [s.last_count for s in f.channel_states] == want, what                       # last_count
        for c in range(nch):
            assert_bit_equal(yh[c, :want[c]], outs[i][c], f"{what}: channel {c}")
            assert not yh[c, want[c]:].any(), f"{what}: channel {c} wrote behind its count"
        if max(lens) > 0:
            assert f.last_kernel_name() == KERNELS[(family, fast)], what
        _check_state(f, states[i], hists[i], what)                                          # after EVERY call: state and history
    f.close()
    return outs, states


def _assert_the_sequence_holds_its_cases(outs, states, Nphi, T):
    """properties of the REFERENCE over CALLS that the test exists for, so that a later change of inputs cannot empty it"""
    counts = [[len(o) for o in call] for call in outs]
    if Nphi == 32:
        assert counts == COUNTS
    assert any(min(c) == 0 < max(c) for c in counts)                                        # zero counts beside non-zero ones
    # a channel on the short-input path (its deficit only shrinks: no output, xIdx and the accumulator stay) while neighbours produce outputs
    short = [(i, c) for i in range(1, len(CALLS)) for c in range(4)
             if CALLS[i][c] > 0 and counts[i][c] == 0 and states[i][c][0] == states[i - 1][c][0] - CALLS[i][c] and states[i][c][1:] == states[i - 1][c][1:]]
    assert any(max(counts[i]) > 0 for i, _ in short), short
    if Nphi == 32:
        assert (states[0][0][0], states[1][0][0]) == (44, 41)                               # channel 0: 44 -> 41 in the second call
    assert any(l == 0 for call in CALLS for l in call) and [0, 0, 0, 0] in CALLS            # zero-length channels; an all-empty call
    for i in range(1, len(CALLS)):                                                          # ... which keep their state
        for c in range(4):
            if CALLS[i][c] == 0:
                assert states[i][c] == states[i - 1][c] and counts[i][c] == 0
    H = T - 1
    if H > 1:                                                                               # lengths below H beside lengths above it
        assert any(0 < min([l for l in call if l], default=0) < H <= max(call) for call in CALLS)
    assert any(257 in call for call in CALLS)                                               # a tile boundary


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("bank,types", CASES, ids=[f"{b[0]}x{b[1]}-{np.dtype(t[0]).name}-{np.dtype(t[1]).name}" for b, t in CASES])
@pytest.mark.parametrize("family", FAMILIES)
def test_a_sequence_of_ragged_calls(pkg, O, monkeypatch, torch_cuda, family, bank, types, fused, fast):
    (Nphi, hLen), (th, tx) = bank, types
    outs, states = _run_sequence(pkg, O, monkeypatch, torch_cuda, family, R4, Nphi, hLen, CALLS, th, tx, fast, fused)
    _assert_the_sequence_holds_its_cases(outs, states, Nphi, -(-hLen // Nphi))


@pytest.mark.parametrize("grid", [1, 3, 1000])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_tiled_and_multi_kernels_on_any_grid(pkg, O, monkeypatch, torch_cuda, family, grid):
    """one workgroup for every tile, a few, and more workgroups than tiles: the grid's LAST workgroup folds the histories"""
    _run_sequence(pkg, O, monkeypatch, torch_cuda, family, R4, 32, 250, CALLS, np.float32, np.float32, True, False, grid=grid)


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("family", FAMILIES)
def test_67_channels_of_every_length_class(pkg, O, monkeypatch, torch_cuda, family, fused, fast):
    """a second wave of the schedule kernel with idle lanes; lengths 0, below H, H and above in one history fold"""
    assert {0} < set(L67) and any(0 < l < 7 for l in L67) and any(l > 256 for l in L67) and len(set(map(tuple, CALLS67))) == 3
    _run_sequence(pkg, O, monkeypatch, torch_cuda, family, R67, 32, 250, CALLS67, np.float32, np.float32, fast, fused)


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_equal_lengths_are_the_existing_call(pkg, monkeypatch, torch_cuda, family, fast):
    """lengths = [n] * nch against filt_into(buffer, x) on a twin filter, as one stream over n = 1, 5, 257, 1500: the same bytes in the
    buffer, the same counts, states and histories"""
    torch = torch_cuda
    h, xs = _signal(41, 32, 250, [[n] * 4 for n in (1, 5, 257, 1500)], np.float32, np.float32, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    twin = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    f.set_timing(True)                                                       # one bracket a ragged call, round the walk AND the filter kernel
    for x in xs:
        n = x.shape[1]
        xd = torch.from_numpy(np.array(x)).cuda()
        ya, yb = (torch.zeros((4, f.outputlength_bound(n)), dtype=torch.float32, device="cuda") for _ in range(2))
        ca, cb = f.filt_into(ya, xd, lengths=np.full(4, n, dtype=np.int64)), twin.filt_into(yb, xd)
        assert list(ca) == list(cb) and max(ca) > 0, n
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), n
        assert f.last_kernel_name() == twin.last_kernel_name() == KERNELS[(family, fast)]
        assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [_state5(s) + (s.last_count,) for s in twin.channel_states], n
        assert_bit_equal(f.history, twin.history, f"history after n = {n}")
    launches, ms = f.timing_read()
    assert launches == 4 and ms > 0.0
    f.close(), twin.close()


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_calls_around_state_and_rate_changes(pkg, O, monkeypatch, torch_cuda, family, fast):
    """ragged calls, set_channel_rates, ragged calls (the reference of channel c is REBUILT at the new rate and given the old one's
    state and history, as tests/test_gpu_rates_farrow.py does); then reset() (the reference restarts at the current rates) and ragged
    calls; then set_channel_states (the reference is seeded likewise) and a ragged call"""
    torch = torch_cuda
    Nphi, hLen, tx = 32, 250, np.float32
    P = _poly(family, Nphi)
    h, xs = _signal(77, Nphi, hLen, CALLS, np.float32, tx, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, Nphi, tx, fast)
    refs = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in R4]

    def both(i, what):
        want = _feed(refs, xs[i], CALLS[i])
        counts, yh = _ragged_call(torch, f, xs[i], CALLS[i], want[0].dtype)
        assert list(counts) == [len(w) for w in want], what
        for c in range(4):
            assert_bit_equal(yh[c, :len(want[c])], want[c], f"{what}: call {i}, channel {c}")
        _check_state(f, [_state5(r.state) for r in refs], [np.array(r.history) for r in refs], f"{what}: call {i}")

    both(0, "before the rate change"), both(1, "before the rate change")
    f.set_channel_rates(NEW_R4)
    rebuilt = []
    for c, old in enumerate(refs):
        st = old.state
        new = _oracle(pkg, O, h, NEW_R4[c], Nphi, P, tx)
        new.set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
        new.set_history(old.history)
        rebuilt.append(new)
    refs = rebuilt
    for i in (2, 3, 4):
        both(i, "after set_channel_rates")
    f.reset()                                                                # the constructor state, a history of zeros, the CURRENT rates
    refs = [_oracle(pkg, O, h, r, Nphi, P, tx) for r in NEW_R4]
    assert [(s.rate,) + _state5(s) for s in f.channel_states] == [(r, 1, 1.0, 1, 0.0, 1) for r in NEW_R4] and not f.history.any()
    both(1, "after reset"), both(0, "after reset")
    start = [(3, 1.0), (1, 17.625), (120, 32.99999), (2, 5.5)]                # per-channel (inputDeficit, phiAccumulator)
    f.set_channel_states([d for d, _ in start], [a for _, a in start])
    for r, (d, a) in zip(refs, start):
        r.set_state(int(math.floor(a)), int(d), float(a))
    both(2, "after set_channel_states"), both(4, "after set_channel_states")
    f.close()


@pytest.mark.parametrize("layout", ["tight", "A", "B", "C"])
@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, O, monkeypatch, torch_cuda, family, fast, layout):
    """poisoned backing stores, tight and odd-stride y layouts, on the first two calls of the sequence: no byte outside [0, count_c) of
    any row changes.  The same for x: the samples of row c at and behind lengths[c] are NaN, and the outputs are the oracle's."""
    torch = torch_cuda
    Nphi, hLen, tx = 32, 250, np.float32
    h, xs = _signal(31, Nphi, hLen, CALLS, np.float32, tx, R4)
    outs, states, hists = _reference(pkg, O, 31, R4, Nphi, hLen, _poly(family, Nphi), CALLS, np.float32, tx, False)
    f = _filter(pkg, monkeypatch, family, h, R4, Nphi, tx, fast)
    oy, _, ox = LAYOUTS[layout]
    for i in (0, 1):
        lens, n = CALLS[i], max(CALLS[i])
        xback = torch.full((4, ox + n + 3), float("nan"), dtype=torch.float32, device="cuda")
        for c in range(4):
            xback[c, ox:ox + lens[c]] = torch.from_numpy(np.array(xs[i][c, :lens[c]])).cuda()
        cap = f.outputlength_bound(n)
        pad = row_pad(layout, oy, cap, 4)
        view, backing = make_buffer(torch, np.float32, 4, cap, oy, pad)
        counts = f.filt_into(view, xback[:, ox:ox + n], lengths=lens)
        assert list(counts) == [len(o) for o in outs[i]] and min(counts) == 0 < max(counts)
        assert f.last_kernel_name() == KERNELS[(family, fast)]
        _assert_rows_only_written(backing, 4, cap, oy, pad, counts, outs[i], f"{family} {layout} call {i}")
        _check_state(f, states[i], hists[i], f"{family} {layout} call {i}")              # (no NaN reached a history either)
    f.close()


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_back_to_back_calls_without_a_wait(pkg, monkeypatch, torch_cuda, family, fast):
    """eight ragged calls enqueued with no wait between them -- more than the staging slots -- on a stream that is busy when the first
    one arrives; the caller overwrites its lengths array as soon as a call returns.  The results are those of the same calls made one
    at a time (each waited for) on a twin filter."""
    torch = torch_cuda
    calls = [CALLS[i % 5] if i != 3 else [9, 0, 1500, 40] for i in range(8)]
    h, xs = _signal(53, 32, 250, calls, np.float32, np.float32, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    twin = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    xds = [torch.from_numpy(np.array(x)).cuda() for x in xs]
    cap = f.outputlength_bound(1500)
    ys = torch.zeros((8, 4, cap), dtype=torch.float32, device="cuda")
    cnts = torch.full((8, 4), -1, dtype=torch.int64, device="cuda")
    lens = np.zeros(4, dtype=np.int64)                                       # ONE array, rewritten for every call
    busy = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    for _ in range(4):
        busy = busy @ busy * 1e-3                                            # (work in front of the first call on the stream)
    for i in range(8):
        lens[:] = calls[i]
        f._filt_into_rates(ys[i], xds[i], counts=cnts[i], lengths=lens)      # returns without waiting
        lens[:] = -12345                                                     # the caller's array is free again
    torch.cuda.synchronize()
    for i in range(8):
        y1 = torch.zeros((4, cap), dtype=torch.float32, device="cuda")
        c1 = twin.filt_into(y1, xds[i], lengths=list(calls[i]))              # (waits for its counts)
        assert cnts[i].cpu().tolist() == list(c1), i
        assert torch.equal(ys[i].view(torch.int32), y1.view(torch.int32)), i
    assert [_state5(s) + (s.last_count,) for s in f.channel_states] == [_state5(s) + (s.last_count,) for s in twin.channel_states]
    assert_bit_equal(f.history, twin.history, "history after the eight calls")
    f.close(), twin.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_refusals_name_the_call_and_leave_everything_untouched(pkg, monkeypatch, torch_cuda, family):
    torch = torch_cuda
    lib = pkg.load_library()
    n = 300
    h, xs = _signal(9, 32, 250, [[n] * 4, [n] * 4], np.float32, np.float32, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, False)
    twin = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, False)
    xd = [torch.from_numpy(np.array(x)).cuda() for x in xs]
    first = f.filt(xd[0], lengths=[n, 0, 5, n])                              # (a stream in progress)
    before = [_state5(s) + (s.last_count,) for s in f.channel_states]
    hist_before = np.array(f.history)
    bound = f.outputlength_bound(n)
    y = torch.empty((4, bound), dtype=torch.float32, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    hnd, stream = f._handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, yp, cp = C.c_void_p(xd[1].data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(cnt.data_ptr())
    arr = lambda v: (C.c_int64 * len(v))(*v)
    good = arr([n, 0, 5, n])

    def refused(rc, code):
        msg = lib.mrhip_last_error().decode()
        assert rc == code and NAME in msg, (rc, code, msg)

    call = lib.mrhip_filt_device_rates_ragged
    refused(call(None, xp, good, n, yp, bound, bound, cp, stream), 1)                       # NULL f
    refused(call(hnd, xp, None, n, yp, bound, bound, cp, stream), 1)                        # NULL x_lens
    other = pkg.FIRFilter(h, 2.123, 32).bind(np.float32, 4)
    refused(call(other._handle, xp, good, n, yp, bound, bound, cp, stream), 1)              # a filter without per-channel rates
    refused(call(hnd, xp, arr([n, -1, 5, n]), n, yp, bound, bound, cp, stream), 1)          # a negative length
    refused(call(hnd, xp, arr([n, 0, 2 ** 31 - 1, n]), 2 ** 31, yp, bound, bound, cp, stream), 5)      # a length >= 2^31 - 1
    refused(call(hnd, None, good, n, yp, bound, bound, cp, stream), 1)                      # x NULL with a non-zero length
    refused(call(hnd, xp, good, n - 1, yp, bound, bound, cp, stream), 1)                    # x_stride < the largest length
    long_n = (1 << 24) // 10                                                                # ceil(n * 32/3) + 2 > 2^24 entries a channel
    refused(call(hnd, xp, arr([1, long_n, 1, 1]), long_n, yp, 1 << 28, 1 << 28, cp, stream), 5)        # a bound above 2^24
    refused(call(hnd, xp, good, n, yp, bound - 1, bound, cp, stream), 2)                    # capacity, then stride, one element short
    refused(call(hnd, xp, good, n, yp, bound, bound - 1, cp, stream), 2)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        scratch.add_(1.0)                                                    # (so that the graph is not empty)
        rc = call(hnd, xp, good, n, yp, bound, bound, cp, C.c_void_p(s.cuda_stream))
    msg = lib.mrhip_last_error().decode()
    assert rc == 5 and "captur" in msg and NAME in msg                       # a capturing stream
    torch.cuda.synchronize()
    with pytest.raises(pkg.MultirateHIPError) as e:
        other.filt(xd[1], lengths=[n] * 4)                                   # the keyword on any other filter
    assert e.value.code == 1
    for bad in ([n, 0, 5], [n, 0, 5, n + 1]):                                # one length per channel; none beyond a row of x
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.filt(xd[1], lengths=bad)
        assert e.value.code == 1
    # nothing was enqueued, nothing written, the state is where it was
    assert (y.view(torch.uint8) == POISON).all().item() and not cnt.any().item()
    assert [_state5(s_) + (s_.last_count,) for s_ in f.channel_states] == before
    assert_bit_equal(np.array(f.history), hist_before, "history after the refused calls")
    # the old entry point's refusals read as before
    old = lib.mrhip_filt_device_rates
    for rc, code, text in ((old(hnd, xp, -1, n, yp, bound, bound, cp, stream), 1, "negative length"),
                           (old(hnd, xp, n, n - 1, yp, bound, bound, cp, stream), 1, "x_stride < x_len"),
                           (old(hnd, None, n, n, yp, bound, bound, cp, stream), 1, "x is NULL"),
                           (old(hnd, xp, n, n, yp, bound - 1, bound, cp, stream), 2,
                            "buffer is too small: mrhip_filt_device_rates needs room for mrhip_outputlength_bound(x_len) outputs per channel"),
                           (old(hnd, xp, n, n, yp, bound, bound - 1, cp, stream), 2, "buffer is too small: y_stride < mrhip_outputlength_bound(x_len)"),
                           (old(other._handle, xp, n, n, yp, bound, bound, cp, stream), 1,
                            "mrhip_filt_device_rates takes a filter of mrhip_create_arbitrary_rates or mrhip_create_farrow_rates")):
        assert rc == code, text
    assert lib.mrhip_last_error().decode() == "mrhip_filt_device_rates takes a filter of mrhip_create_arbitrary_rates or mrhip_create_farrow_rates"
    assert old(hnd, xp, n, n, yp, bound, bound - 1, cp, stream) == 2
    assert lib.mrhip_last_error().decode() == "buffer is too small: y_stride < mrhip_outputlength_bound(x_len)"
    # and the stream goes on as if nothing had happened: the twin made the two calls and nothing else
    want0, want1 = twin.filt(xd[0], lengths=[n, 0, 5, n]), twin.filt(xd[1], lengths=[5, n, n, 0])
    second = f.filt(xd[1], lengths=[5, n, n, 0])
    for c in range(4):
        assert torch.equal(first[c], want0[c]) and torch.equal(second[c], want1[c]), c
    assert [_state5(s_) for s_ in f.channel_states] == [_state5(s_) for s_ in twin.channel_states]
    other.close(), twin.close(), f.close()
