"""GPU tests of input lengths from device memory, and chaining, for the filters with per-channel rates: FIRFilter.filt_rates_async
(mrhip_filt_device_rates_lens_device, mrhip_filt_device_rates_chained; include/multirate_hip.h, "Input lengths from device memory, and
chaining, for the filters with per-channel rates").

Bar: for every channel c the outputs and the count of every call, the end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx) and
the history are BIT FOR BIT those of the oracle's one-channel filter fed x[c, :lengths[c]] call after call -- the lengths being what a
CUDA tensor holds when the stream reaches the call, or the counts of the filter in front -- for both families, on both kernels of
each, under STRICT and FUSED, over shared, per-channel and complex per-channel taps.  A length outside [0, max_length] feeds its channel
nothing.  No tolerance anywhere.  Fixtures, signals and references are those of tests/test_gpu_rates_ragged.py.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, POISON, make_buffer, row_pad
from test_gpu_rates_arb import _assert_rows_only_written
from test_gpu_rates_ragged import (CALLS, CALLS67, COUNTS, FAMILIES, FEW_TYPES, KERNELS, R4, R67, _check_state, _filter, _oracle, _poly, _reference,
                                   _signal, _state5, _tt, torch_cuda)  # noqa: F401  (torch_cuda: the module's fixture)

pytestmark = pytest.mark.gpu

LENS, CHAINED = "mrhip_filt_device_rates_lens_device", "mrhip_filt_device_rates_chained"
I64_MIN = -2 ** 63


def _dev_call(torch, f, x, lens, out_dtype, max_length=None):
    """one call with the lengths in a CUDA tensor, into a zeroed buffer of the call's bound: (counts, the buffer on the host)"""
    nch = len(lens)
    m = max(max(lens), 0) if max_length is None else max_length
    y = torch.zeros((nch, f.outputlength_bound(m)), dtype=_tt(torch, out_dtype), device="cuda")
    xd = torch.from_numpy(np.array(x)).cuda()
    ld = torch.tensor(list(lens), dtype=torch.int64, device="cuda")
    counts = f.filt_rates_async(y, xd, lengths=ld, max_length=m)             # (returns without waiting)
    assert counts.is_cuda and counts.dtype == torch.int64 and tuple(counts.shape) == (nch,)
    return counts.cpu().numpy(), y.cpu().numpy()


def _assert_call(f, counts, yh, outs, states, hists, what):
    want = [len(o) for o in outs]
    assert list(counts) == want, (what, list(counts), want)
    assert [s.last_count for s in f.channel_states] == want, what
    for c, o in enumerate(outs):
        assert_bit_equal(yh[c, :want[c]], o, f"{what}: channel {c}")
        assert not yh[c, want[c]:].any(), f"{what}: channel {c} wrote behind its count"
    _check_state(f, states, hists, what)


def _run_sequence(pkg, O, monkeypatch, torch, family, rates, Nphi, hLen, calls, th, tx, fast, fused):
    P = _poly(family, Nphi)
    seed = 5000 + 10 * Nphi + hLen                                           # (the ragged module's: one reference for both)
    h, xs = _signal(seed, Nphi, hLen, calls, th, tx, rates)
    outs, states, hists = _reference(pkg, O, seed, rates, Nphi, hLen, P, calls, th, tx, fused)
    f = _filter(pkg, monkeypatch, family, h, rates, Nphi, tx, fast, fused)
    for i, (x, lens) in enumerate(zip(xs, calls)):
        what = f"{family} Nphi {Nphi} hLen {hLen} {np.dtype(th).name}/{np.dtype(tx).name} call {i} lengths {lens[:6]}"
        counts, yh = _dev_call(torch, f, x, lens, outs[0][0].dtype)
        _assert_call(f, counts, yh, outs[i], states[i], hists[i], what)
        if max(lens) > 0:
            assert f.last_kernel_name() == KERNELS[(family, fast)], what
    f.close()
    return outs


SEQ_CASES = [(b, t) for b in ((32, 250), (4, 4)) for t in FEW_TYPES]


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("bank,types", SEQ_CASES, ids=[f"{b[0]}x{b[1]}-{np.dtype(t[0]).name}-{np.dtype(t[1]).name}" for b, t in SEQ_CASES])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_sequence_of_calls_with_the_lengths_in_a_cuda_tensor(pkg, O, monkeypatch, torch_cuda, family, bank, types, fused, fast):
    (Nphi, hLen), (th, tx) = bank, types
    outs = _run_sequence(pkg, O, monkeypatch, torch_cuda, family, R4, Nphi, hLen, CALLS, th, tx, fast, fused)
    if Nphi == 32:
        assert [[len(o) for o in call] for call in outs] == COUNTS


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("taps", ["per-channel", "complex-per-channel"])
def test_the_sequence_over_per_channel_and_complex_per_channel_taps(pkg, O, monkeypatch, torch_cuda, taps, fast):
    """FIRArbitrary over a bank per channel: O.FIRFilter(H[c], rates[c], Nphi) fed x[c, :lengths[c]]; over complex banks and real samples
    the oracle by components (a complex tap times a real sample is two real products), as tests/test_gpu_rates_arb_ctaps.py"""
    torch = torch_cuda
    Nphi, hLen, tx = 32, 250, np.float32
    _, xs = _signal(61, Nphi, hLen, CALLS, np.float32, tx, R4)
    rng = np.random.default_rng(62)
    H = (rng.standard_normal((4, hLen)) * Nphi / hLen).astype(np.float32)
    for name in ("MRHIP_ARB_RATES_TILED", "MRHIP_ARB_RATES_BANK_TILED", "MRHIP_ARB_RATES_CTAPS_TILED"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if fast else "1")
    if taps == "per-channel":
        f = pkg.FIRFilter.per_channel_taps_and_rates(H, R4, Nphi).bind(tx, 4)
        parts = [[O.FIRFilter(H[c], float(r), Nphi, tx=tx)] for c, r in enumerate(R4)]
    else:
        Hc = (H + 1j * (rng.standard_normal((4, hLen)) * Nphi / hLen)).astype(np.complex64)
        f = pkg.FIRFilter.per_channel_complex_taps_and_rates(Hc, R4, Nphi).bind(tx, 4)
        parts = [[O.FIRFilter(np.ascontiguousarray(Hc[c].real), float(r), Nphi, tx=tx), O.FIRFilter(np.ascontiguousarray(Hc[c].imag), float(r), Nphi, tx=tx)]
                 for c, r in enumerate(R4)]
    for i, (x, lens) in enumerate(zip(xs, CALLS)):
        outs = []
        for c, p in enumerate(parts):
            ys = [r.filt(x[c, :lens[c]]) for r in p]
            if len(ys) == 2:
                y = np.empty(len(ys[0]), dtype=np.complex64)
                y.real, y.imag = ys
                ys = [y]
            outs.append(ys[0])
        counts, yh = _dev_call(torch, f, x, lens, outs[0].dtype)
        _assert_call(f, counts, yh, outs, [_state5(p[0].state) for p in parts], [np.array(p[0].history) for p in parts], f"{taps} call {i}")
        assert list(counts) == COUNTS[i]
        if max(lens) > 0:
            assert f.last_kernel_name() == ("arb_rates_bank_" if taps == "per-channel" else "arb_rates_ctaps_") + ("tiled" if fast else "generic")
    f.close()


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("family", FAMILIES)
def test_67_channels(pkg, O, monkeypatch, torch_cuda, family, fused, fast):
    """a second workgroup of the import kernel with idle lanes; lengths 0, below H, H and above in one call"""
    _run_sequence(pkg, O, monkeypatch, torch_cuda, family, R67, 32, 250, CALLS67, np.float32, np.float32, fast, fused)


def _everything(f):
    return [_state5(s) + (s.last_count,) for s in f.channel_states]


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_equal_to_the_host_ragged_call_and_mixing_with_the_older_calls(pkg, monkeypatch, torch_cuda, family, fast):
    """the same lengths through mrhip_filt_device_rates_ragged on a twin filter: identical bytes in the buffer, counts, states and
    histories; the filter under test alternates the device-length call, the host ragged call and the plain call, the twin makes the
    host's form of each"""
    torch = torch_cuda
    forms = [("device", CALLS[0]), ("ragged", CALLS[1]), ("device", CALLS[2]), ("plain", [100] * 4), ("device", [100] * 4), ("ragged", [257, 0, 5, 257]),
             ("device", [1, 300, 7, 0]), ("plain", [40] * 4), ("device", CALLS[4])]
    calls = [lens for _, lens in forms]
    h, xs = _signal(43, 32, 250, calls, np.float32, np.float32, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    twin = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    f.set_timing(True)
    for i, (x, (form, lens)) in enumerate(zip(xs, forms)):
        n = max(lens)
        xd = torch.from_numpy(np.array(x)).cuda()
        ya, yb = (torch.zeros((4, f.outputlength_bound(n)), dtype=torch.float32, device="cuda") for _ in range(2))
        if form == "plain":
            ca, cb = f.filt_into(ya, xd), twin.filt_into(yb, xd)
        else:
            cb = twin.filt_into(yb, xd, lengths=lens)
            if form == "ragged":
                ca = f.filt_into(ya, xd, lengths=lens)
            else:
                ca = f.filt_rates_async(ya, xd, lengths=torch.tensor(lens, dtype=torch.int64, device="cuda"), max_length=n).cpu().numpy()
        assert list(ca) == list(cb), i
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), i
        assert f.last_kernel_name() == twin.last_kernel_name()
        assert _everything(f) == _everything(twin), i
        assert_bit_equal(f.history, twin.history, f"history after call {i}")
    launches, ms = f.timing_read()
    assert launches == len(calls) and ms > 0.0                               # one bracket a call, whichever form
    f.close(), twin.close()


def _get_states(pkg, f):
    """mrhip_get_channel_states itself: (status, message, the states it filled in)"""
    lib = pkg.load_library()
    out = (pkg.host.ChannelState * f._nch)()
    rc = lib.mrhip_get_channel_states(f._handle, C.cast(out, C.c_void_p))
    return rc, lib.mrhip_last_error().decode(), list(out)


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_refused_lengths_feed_their_channels_nothing(pkg, O, monkeypatch, torch_cuda, family, fast):
    """-1, max_length + 1, 2^40 and INT64_MIN in four of 67 channels of the second call: those channels write nothing and keep state and
    history bit for bit (the oracle is fed 0 samples there), their neighbours equal the oracle; the report, and what clears it"""
    torch = torch_cuda
    Nphi, hLen, tx = 32, 250, np.float32
    live = [c for c in range(67) if CALLS67[1][c] > 0]                       # the refused channels would have had samples
    fed = [list(c) for c in CALLS67]
    for c in (live[3], live[17], live[40], live[-1]):
        fed[1][c] = 0
    m = max(fed[1])                                                          # max_length of the call
    bad = {live[3]: -1, live[17]: m + 1, live[40]: 2 ** 40, live[-1]: I64_MIN}
    assert live[-1] > 63 and m > 256                                         # one of them in the second workgroup of the import
    h, xs = _signal(71, Nphi, hLen, fed, np.float32, tx, R67)
    outs, states, hists = _reference(pkg, O, 71, R67, Nphi, hLen, _poly(family, Nphi), fed, np.float32, tx, False)
    f = _filter(pkg, monkeypatch, family, h, R67, Nphi, tx, fast)
    counts, yh = _dev_call(torch, f, xs[0], fed[0], np.float32)
    _assert_call(f, counts, yh, outs[0], states[0], hists[0], "the call before")
    given = list(fed[1])
    for c, v in bad.items():
        given[c] = v
    y = torch.empty((67, f.outputlength_bound(m)), dtype=torch.float32, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    counts = f.filt_rates_async(y, torch.from_numpy(np.array(xs[1])).cuda(), lengths=torch.tensor(given, dtype=torch.int64, device="cuda"), max_length=m)
    counts, yh = counts.cpu().numpy(), y.cpu().numpy()
    want = [len(o) for o in outs[1]]
    assert list(counts) == want and all(counts[c] == 0 for c in bad)
    for c in range(67):
        assert_bit_equal(yh[c, :want[c]], outs[1][c], f"channel {c}")
        assert (yh[c, want[c]:].view(np.uint8) == POISON).all(), f"channel {c} wrote behind its count"      # a refused row: not one byte
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.channel_states
    assert e.value.code == 1 and "LENGTH was refused" in str(e.value) and "fed nothing" in str(e.value)
    rc, msg, got = _get_states(pkg, f)                                       # the states are filled in all the same
    assert rc == 1 and "LENGTH" in msg and [_state5(s) for s in got] == states[1] and [s.last_count for s in got] == want
    for c in bad:                                                            # ... and the refused channels stand where the call before left them
        assert _state5(got[c]) == states[0][c]
    hist = np.atleast_2d(f.history)
    for c in range(67):
        assert_bit_equal(hist[c], hists[1][c], f"history of channel {c}")
    f.set_channel_states([s.inputDeficit for s in got], [s.phiAccumulator for s in got])      # clears the mark, moves nothing
    _check_state(f, states[1], hists[1], "after set_channel_states")
    counts, yh = _dev_call(torch, f, xs[2], fed[2], np.float32)              # the stream goes on as the oracle's
    _assert_call(f, counts, yh, outs[2], states[2], hists[2], "the call after")
    # reset() clears it too
    f.filt_rates_async(y, torch.from_numpy(np.array(xs[1])).cuda(), lengths=torch.full((67,), -1, dtype=torch.int64, device="cuda"), max_length=m)
    assert _get_states(pkg, f)[0] == 1
    f.reset()
    assert [_state5(s) for s in f.channel_states] == [(1, 1.0, 1, 0.0, 1)] * 67
    f.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_a_refused_rate_is_reported_ahead_of_a_refused_length(pkg, monkeypatch, torch_cuda, family):
    torch = torch_cuda
    h, xs = _signal(73, 32, 250, CALLS, np.float32, np.float32, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, False)
    y = torch.zeros((4, f.outputlength_bound(257)), dtype=torch.float32, device="cuda")
    xd = torch.from_numpy(np.array(xs[0])).cuda()
    f.filt_rates_async(y, xd, lengths=torch.tensor([257, -1, 5, 257], dtype=torch.int64, device="cuda"), max_length=257)
    rc, msg, _ = _get_states(pkg, f)
    assert rc == 1 and "LENGTH" in msg
    f.set_channel_rates_device(torch.tensor([float("nan"), 32.0 / 3, 2.123, 2.123], dtype=torch.float64, device="cuda"), 0.005, 11.0)
    rc, msg, got = _get_states(pkg, f)
    assert rc == 1 and "mrhip_set_channel_rates_device" in msg and "rate was refused" in msg and "LENGTH" not in msg
    f.set_channel_states([s.inputDeficit for s in got], [s.phiAccumulator for s in got])      # clears both
    assert _get_states(pkg, f)[0] == 0
    f.close()


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_lengths_are_read_in_stream_order(pkg, monkeypatch, torch_cuda, family, fast):
    """twenty calls back to back with no wait on a stream that is busy when the first arrives: the ONE lengths tensor is written by
    torch arithmetic on the stream just before each call and overwritten by a fill right after it.  Checked once at the end, against
    the same calls made one at a time through the host ragged call on a twin filter."""
    torch = torch_cuda
    calls = [CALLS[i % 5] if i % 7 != 3 else [9, 0, 1500, 40] for i in range(20)]
    h, xs = _signal(53, 32, 250, calls[:8], np.float32, np.float32, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    twin = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, fast)
    xfull = torch.zeros((8, 4, 1500), dtype=torch.float32, device="cuda")
    for i, x in enumerate(xs):
        xfull[i, :, :x.shape[1]] = torch.from_numpy(np.array(x)).cuda()
    cap = f.outputlength_bound(1500)
    ys = torch.zeros((20, 4, cap), dtype=torch.float32, device="cuda")
    cnts = torch.full((20, 4), -1, dtype=torch.int64, device="cuda")
    halves = torch.tensor(calls, dtype=torch.int64, device="cuda")
    lens = torch.empty(4, dtype=torch.int64, device="cuda")
    busy = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    for _ in range(4):
        busy = busy @ busy * 1e-3                                            # (work in front of the first call on the stream)
    for i in range(20):
        torch.add(halves[i] * 2, -halves[i], out=lens)                       # the lengths: computed on the stream, just before the call
        f.filt_rates_async(ys[i], xfull[i % 8], lengths=lens, max_length=1500, counts=cnts[i])
        lens.fill_(-12345)                                                   # ... and gone right after it
    torch.cuda.synchronize()
    for i in range(20):
        y1 = torch.zeros((4, cap), dtype=torch.float32, device="cuda")
        c1 = twin.filt_into(y1, xfull[i % 8], lengths=list(calls[i]))
        assert cnts[i].cpu().tolist() == list(c1), i
        assert torch.equal(ys[i].view(torch.int32), y1.view(torch.int32)), i
    assert _everything(f) == _everything(twin)                               # (and no length was refused: channel_states answers)
    assert_bit_equal(f.history, twin.history, "history after the twenty calls")
    f.close(), twin.close()


@pytest.mark.parametrize("layout", ["tight", "A", "B", "C"])
@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("family", FAMILIES)
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, O, monkeypatch, torch_cuda, family, fast, layout):
    """poisoned backing stores, tight and odd-stride y layouts, on the first two calls of the sequence: no byte outside [0, count_c) of
    any row changes; the samples of row c of x at and behind lengths[c] are NaN, and the outputs are the oracle's"""
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
        counts = f.filt_rates_async(view, xback[:, ox:ox + n], lengths=torch.tensor(lens, dtype=torch.int64, device="cuda"), max_length=n).cpu().numpy()
        assert list(counts) == [len(o) for o in outs[i]] and min(counts) == 0 < max(counts)
        assert f.last_kernel_name() == KERNELS[(family, fast)]
        _assert_rows_only_written(backing, 4, cap, oy, pad, counts, outs[i], f"{family} {layout} call {i}")
        _check_state(f, states[i], hists[i], f"{family} {layout} call {i}")
    f.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_host_refusals_name_the_call_and_leave_everything_untouched(pkg, monkeypatch, torch_cuda, family):
    torch = torch_cuda
    lib = pkg.load_library()
    n = 300
    h, xs = _signal(9, 32, 250, [[n] * 4, [n] * 4], np.float32, np.float32, R4)
    f = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, False)
    prev = _filter(pkg, monkeypatch, family, h, R4, 32, np.float32, False)
    xd = [torch.from_numpy(np.array(x)).cuda() for x in xs]
    f.filt(xd[0], lengths=[n, 0, 5, n])                                      # (a stream in progress)
    before, hist_before = _everything(f), np.array(f.history)
    bound = f.outputlength_bound(n)
    y = torch.empty((4, bound), dtype=torch.float32, device="cuda")
    y.view(torch.uint8).fill_(POISON)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = torch.tensor([n, 0, 5, n], dtype=torch.int64, device="cuda")
    hnd, stream = f._handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, yp, cp, lp = C.c_void_p(xd[1].data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(good.data_ptr())

    def refused(name, rc, code, word=""):
        msg = lib.mrhip_last_error().decode()
        assert rc == code and name in msg and word in msg, (rc, code, msg)

    lens, chained = lib.mrhip_filt_device_rates_lens_device, lib.mrhip_filt_device_rates_chained
    other = pkg.FIRFilter(h, 2.123, 32).bind(np.float32, 4)
    long_n = (1 << 24) // 10                                                 # ceil(n * 32/3) + 2 > 2^24 entries a channel
    refused(LENS, lens(None, xp, lp, n, n, yp, bound, bound, cp, stream), 1, "NULL filter")
    refused(LENS, lens(hnd, xp, None, n, n, yp, bound, bound, cp, stream), 1, "x_lens is NULL")
    refused(LENS, lens(other._handle, xp, lp, n, n, yp, bound, bound, cp, stream), 1, "takes a filter of")
    refused(LENS, lens(hnd, xp, lp, -1, n, yp, bound, bound, cp, stream), 1, "negative x_len_max")
    refused(LENS, lens(hnd, xp, lp, n, n, yp, -1, bound, cp, stream), 1, "negative y_capacity")
    refused(LENS, lens(hnd, xp, lp, 2 ** 31 - 1, 2 ** 31, yp, bound, bound, cp, stream), 5, "2^31-1")
    refused(LENS, lens(hnd, None, lp, n, n, yp, bound, bound, cp, stream), 1, "x is NULL")
    refused(LENS, lens(hnd, xp, lp, n, n - 1, yp, bound, bound, cp, stream), 1, "x_stride < x_len_max")
    refused(LENS, lens(hnd, xp, lp, long_n, long_n, yp, 1 << 28, 1 << 28, cp, stream), 5, "2^24")
    refused(LENS, lens(hnd, xp, lp, n, n, yp, bound - 1, bound, cp, stream), 2, "needs room for")
    refused(LENS, lens(hnd, xp, lp, n, n, yp, bound, bound - 1, cp, stream), 2, "y_stride")
    refused(LENS, lens(hnd, xp, lp, n, n, None, bound, bound, cp, stream), 1, "y is NULL")
    # the chained call: the pair first, then the checks above in its own name
    refused(CHAINED, chained(hnd, None, xp, n, n, yp, bound, bound, cp, stream), 1, "NULL filter")
    refused(CHAINED, chained(other._handle, prev._handle, xp, n, n, yp, bound, bound, cp, stream), 1, "takes a filter of")
    refused(CHAINED, chained(hnd, hnd, xp, n, n, yp, bound, bound, cp, stream), 1, "prev is the filter itself")
    three = _filter(pkg, monkeypatch, family, h, R4[:3], 32, np.float32, False)
    refused(CHAINED, chained(hnd, three._handle, xp, n, n, yp, bound, bound, cp, stream), 1, "different numbers of channels")
    wide = _filter(pkg, monkeypatch, family, h.astype(np.float64), R4, 32, np.float64, False)
    refused(CHAINED, chained(hnd, wide._handle, xp, n, n, yp, bound, bound, cp, stream), 1, "sample dtype")
    refused(CHAINED, chained(hnd, prev._handle, xp, n, n, yp, bound, bound, cp, stream), 1, "has not been called since")
    refused(CHAINED, chained(hnd, other._handle, xp, n, n, yp, bound, bound, cp, stream), 1, "not planned on the device")
    prev.filt(xd[0], lengths=[n, 0, 5, n])
    prev.reset()
    refused(CHAINED, chained(hnd, prev._handle, xp, n, n, yp, bound, bound, cp, stream), 1, "has not been called since")      # reset: no call's counts
    prev.filt(xd[0], lengths=[n, 0, 5, n])
    refused(CHAINED, chained(hnd, prev._handle, xp, -1, n, yp, bound, bound, cp, stream), 1, "negative x_len_bound")
    refused(CHAINED, chained(hnd, prev._handle, None, n, n, yp, bound, bound, cp, stream), 1, "x is NULL")
    refused(CHAINED, chained(hnd, prev._handle, xp, n, n - 1, yp, bound, bound, cp, stream), 1, "x_stride < x_len_bound")
    refused(CHAINED, chained(hnd, prev._handle, xp, long_n, long_n, yp, 1 << 28, 1 << 28, cp, stream), 5, "2^24")
    refused(CHAINED, chained(hnd, prev._handle, xp, n, n, yp, bound - 1, bound, cp, stream), 2, "needs room for")
    refused(CHAINED, chained(hnd, prev._handle, xp, n, n, yp, bound, bound - 1, cp, stream), 2, "y_stride")
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        scratch.add_(1.0)                                                    # (so that the graph is not empty)
        rc1 = lens(hnd, xp, lp, n, n, yp, bound, bound, cp, C.c_void_p(s.cuda_stream))
        m1 = lib.mrhip_last_error().decode()
        rc2 = chained(hnd, prev._handle, xp, n, n, yp, bound, bound, cp, C.c_void_p(s.cuda_stream))
        m2 = lib.mrhip_last_error().decode()
    assert rc1 == 5 and "captur" in m1 and LENS in m1 and rc2 == 5 and "captur" in m2 and CHAINED in m2
    torch.cuda.synchronize()
    # the older chained call and the cascade keep refusing such filters, in their words
    assert lib.mrhip_filt_device_chained(hnd, other._handle, xp, n, n, yp, bound, bound, None, stream) != 0
    assert "mrhip_filt_device_chained" in lib.mrhip_last_error().decode()
    # nothing was enqueued, nothing written, the state is where it was
    assert (y.view(torch.uint8) == POISON).all().item() and not cnt.any().item()
    assert _everything(f) == before
    assert_bit_equal(np.array(f.history), hist_before, "history after the refused calls")
    for flt in (other, prev, three, wide, f):
        flt.close()


def _chain_inputs(seed, lens_per_call, tx):
    rng = np.random.default_rng(seed)
    xs = []
    for lens in lens_per_call:
        x = (rng.random((4, max(lens))) - 0.5).astype(tx)
        x.setflags(write=False)
        xs.append(x)
    return xs


R4B = [1.5, 0.75, 2.123, 0.3]                                                # the second stage's rates


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("families", [("arbitrary", "farrow"), ("farrow", "arbitrary")], ids=["arb-farrow", "farrow-arb"])
def test_a_chain_of_two_filters_with_per_channel_rates(pkg, O, monkeypatch, torch_cuda, families, fast):
    """three calls with ragged first-stage inputs, so that the first stage's counts differ and include 0: stage 2's outputs, counts,
    states and histories are the oracle's two-stage chain per channel; stage 1 is the oracle's first stage"""
    torch = torch_cuda
    Nphi, tx = 32, np.float32
    calls = CALLS[:3]
    assert any(0 in c for c in COUNTS[:3])                                   # ... and include 0
    h1, xs = _signal(81, Nphi, 250, calls, np.float32, tx, R4)
    h2, _ = _signal(82, Nphi, 100, calls, np.float32, tx, R4B)
    f1 = _filter(pkg, monkeypatch, families[0], h1, R4, Nphi, tx, fast)
    f2 = _filter(pkg, monkeypatch, families[1], h2, R4B, Nphi, tx, fast)
    r1 = [_oracle(pkg, O, h1, r, Nphi, _poly(families[0], Nphi), tx) for r in R4]
    r2 = [_oracle(pkg, O, h2, r, Nphi, _poly(families[1], Nphi), tx) for r in R4B]
    for i, (x, lens) in enumerate(zip(xs, calls)):
        mid = [r.filt(x[c, :lens[c]]) for c, r in enumerate(r1)]
        want = [r.filt(mid[c]) for c, r in enumerate(r2)]
        assert [len(m) for m in mid] == COUNTS[i] and len(set(COUNTS[i])) > 1             # the first stage's counts differ ...
        b1 = f1.outputlength_bound(max(lens))
        b2 = f2.outputlength_bound(b1)
        y1 = torch.zeros((4, b1), dtype=torch.float32, device="cuda")
        y2 = torch.zeros((4, b2), dtype=torch.float32, device="cuda")
        c1 = torch.empty(4, dtype=torch.int64, device="cuda")
        f1._filt_into_rates(y1, torch.from_numpy(np.array(x)).cuda(), counts=c1, lengths=lens)      # no wait ...
        c2 = f2.filt_rates_async(y2, y1, after=f1, max_length=b1)                                   # ... and none
        what = f"{families} call {i}"
        assert c1.cpu().tolist() == COUNTS[i], what
        _assert_call(f2, c2.cpu().numpy(), y2.cpu().numpy(), want, [_state5(r.state) for r in r2], [np.array(r.history) for r in r2], what)
        y1h = y1.cpu().numpy()
        for c in range(4):
            assert_bit_equal(y1h[c, :len(mid[c])], mid[c], f"{what}: stage 1, channel {c}")
        _check_state(f1, [_state5(r.state) for r in r1], [np.array(r.history) for r in r1], what + ": stage 1")
        assert f2.last_kernel_name() == KERNELS[(families[1], fast)]
    f1.close(), f2.close()


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "tiled-or-multi"])
@pytest.mark.parametrize("first", ["rational-3//5", "arbitrary"])
def test_a_filter_with_per_channel_rates_behind_a_one_state_filter(pkg, O, monkeypatch, torch_cuda, first, fast):
    """the common decimator (or resampler) in front, fed through filt_into_async: every channel of stage 2 is fed the first stage's one
    count, known on the device only"""
    torch = torch_cuda
    Nphi, tx = 32, np.float32
    sizes = [[257] * 4, [1] * 4, [1000] * 4]
    xs = _chain_inputs(91, sizes, tx)
    h2, _ = _signal(82, Nphi, 100, CALLS[:3], np.float32, tx, R4B)
    rng = np.random.default_rng(92)
    if first == "rational-3//5":
        h1 = (rng.standard_normal(60) / 5).astype(np.float32)
        f1 = pkg.FIRFilter(h1, Fraction(3, 5)).bind(tx, 4)
        r1 = [O.FIRFilter(h1, Fraction(3, 5), tx=tx) for _ in range(4)]
    else:
        h1 = (rng.standard_normal(250) * Nphi / 250).astype(np.float32)
        f1 = pkg.FIRFilter(h1, 0.37, Nphi).bind(tx, 4)
        r1 = [O.FIRFilter(h1, 0.37, Nphi, tx=tx) for _ in range(4)]
    f2 = _filter(pkg, monkeypatch, "arbitrary", h2, R4B, Nphi, tx, fast)
    r2 = [_oracle(pkg, O, h2, r, Nphi, None, tx) for r in R4B]
    for i, x in enumerate(xs):
        n = x.shape[1]
        mid = [r.filt(x[c]) for c, r in enumerate(r1)]
        want = [r.filt(mid[c]) for c, r in enumerate(r2)]
        b1 = f1.outputlength_bound(n)
        b2 = f2.outputlength_bound(b1)
        y1 = torch.zeros((4, b1), dtype=torch.float32, device="cuda")
        y2 = torch.zeros((4, b2), dtype=torch.float32, device="cuda")
        f1.filt_into_async(y1, torch.from_numpy(np.array(x)).cuda())
        c2 = f2.filt_rates_async(y2, y1, after=f1)                           # (max_length: the row length of y1, the bound)
        what = f"{first} call {i}"
        _assert_call(f2, c2.cpu().numpy(), y2.cpu().numpy(), want, [_state5(r.state) for r in r2], [np.array(r.history) for r in r2], what)
        assert f1.sync_state() == len(mid[0]), what                          # stage 1 is unaffected
        y1h = y1.cpu().numpy()
        for c in range(4):
            assert_bit_equal(y1h[c, :len(mid[c])], mid[c], f"{what}: stage 1, channel {c}")
    st, so = f1.state, r1[0].state
    assert (st.phiIdx, st.inputDeficit) == (so.phiIdx, so.inputDeficit)
    f1.close(), f2.close()
