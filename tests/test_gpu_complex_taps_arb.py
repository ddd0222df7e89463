"""GPU tests of FIRArbitrary with complex taps (csrc/kernels_ctaps_arb.hip; mrhip_create_arbitrary_ctaps,
FIRFilter.complex_taps_arbitrary).

Bar: arb_ctaps_tiled_kernel (MRHIP_CTAPS_TILED=1) == arb_ctaps_generic_kernel (MRHIP_CTAPS_TILED=0) ==
tests/complex_taps_arb_restatement.py, BIT FOR BIT -- outputs, per-call counts, end state and history -- and, for real samples,
== the untouched oracle by components (re(y) / im(y) are its outputs with the taps real(h) / imag(h)).  The restatement itself
is pinned to the oracle by tests/test_complex_taps_arb_cpu.py.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_arb_restatement import ComplexTapsArbitraryRestated
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NCH = 3
TYPES = [(np.complex64, np.float32), (np.complex128, np.float64), (np.complex64, np.complex64), (np.complex64, np.complex128),
         (np.complex128, np.complex64)]
RATES = [0.47, 1.0, 2.123, 32.0 / 3]
BANKS = [(4, 4), (4, 30), (32, 250), (32, 1024)]              # (Nphi, hLen): T = 1 (no history), 8, 8, 32
X_LENS = [1, 5, 257, 1500]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
GENERIC, TILED = "arb_ctaps_generic_kernel", "arb_ctaps_tiled_kernel"


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


def _signal(seed, hLen, x_len, th, tx, nch=NCH):
    rng = np.random.default_rng(seed)
    h = ((rng.standard_normal(hLen) + 1j * rng.standard_normal(hLen)) / hLen).astype(th)
    x = rng.random((nch, x_len)) - 0.5
    if np.dtype(tx).kind == "c":
        x = x + 1j * (rng.random((nch, x_len)) - 0.5)
    return h, x.astype(tx)


def _filter(pkg, monkeypatch, h, rate, Nphi, tx, nch, tiled):
    """a bound filter on the tiled kernel wherever its LDS plan fits (MRHIP_CTAPS_TILED=1) or on the universal one (=0)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.setenv("MRHIP_CTAPS_TILED", "1" if tiled else "0")
    return pkg.FIRFilter.complex_taps_arbitrary(h, rate, Nphi).bind(tx, nch)


def _oracle_by_components(O, h, rate, Nphi, x):
    """real samples: per channel, the oracle's outputs with the taps real(h) and imag(h), put together"""
    rt = np.float32 if h.dtype == np.complex64 else np.float64
    out = []
    for c in range(x.shape[0]):
        yr = O.FIRFilter(np.ascontiguousarray(h.real).astype(rt), rate, Nphi, tx=x.dtype).filt(x[c])
        yi = O.FIRFilter(np.ascontiguousarray(h.imag).astype(rt), rate, Nphi, tx=x.dtype).filt(x[c])
        y = np.empty(len(yr), dtype=np.complex64 if yr.dtype == np.float32 else np.complex128)
        y.real, y.imag = yr, yi
        out.append(y)
    return np.stack(out)


# ---- 1. shape sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th,tx", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("rate", RATES)
def test_shape_sweep_tiled_equals_universal_equals_restatement(pkg, monkeypatch, rate, th, tx):
    want_dtype = np.complex128 if (th == np.complex128 or np.dtype(tx) in (np.float64, np.complex128)) else np.complex64
    for Nphi, hLen in BANKS:
        for x_len in X_LENS:
            h, x = _signal(1000 * Nphi + hLen + x_len, hLen, x_len, th, tx)
            for name, how in CHUNKINGS.items():
                pieces = _chunks(x_len, how)
                refs = [ComplexTapsArbitraryRestated(h, rate, Nphi, tx=tx) for _ in range(NCH)]
                want = [[r.filt(x[c, a:b], scalar=False) for a, b in pieces] for c, r in enumerate(refs)]
                for tiled in (False, True):
                    what = f"Nphi {Nphi} hLen {hLen} x_len {x_len} {name} tiled={tiled}"
                    f = _filter(pkg, monkeypatch, h, rate, Nphi, tx, NCH, tiled)
                    assert f.output_dtype == want_dtype
                    for i, (a, b) in enumerate(pieces):
                        y = f.filt(np.ascontiguousarray(x[:, a:b]))
                        assert y.dtype == want_dtype and y.shape == (NCH, len(want[0][i])), (what, a, b, y.shape)
                        for c in range(NCH):
                            assert_bit_equal(y[c], want[c][i], f"{what} chunk [{a}, {b}) channel {c}")
                        if y.shape[1] > 0:
                            assert f.last_kernel_name() == (TILED if tiled else GENERIC), what
                    st = f.state
                    assert st.kind == 4 and st.tap_dtype == (3 if th == np.complex128 else 2)
                    assert (st.inputDeficit, st.phiAccumulator, st.phiIdx, st.alpha) == \
                        (refs[0].inputDeficit, refs[0].phiAccumulator, refs[0].phiIdx, refs[0].alpha), what
                    hist = f.history.reshape(NCH, -1)
                    assert hist.dtype == np.dtype(tx)
                    for c in range(NCH):
                        assert_bit_equal(hist[c], refs[c].history_array(), f"{what} history {c}")
                    f.close()


# ---- 2. a tile whose run exceeds the planned span ----------------------------------------------------------------------------------
def test_over_span_tiles_read_global_memory_and_equal_the_universal_kernel_and_the_oracle(pkg, O, monkeypatch):
    """rate 1/50: a full tile of 256 outputs runs over 12 750 samples, more than the 40 KiB of samples the plan gives a tile
    (10 240 Float32 samples): the three full tiles read their windows from global memory, the last (32 outputs) is staged"""
    rate, Nphi, hLen, x_len, nch = 1.0 / 50, 32, 250, 40_000, 2
    h, x = _signal(7, hLen, x_len, np.complex64, np.float32, nch=nch)
    ys = {}
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, h, rate, Nphi, np.float32, nch, tiled)
        ys[tiled] = f.filt(x)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        ys[tiled, "hist"], ys[tiled, "state"] = f.history, (f.state.inputDeficit, f.state.phiAccumulator)
        f.close()
    assert ys[True].shape == (nch, 800)
    assert_bit_equal(ys[True], ys[False], "tiled == universal")
    assert_bit_equal(ys[True, "hist"], ys[False, "hist"], "history")
    assert ys[True, "state"] == ys[False, "state"]
    assert_bit_equal(ys[True], _oracle_by_components(O, h, rate, Nphi, x), "oracle by components")


# ---- 3. channel groups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 5, 9, 33])
def test_channel_groups_every_cpl_and_a_ragged_last_group(pkg, O, monkeypatch, nch):
    rate, Nphi, hLen, x_len = math.pi / 3, 32, 250, 2000
    h, x = _signal(50 + nch, hLen, x_len, np.complex64, np.float32, nch=nch)
    want = _oracle_by_components(O, h, rate, Nphi, x)
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, h, rate, Nphi, np.float32, nch, tiled)
        y = f.filt(x).reshape(nch, -1)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert_bit_equal(y, want, f"{nch} channels, tiled={tiled}")
        f.close()


# ---- 4. a call that mrhip_filt_device splits into pieces ------------------------------------------------------------------------------
def test_split_call_places_every_piece_by_the_output_element_size(pkg, O, monkeypatch, torch_cuda):
    """MRHIP_LAUNCH_MAX=4099: eight pieces; real samples and a complex output -- a y offset taken in sample-size units would put
    every piece after the first at half its place"""
    torch = torch_cuda
    rate, Nphi, hLen, x_len, nch = 1.37, 32, 250, 30_011, 2
    h, x = _signal(9, hLen, x_len, np.complex64, np.float32, nch=nch)
    want = _oracle_by_components(O, h, rate, Nphi, x)
    xd = torch.from_numpy(x).cuda()
    monkeypatch.setenv("MRHIP_LAUNCH_MAX", "4099")
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, h, rate, Nphi, np.float32, nch, tiled)
        y = f.filt(xd).cpu().numpy()
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert_bit_equal(y, want, f"split call, tiled={tiled}")
        assert_bit_equal(f.history.reshape(nch, -1)[1], x[1, -(f.historyLen):], "history")
        f.close()


# ---- 5. asynchronous and captured calls -------------------------------------------------------------------------------------
def _sync_stream(pkg, monkeypatch, h, rate, Nphi, x, chunk, n):
    f = _filter(pkg, monkeypatch, h, rate, Nphi, x.dtype, x.shape[0], tiled=False)
    out = [f.filt(np.ascontiguousarray(x[:, i * chunk:(i + 1) * chunk])).reshape(x.shape[0], -1) for i in range(n)]
    st = f.state
    hist = f.history
    f.close()
    return out, (st.inputDeficit, st.phiAccumulator), hist


@pytest.mark.parametrize("tiled", [False, True])
def test_async_calls_equal_the_synchronous_stream(pkg, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, chunk, n = 2.123, 32, 250, 96, 5
    h, x = _signal(21, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _sync_stream(pkg, monkeypatch, h, rate, Nphi, x, chunk, n)
    f = _filter(pkg, monkeypatch, h, rate, Nphi, np.complex64, NCH, tiled)
    xd = torch.from_numpy(x).cuda()
    bound = f.outputlength_bound(chunk)
    ys = torch.zeros((n, NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i in range(n):
        f.filt_into_async(ys[i], xd[:, i * chunk:(i + 1) * chunk], cnt[i:i + 1])
    last = f.sync_state()
    assert f.last_kernel_name() == (TILED if tiled else GENERIC)      # both kernels take the count from the call record
    counts = cnt.cpu().tolist()
    assert counts == [w.shape[1] for w in want] and last == counts[-1]
    for i in range(n):
        assert_bit_equal(ys[i, :, :counts[i]].cpu().numpy(), want[i], f"asynchronous call {i}")
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


@pytest.mark.parametrize("tiled", [False, True])
def test_captured_call_replayed_three_times_equals_the_synchronous_stream(pkg, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, chunk, n = 2.123, 32, 250, 96, 5               # chunk >= historyLen (7)
    h, x = _signal(22, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _sync_stream(pkg, monkeypatch, h, rate, Nphi, x, chunk, n)
    f = _filter(pkg, monkeypatch, h, rate, Nphi, np.complex64, NCH, tiled)
    xd = torch.from_numpy(x).cuda()
    # The stream starts with a plain call and an asynchronous one of the captured size: the schedule's work buffers are allocated
    # by the first device-planned call of a size (allocations cannot be captured).  The graph takes the stream over from there.
    assert_bit_equal(f.filt(xd[:, :chunk].contiguous()).cpu().numpy(), want[0], "plain call")
    bound = f.outputlength_bound(chunk)
    y1 = torch.zeros((NCH, bound), dtype=torch.complex64, device="cuda")
    f.filt_into_async(y1, xd[:, chunk:2 * chunk])
    c1 = f.sync_state()
    assert_bit_equal(y1[:, :c1].cpu().numpy(), want[1], "asynchronous call of the captured size")
    xs = torch.zeros((NCH, chunk), dtype=torch.complex64, device="cuda")
    ys = torch.zeros((NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        f.filt_into_async(ys, xs, cnt)
    for i in range(2, n):
        xs.copy_(xd[:, i * chunk:(i + 1) * chunk])
        g.replay()
        torch.cuda.synchronize()
        c = int(cnt.cpu()[0])
        assert c == want[i].shape[1]
        assert_bit_equal(ys[:, :c].cpu().numpy(), want[i], f"replay {i}")
    f.sync_state()
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


# ---- 6. tapsforphase, get_taps, reset ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [np.complex64, np.complex128])
def test_tapsforphase_get_taps_and_reset(pkg, monkeypatch, th):
    rate, Nphi, hLen, x_len = 0.47, 4, 30, 300
    h, x = _signal(31, hLen, x_len, th, np.float32, nch=1)
    r = ComplexTapsArbitraryRestated(h, rate, Nphi, tx=np.float32)
    f = _filter(pkg, monkeypatch, h, rate, Nphi, np.float32, 1, tiled=True)
    assert_bit_equal(f.taps(0), r.pfb, "pfb as stored")
    assert_bit_equal(f.taps(1), r.dpfb, "dpfb as stored")
    for phase in (1.0, 1.25, Nphi + 0.5):
        t = f.tapsforphase(phase)
        assert t.dtype == th
        assert_bit_equal(t, r.tapsforphase(phase), f"tapsforphase({phase})")
    for bad in (0.5, Nphi + 1.0, -1.0):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.tapsforphase(bad)
        assert e.value.code == 1
    y1 = f.filt(x[0])
    assert_bit_equal(y1, r.filt(x[0], scalar=False), "first run")
    f.reset()
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == (1, 1.0) and not f.history.any()
    assert_bit_equal(f.filt(x[0]), y1, "reset, then the same again")
    f.close()


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------
def test_contract_edges(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    lib = pkg.load_library()
    F32, F64, C64, C128 = 0, 1, 2, 3
    h = np.full(8, 0.5 - 0.25j, dtype=np.complex64)
    f = _filter(pkg, monkeypatch, h, 1.5, 4, np.float32, 1, tiled=True)
    assert lib.mrhip_set_numerics(f._handle, 1) == 5            # FUSED: no fused form is defined
    assert lib.mrhip_set_numerics(f._handle, 0) == 0
    # buffer too small: raised before any work, the state stays
    xd = torch.ones(100, dtype=torch.float32, device="cuda")
    small = torch.zeros(10, dtype=torch.complex64, device="cuda")
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.filt_into(small, xd)
    assert e.value.code == 2
    assert (f.state.inputDeficit, f.state.phiAccumulator) == (1, 1.0) and not f.history.any()
    want = ComplexTapsArbitraryRestated(h, 1.5, 4, tx=np.float32).filt(np.ones(100, dtype=np.float32), scalar=False)
    assert_bit_equal(f.filt(xd).cpu().numpy(), want, "the same call with room")
    f.close()
    out = C.c_void_p()
    for th, hh in ((F32, h.real.astype(np.float32)), (F64, h.real.astype(np.float64))):      # real taps: the existing constructor
        assert lib.mrhip_create_arbitrary_ctaps(hh.ctypes.data_as(C.c_void_p), len(hh), th, 1.5, 4, F32, 1, 0, C.byref(out)) == 1
        assert not out.value
    for th, hh in ((C64, h), (C128, h.astype(np.complex128))):
        p = hh.ctypes.data_as(C.c_void_p)
        assert lib.mrhip_create_arbitrary(p, len(hh), th, 1.5, 4, F32, 1, 0, C.byref(out)) == 5 and not out.value
        assert "rational family" in lib.mrhip_last_error().decode()
        assert lib.mrhip_create_farrow(p, len(hh), th, 1.5, 4, 2, F32, 1, 0, C.byref(out)) == 5 and not out.value
        assert lib.mrhip_create_arbitrary_ctaps(p, len(hh), th, -1.0, 4, F32, 1, 0, C.byref(out)) == 1 and not out.value
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.ShardedFIRFilter(h, 1.5, 2, [0], Nphi=4)                # sharded filters keep refusing complex taps
    assert e.value.code == 5


def test_cascade_takes_such_a_stage_through_the_per_stage_calls(pkg, monkeypatch, torch_cuda):
    """a cascade runs its stages as plain calls, so a complex-tap FIRArbitrary is a stage like any FIRArbitrary: Float32 in,
    Complex64 between the stages, a real-tap decimator behind it == the two filters called by hand"""
    torch = torch_cuda
    h, x = _signal(41, 250, 3000, np.complex64, np.float32, nch=2)
    h2 = np.random.default_rng(42).standard_normal(16).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    monkeypatch.setenv("MRHIP_CTAPS_TILED", "1")
    a, b = pkg.FIRFilter.complex_taps_arbitrary(h, 2.123, 32), pkg.FIRFilter(h2, Fraction(1, 2))
    by_hand = b.filt(a.filt(xd))
    cas = pkg.FilterCascade(pkg.FIRFilter.complex_taps_arbitrary(h, 2.123, 32), pkg.FIRFilter(h2, Fraction(1, 2)))
    y = cas.filt(xd)
    assert cas.stages[0].last_kernel_name() == TILED and y.dtype == torch.complex64
    assert_bit_equal(y.cpu().numpy(), by_hand.cpu().numpy(), "cascade == by hand")
    cas.close(), a.close(), b.close()


# ---- 8. known answer -------------------------------------------------------------------------------------------------------------
def test_known_answer_running_sum(pkg, monkeypatch):
    """h = (1+1im) * ones(Nphi * T), x = ones: every column of pfb is (1+1im) * ones(T) and dh = [diff(h), 0] is zero, so
    dpfb is zero and yUpper * α adds nothing.  Rate 1.0: Δ = Nphi, the accumulator stays 1.0 and every sample gives an output,
    y[k] = (1+1im) * min(k, T), the running sum of the ones that have arrived.  Rate 0.5: Δ = 2 Nphi, every second sample
    (1, 3, 5, ...) gives one: y[k] = (1+1im) * min(2k - 1, T)."""
    Nphi, T = 4, 3
    h = np.full(Nphi * T, 1 + 1j, dtype=np.complex64)
    x = np.ones(10, dtype=np.float32)
    k = np.arange(1, 11)
    for tiled in (False, True):
        for rate, arrived in ((1.0, k), (0.5, 2 * k[:5] - 1)):
            f = _filter(pkg, monkeypatch, h, rate, Nphi, np.float32, 1, tiled)
            assert np.array_equal(f.taps(0), np.full((T, Nphi), 1 + 1j)) and not f.taps(1).any()
            y = f.filt(x)
            assert y.dtype == np.complex64
            assert np.array_equal(y, (np.minimum(arrived, T) * (1 + 1j)).astype(np.complex64)), (tiled, rate, y)
            f.close()
