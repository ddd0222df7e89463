"""GPU tests of the complex-tap kernels (csrc/kernels_ctaps.hip): FIRFilter(h::Vector{Complex}, ratio) for the rational family.

Bar: poly_ctaps_tiled_kernel == poly_ctaps_generic_kernel (MRHIP_FORCE_GENERIC) == tests/complex_taps_restatement.py, BIT FOR
BIT -- outputs, per-call counts, end state and history -- for whole and chunked feeding (chunks shorter than the history
included) and every (tap, sample) type pair the contract in include/multirate_hip.h ("Complex taps") allows.  The restatement
itself is pinned to the oracle by tests/test_complex_taps_cpu.py.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_restatement import ComplexTapsRestated, taps2pfb
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NCH = 3
# (L, M, hLen, x_len): FIRStandard, FIRDecimator, FIRInterpolator, FIRRational, and the headline ratio
SHAPES = [(1, 1, 17, 700), (1, 3, 33, 700), (4, 1, 30, 700), (3, 2, 50, 700), (147, 160, 3 * 147 + 5, 2000)]
TYPES = [(np.complex64, np.float32), (np.complex64, np.complex64), (np.complex64, np.float64),
         (np.complex128, np.float32), (np.complex64, np.complex128), (np.complex128, np.complex128)]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
GENERIC, TILED = "poly_ctaps_generic_kernel", "poly_ctaps_tiled_kernel"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _tdtype(torch, d):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128}[np.dtype(d)]


def _chunks(n, how):
    if how is None:
        return [(0, n)]
    if isinstance(how, int):
        return [(a, min(a + how, n)) for a in range(0, n, how)]
    out, pos = [], 0
    for c in how:
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


def _filter(pkg, monkeypatch, h, ratio, tx, nch, generic):
    """a bound filter on the universal kernel (MRHIP_FORCE_GENERIC is read when the device object is created) or with the
    tiled kernel forced wherever its LDS plan fits (MRHIP_CTAPS_TILED=1: the default plan also asks for a chip-filling call)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "1" if generic else "0")
    monkeypatch.setenv("MRHIP_CTAPS_TILED", "1")
    return pkg.FIRFilter.complex_taps(h, ratio).bind(tx, nch)


@pytest.mark.parametrize("th,tx", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("L,M,hLen,x_len", SHAPES)
def test_shape_sweep_tiled_equals_universal_equals_restatement(pkg, monkeypatch, L, M, hLen, x_len, th, tx):
    h, x = _signal(1000 * L + M, hLen, x_len, th, tx)
    ratio = Fraction(L, M)
    want_dtype = np.complex128 if (th == np.complex128 or np.dtype(tx) in (np.float64, np.complex128)) else np.complex64
    for name, how in CHUNKINGS.items():
        pieces = _chunks(x_len, how)
        refs = [ComplexTapsRestated(h, ratio, tx=tx) for _ in range(NCH)]
        want = [[r.filt(x[c, a:b]) for a, b in pieces] for c, r in enumerate(refs)]
        for generic in (True, False):
            f = _filter(pkg, monkeypatch, h, ratio, tx, NCH, generic)
            assert f.output_dtype == want_dtype
            for i, (a, b) in enumerate(pieces):
                y = f.filt(np.ascontiguousarray(x[:, a:b]))
                assert y.dtype == want_dtype and y.shape == (NCH, len(want[0][i])), (name, generic, a, b, y.shape)
                for c in range(NCH):
                    assert_bit_equal(y[c], want[c][i], f"{name} generic={generic} chunk [{a}, {b}) channel {c}")
                if y.shape[1] > 0:
                    assert f.last_kernel_name() == (GENERIC if generic else TILED)
            st = f.state
            assert st.tap_dtype == (3 if th == np.complex128 else 2)
            assert (st.phiIdx, st.inputDeficit) == (refs[0].phiIdx, refs[0].inputDeficit), (name, generic)
            hist = f.history.reshape(NCH, -1)
            assert hist.dtype == np.dtype(tx)
            for c in range(NCH):
                assert_bit_equal(hist[c], refs[c].history_array(), f"{name} generic={generic} history {c}")
            f.close()


def test_device_tensors_chunked_entry_reset_state_and_taps(pkg, monkeypatch, torch_cuda):
    """mrhip_filt_device / _chunked on device tensors, reset, set_state + set_history, get_taps"""
    torch = torch_cuda
    L, M, hLen, x_len = 3, 2, 50, 700
    h, x = _signal(5, hLen, x_len, np.complex64, np.float32)
    ratio = Fraction(L, M)
    refs = [ComplexTapsRestated(h, ratio, tx=np.float32) for _ in range(NCH)]
    want = np.stack([r.filt(x[c]) for c, r in enumerate(refs)])
    xd = torch.from_numpy(x).cuda()
    f = _filter(pkg, monkeypatch, h, ratio, np.float32, NCH, generic=False)
    assert_bit_equal(f.taps(), taps2pfb(h, L), "taps as stored")
    assert_bit_equal(f.filt(xd).cpu().numpy(), want, "device tensors, whole")
    f.reset()
    yb = torch.zeros((NCH, want.shape[1]), dtype=torch.complex64, device="cuda")
    assert f.filt_into_chunked(yb, xd, 97) == want.shape[1]
    assert_bit_equal(yb.cpu().numpy(), want, "mrhip_filt_device_chunked")
    # enter the stream in the middle: state and history of the first 301 samples, then the rest
    mid = [ComplexTapsRestated(h, ratio, tx=np.float32) for _ in range(NCH)]
    head = np.stack([r.filt(x[c, :301]) for c, r in enumerate(mid)])
    f.reset()
    f.set_state(mid[0].phiIdx, mid[0].inputDeficit)
    f.set_history(np.stack([r.history_array() for r in mid]))
    tail = f.filt(np.ascontiguousarray(x[:, 301:]))
    assert_bit_equal(np.concatenate([head, tail], axis=1), want, "set_state + set_history, then the rest")
    f.close()


def test_plan_accepts_a_chip_filling_call_and_rejects_small_and_oversized_ones(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen = 3, 2, 50
    h, x = _signal(11, hLen, 60_000, np.complex64, np.complex64)
    xd = torch.from_numpy(x).cuda()
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "1")
    fg = pkg.FIRFilter.complex_taps(h, Fraction(L, M)).bind(np.complex64, NCH)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.delenv("MRHIP_CTAPS_TILED", raising=False)
    ft = pkg.FIRFilter.complex_taps(h, Fraction(L, M)).bind(np.complex64, NCH)
    # 3 x 90 000 outputs: more tiles than the chip has CUs -> the default plan takes the call
    y_t, y_g = ft.filt(xd), fg.filt(xd)
    assert ft.last_kernel_name() == TILED and fg.last_kernel_name() == GENERIC
    assert_bit_equal(y_t.cpu().numpy(), y_g.cpu().numpy(), "tiled == universal, chip-filling call")
    # 3 x 1050 outputs: a dozen tiles -> the default plan leaves the call to the universal kernel
    y_t, y_g = ft.filt(xd[:, :700].contiguous()), fg.filt(xd[:, :700].contiguous())
    assert ft.last_kernel_name() == GENERIC
    assert_bit_equal(y_t.cpu().numpy(), y_g.cpu().numpy(), "continuation on the universal kernel")
    # switched off
    monkeypatch.setenv("MRHIP_CTAPS_TILED", "0")
    ft.filt(xd)
    assert ft.last_kernel_name() == GENERIC
    ft.close(), fg.close()
    # a bank of 13 000 pairs of Float32 (104 KB) does not fit the LDS plan even when the tiled kernel is forced
    monkeypatch.setenv("MRHIP_CTAPS_TILED", "1")
    hb, xb = _signal(12, 13_000, 300, np.complex64, np.float32, nch=1)
    fb = pkg.FIRFilter.complex_taps(hb, 1).bind(np.float32, 1)
    yb = fb.filt(xb)
    assert fb.last_kernel_name() == GENERIC and yb.shape == (1, 300)
    # (value check against NumPy's own complex dot: not bit-level, the restatement of 3.9e6 scalar products is too slow here)
    ext = np.concatenate([np.zeros(12_999, np.float32), xb[0]])
    ref = np.array([np.dot(hb[::-1].astype(np.complex128), ext[k:k + 13_000]) for k in range(300)])
    assert np.max(np.abs(yb[0] - ref)) < 1e-4
    fb.close()


def _sync_stream(pkg, monkeypatch, h, ratio, x, chunk, n):
    f = _filter(pkg, monkeypatch, h, ratio, x.dtype, x.shape[0], generic=True)
    out = [f.filt(np.ascontiguousarray(x[:, i * chunk:(i + 1) * chunk])) for i in range(n)]
    st = f.state
    hist = f.history
    f.close()
    return out, (st.phiIdx, st.inputDeficit), hist


def test_async_calls_equal_the_synchronous_stream(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 2, 50, 96, 5
    h, x = _signal(21, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _sync_stream(pkg, monkeypatch, h, Fraction(L, M), x, chunk, n)
    f = _filter(pkg, monkeypatch, h, Fraction(L, M), np.complex64, NCH, generic=False)
    xd = torch.from_numpy(x).cuda()
    bound = f.outputlength_bound(chunk)
    ys = torch.zeros((n, NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i in range(n):
        f.filt_into_async(ys[i], xd[:, i * chunk:(i + 1) * chunk], cnt[i:i + 1])
    last = f.sync_state()
    assert f.last_kernel_name() == GENERIC                     # the device-planned path: the universal complex-tap kernel
    counts = cnt.cpu().tolist()
    assert counts == [w.shape[1] for w in want] and last == counts[-1]
    for i in range(n):
        assert_bit_equal(ys[i, :, :counts[i]].cpu().numpy(), want[i], f"asynchronous call {i}")
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


def test_captured_call_replayed_three_times_equals_the_synchronous_stream(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 2, 50, 96, 3
    h, x = _signal(22, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _sync_stream(pkg, monkeypatch, h, Fraction(L, M), x, chunk, n)
    f = _filter(pkg, monkeypatch, h, Fraction(L, M), np.complex64, NCH, generic=False)
    xd = torch.from_numpy(x).cuda()
    bound = f.outputlength_bound(chunk)
    xs = torch.zeros((NCH, chunk), dtype=torch.complex64, device="cuda")
    ys = torch.zeros((NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        f.filt_into_async(ys, xs, cnt)
    for i in range(n):
        xs.copy_(xd[:, i * chunk:(i + 1) * chunk])
        g.replay()
        torch.cuda.synchronize()
        c = int(cnt.cpu()[0])
        assert c == want[i].shape[1]
        assert_bit_equal(ys[:, :c].cpu().numpy(), want[i], f"replay {i}")
    f.sync_state()
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


def test_known_answer_running_sum(pkg, monkeypatch):
    """h = [1+1im, 1+1im, 1+1im], x = 1:12, ratio 1//1: y = s (1+1im), s the running 3-sum"""
    x = np.arange(1, 13, dtype=np.float32)
    s = x + np.concatenate([[0], x[:-1]]) + np.concatenate([[0, 0], x[:-2]])
    for generic in (True, False):
        f = _filter(pkg, monkeypatch, np.full(3, 1 + 1j, dtype=np.complex64), 1, np.float32, 1, generic)
        y = f.filt(x)
        assert y.dtype == np.complex64
        assert np.array_equal(y, (s * (1 + 1j)).astype(np.complex64))
        f.close()


def test_contract_edges(pkg, monkeypatch):
    lib = pkg.load_library()
    F32, C64, C128 = 0, 2, 3
    h = np.full(8, 0.5 - 0.25j, dtype=np.complex64)
    f = pkg.FIRFilter.complex_taps(h, Fraction(1, 2)).bind(np.float32, 1)
    assert lib.mrhip_set_numerics(f._handle, 1) == 5            # FUSED: no fused form is defined
    assert lib.mrhip_set_numerics(f._handle, 0) == 0
    f.close()
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter(h)                                         # the plain constructor still refuses
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.complex_taps(h, 1.5)
    assert e.value.code == 5
    ptr = h.ctypes.data_as(C.c_void_p)
    for th, hh in ((C64, h), (C128, h.astype(np.complex128))):
        p = hh.ctypes.data_as(C.c_void_p)
        out = C.c_void_p()
        assert lib.mrhip_create_arbitrary(p, len(hh), th, 1.5, 4, F32, 1, 0, C.byref(out)) == 5 and not out.value
        assert "rational family" in lib.mrhip_last_error().decode()
        assert lib.mrhip_create_farrow(p, len(hh), th, 1.5, 4, 2, F32, 1, 0, C.byref(out)) == 5 and not out.value
    del ptr


def test_ring_is_not_resident_and_equals_the_plain_stream(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 2, 50, 96, 4
    h, x = _signal(31, hLen, chunk * n, np.complex64, np.complex64)
    want, state, _ = _sync_stream(pkg, monkeypatch, h, Fraction(L, M), x, chunk, n)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.delenv("MRHIP_CTAPS_TILED", raising=False)
    f = pkg.FIRFilter.complex_taps(h, Fraction(L, M)).bind(np.complex64, NCH)
    xd = torch.from_numpy(x).cuda()
    total = sum(w.shape[1] for w in want)
    yb = torch.zeros((NCH, total), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    with f.open_ring() as ring:
        assert ring.info()["resident"] is False
        got, _ = ring.push_chunks(yb, xd, chunk)
        ring.drain()
    assert got == total
    assert_bit_equal(yb.cpu().numpy(), np.concatenate(want, axis=1), "ring output")
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    f.close()
