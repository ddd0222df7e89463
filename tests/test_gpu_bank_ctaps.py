"""GPU tests of the per-channel complex-tap kernels (csrc/kernels_bank_ctaps.hip): FIRFilter.per_channel_complex_taps(H, ratio), one
FIRFilter(H[c]::Vector{Complex}, ratio) per channel behind one filter object (mrhip_create_rational_bank_ctaps).

Bar (include/multirate_hip.h, "Per-channel complex taps"): for every channel c the outputs, the per-call counts, the end state and the
history are BIT FOR BIT those of tests/complex_taps_restatement.py's ComplexTapsRestated(H[c], ratio, tx) fed x[c] -- on
poly_bank_ctaps_generic_kernel (MRHIP_FORCE_GENERIC=1) and on poly_bank_ctaps_tiled_kernel (MRHIP_BANK_CTAPS_TILED=1), whole and chunked (a
one-sample chunk, an empty one, chunks shorter than the history), host- and device-planned.  No tolerance anywhere, except in the one
sanity check of an oversized bank the restatement is too slow for.  The restatement itself is pinned to the oracle by
tests/test_complex_taps_cpu.py.
"""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_restatement import ComplexTapsRestated, taps2pfb
from conftest import assert_bit_equal
from test_gpu_complex_taps import TYPES

pytestmark = pytest.mark.gpu

NCH = 3
# (L, M, hLen, x_len): FIRStandard and FIRDecimator (the seam), FIRInterpolator with hLen no multiple of L (padded zeros), two FIRRational,
# the headline ratio
SHAPES = [(1, 1, 5, 300), (1, 3, 7, 300), (3, 1, 10, 300), (3, 5, 11, 400), (7, 4, 30, 400), (147, 160, 147 * 3 + 5, 2000)]
FEW_TYPES = [(np.complex64, np.float32), (np.complex64, np.complex64)]
CASES = [((3, 5, 11, 400), t) for t in TYPES] + [(s, t) for s in SHAPES if s[:2] != (3, 5) for t in FEW_TYPES]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
GENERIC, TILED = "poly_bank_ctaps_generic_kernel", "poly_bank_ctaps_tiled_kernel"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _tdtype(torch, d):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128}[np.dtype(d)]


def _out_dtype(th, tx):
    f64 = np.dtype(th) == np.complex128 or np.dtype(tx) in (np.dtype(np.float64), np.dtype(np.complex128))
    return np.dtype(np.complex128 if f64 else np.complex64)


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


@functools.lru_cache(maxsize=None)
def _signal(seed, hLen, x_len, th, tx, nch=NCH):
    """rows that tell channels apart: row 0 random complex, row 1 a single 1+0j at tap 0 (the channel's output is its own input passed
    through the polyphase schedule), row 2 = -conj(row 0 reversed); further rows random"""
    rng = np.random.default_rng(seed)
    H = ((rng.standard_normal((nch, hLen)) + 1j * rng.standard_normal((nch, hLen))) / hLen).astype(th)
    if nch > 1:
        H[1] = 0
        H[1, 0] = 1
    if nch > 2:
        H[2] = -np.conj(H[0][::-1])
    x = rng.random((nch, x_len)) - 0.5
    if np.dtype(tx).kind == "c":
        x = x + 1j * (rng.random((nch, x_len)) - 0.5)
    x = x.astype(tx)
    H.setflags(write=False), x.setflags(write=False)
    return H, x


_REFS = {}


def _reference(seed, L, M, hLen, x_len, th, tx, how, nch=NCH):
    """the restatement per channel, one ComplexTapsRestated(H[c], ratio, tx) fed x[c] in the pieces of `how`: (outputs [c][piece],
    (phiIdx, inputDeficit), histories [c]); computed once per case and shared"""
    key = (seed, L, M, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), nch)
    if key not in _REFS:
        H, x = _signal(seed, hLen, x_len, th, tx, nch)
        refs = [ComplexTapsRestated(H[c], Fraction(L, M), tx=tx) for c in range(nch)]
        outs = [[r.filt(x[c, a:b]) for a, b in _chunks(x_len, how)] for c, r in enumerate(refs)]
        states = {(r.phiIdx, r.inputDeficit) for r in refs}
        assert len(states) == 1                                   # (the state does not depend on the taps)
        _REFS[key] = (outs, states.pop(), [r.history_array() for r in refs])
    return _REFS[key]


def _filter(pkg, monkeypatch, H, ratio, tx, generic, grid=None):
    """a bound filter on the universal kernel (MRHIP_FORCE_GENERIC is read when the device object is created) or with the tiled kernel
    wherever its LDS plan fits (MRHIP_BANK_CTAPS_TILED=1)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "1" if generic else "0")
    monkeypatch.setenv("MRHIP_BANK_CTAPS_TILED", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_BANK_CTAPS_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_BANK_CTAPS_GRID", str(grid))
    return pkg.FIRFilter.per_channel_complex_taps(H, ratio).bind(tx, H.shape[0])


def _run_case(pkg, monkeypatch, shape, th, tx, nch=NCH, grid=None, chunkings=CHUNKINGS):
    L, M, hLen, x_len = shape
    seed = 1000 * L + M
    H, x = _signal(seed, hLen, x_len, th, tx, nch)
    want_dtype = _out_dtype(th, tx)
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        want, state, hists = _reference(seed, L, M, hLen, x_len, th, tx, how, nch)
        for generic in (True, False):
            f = _filter(pkg, monkeypatch, H, Fraction(L, M), tx, generic, grid)
            assert f.output_dtype == want_dtype
            for i, (a, b) in enumerate(pieces):
                y = f.filt(np.ascontiguousarray(x[:, a:b]))
                assert y.dtype == want_dtype and y.shape == (nch, len(want[0][i])), (name, generic, a, b, y.shape)   # the per-call count
                for c in range(nch):
                    assert_bit_equal(y[c], want[c][i], f"{name} generic={generic} chunk [{a}, {b}) channel {c}")
                if y.shape[1] > 0:
                    assert f.last_kernel_name() == (GENERIC if generic else TILED)
            st = f.state
            assert st.tap_dtype == (3 if np.dtype(th) == np.complex128 else 2)
            assert (st.phiIdx, st.inputDeficit) == state, (name, generic)
            hist = f.history.reshape(nch, -1)
            assert hist.dtype == np.dtype(tx)
            for c in range(nch):
                assert_bit_equal(hist[c], hists[c], f"{name} generic={generic} history {c}")
            f.close()


@pytest.mark.parametrize("shape,types", CASES, ids=lambda v: "-".join(np.dtype(t).name for t in v) if isinstance(v[0], type) else "x".join(map(str, v)))
def test_both_kernels_equal_the_restatement_per_channel(pkg, monkeypatch, shape, types):
    _run_case(pkg, monkeypatch, shape, *types)


@pytest.mark.parametrize("types", FEW_TYPES, ids=lambda v: "-".join(np.dtype(t).name for t in v))
def test_channel_c_equals_the_one_channel_complex_taps_filter_and_equal_rows_the_shared_one(pkg, monkeypatch, types):
    th, tx = types
    L, M, hLen, x_len = 3, 5, 11, 400
    H, x = _signal(51, hLen, x_len, th, tx)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    singles = []
    for c in range(NCH):
        one = pkg.FIRFilter.complex_taps(H[c], Fraction(L, M)).bind(tx, 1)
        singles.append((one.filt(np.array(x[c])), np.array(one.history)))
        one.close()
    same = np.ascontiguousarray(np.broadcast_to(H[0], (NCH, hLen)))
    shared = pkg.FIRFilter.complex_taps(H[0], Fraction(L, M)).bind(tx, NCH)
    y_shared, h_shared = shared.filt(np.array(x)), np.array(shared.history)
    shared.close()
    for generic in (True, False):
        f = _filter(pkg, monkeypatch, H, Fraction(L, M), tx, generic)
        y = f.filt(np.array(x))
        assert f.last_kernel_name() == (GENERIC if generic else TILED)
        hist = f.history
        for c in range(NCH):
            assert_bit_equal(y[c], singles[c][0].reshape(-1), f"channel {c} == complex_taps(H[{c}]), generic={generic}")
            assert_bit_equal(hist[c], singles[c][1].reshape(-1), f"history of channel {c}, generic={generic}")
        f.close()
        b = _filter(pkg, monkeypatch, same, Fraction(L, M), tx, generic)
        assert_bit_equal(b.filt(np.array(x)), y_shared, f"equal rows == the shared complex-taps filter, generic={generic}")
        assert b.last_kernel_name() == (GENERIC if generic else TILED)
        assert_bit_equal(b.history, h_shared, f"history, equal rows, generic={generic}")
        b.close()


def test_a_workgroup_that_crosses_channel_boundaries_reloads_its_bank(pkg, monkeypatch):
    """nch = 5 under MRHIP_BANK_CTAPS_GRID=2: each of the two workgroups walks tiles of at least two channels"""
    shape, nch = (3, 5, 11, 4000), 5
    L, M, hLen, x_len = shape
    th, tx = np.complex64, np.complex64
    _run_case(pkg, monkeypatch, shape, th, tx, nch=nch, grid=2, chunkings={"whole": None})
    H, x = _signal(1000 * L + M, hLen, x_len, th, tx, nch)
    capped = _filter(pkg, monkeypatch, H, Fraction(L, M), tx, generic=False, grid=2)
    y_capped = capped.filt(x)
    assert capped.last_kernel_name() == TILED
    free = _filter(pkg, monkeypatch, H, Fraction(L, M), tx, generic=False)
    y_free = free.filt(x)
    assert free.last_kernel_name() == TILED
    assert_bit_equal(y_capped, y_free, "two workgroups == the uncapped launch")
    capped.close(), free.close()


def _restated_stream(H, ratio, x, chunk, n):
    refs = [ComplexTapsRestated(H[c], ratio, tx=x.dtype) for c in range(H.shape[0])]
    out = [np.stack([r.filt(x[c, i * chunk:(i + 1) * chunk]) for c, r in enumerate(refs)]) for i in range(n)]
    return out, (refs[0].phiIdx, refs[0].inputDeficit), np.stack([r.history_array() for r in refs])


def test_async_calls_equal_the_restatements_chunk_loop(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 5, 11, 1000, 5
    H, x = _signal(21, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _restated_stream(H, Fraction(L, M), x, chunk, n)
    f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.complex64, generic=False)
    xd = torch.from_numpy(np.array(x)).cuda()
    bound = f.outputlength_bound(chunk)
    ys = torch.zeros((n, NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i in range(n):
        f.filt_into_async(ys[i], xd[:, i * chunk:(i + 1) * chunk], cnt[i:i + 1])
    last = f.sync_state()
    assert f.last_kernel_name() == GENERIC                     # the device-planned path: the universal bank-ctaps kernel
    counts = cnt.cpu().tolist()
    assert counts == [w.shape[1] for w in want] and last == counts[-1]
    for i in range(n):
        assert_bit_equal(ys[i, :, :counts[i]].cpu().numpy(), want[i], f"asynchronous call {i}")
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


def test_captured_call_replayed_three_times_equals_the_restatements_chunk_loop(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 5, 11, 1000, 4
    H, x = _signal(22, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _restated_stream(H, Fraction(L, M), x, chunk, n)
    f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.complex64, generic=False)
    xd = torch.from_numpy(np.array(x)).cuda()
    assert_bit_equal(f.filt(xd[:, :chunk].contiguous()).cpu().numpy(), want[0], "the plain call in front of the capture")
    assert f.last_kernel_name() == TILED
    bound = f.outputlength_bound(chunk)
    xs = torch.zeros((NCH, chunk), dtype=torch.complex64, device="cuda")
    ys = torch.zeros((NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        f.filt_into_async(ys, xs, cnt)
    for i in range(1, n):
        xs.copy_(xd[:, i * chunk:(i + 1) * chunk])
        g.replay()
        torch.cuda.synchronize()
        c = int(cnt.cpu()[0])
        assert c == want[i].shape[1]
        assert_bit_equal(ys[:, :c].cpu().numpy(), want[i], f"replay {i}")
    f.sync_state()
    assert f.last_kernel_name() == GENERIC                     # the captured call: the universal bank-ctaps kernel
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


def test_chunked_entry_equals_the_restatements_chunk_loop(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 5, 11, 96, 5
    H, x = _signal(23, hLen, chunk * n, np.complex64, np.float32)
    want, state, hist = _restated_stream(H, Fraction(L, M), x, chunk, n)
    whole = np.concatenate(want, axis=1)
    xd = torch.from_numpy(np.array(x)).cuda()
    # (mrhip_filt_device_chunked issues host-planned mrhip_filt_device calls -- for FIRRational one over the whole resident signal -- so
    # it is served by whichever kernel the host plan picks, not by the device-planned path)
    for generic in (True, False):
        f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic)
        yb = torch.zeros((NCH, whole.shape[1]), dtype=torch.complex64, device="cuda")
        assert f.filt_into_chunked(yb, xd, chunk) == whole.shape[1]
        assert f.last_kernel_name() == (GENERIC if generic else TILED)
        assert_bit_equal(yb.cpu().numpy(), whole, f"mrhip_filt_device_chunked, generic={generic}")
        st = f.state
        assert (st.phiIdx, st.inputDeficit) == state
        assert_bit_equal(f.history, hist, f"history after the chunked call, generic={generic}")
        f.close()


def test_ring_is_not_resident_and_equals_the_restatements_chunk_loop(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 5, 11, 96, 4
    H, x = _signal(31, hLen, chunk * n, np.complex64, np.complex64)
    want, state, _ = _restated_stream(H, Fraction(L, M), x, chunk, n)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.delenv("MRHIP_BANK_CTAPS_TILED", raising=False)
    f = pkg.FIRFilter.per_channel_complex_taps(H, Fraction(L, M)).bind(np.complex64, NCH)
    xd = torch.from_numpy(np.array(x)).cuda()
    total = sum(w.shape[1] for w in want)
    yb = torch.zeros((NCH, total), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    with f.open_ring() as ring:
        assert ring.info()["resident"] is False
        got, _ = ring.push_chunks(yb, xd, chunk)
        ring.drain()
    assert got == total
    assert f.last_kernel_name() == GENERIC                     # stream-ordered launches: the universal bank-ctaps kernel
    assert_bit_equal(yb.cpu().numpy(), np.concatenate(want, axis=1), "ring output")
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    f.close()


def test_filt_multi_with_a_plain_filter_beside_it_equals_the_single_calls(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, x_len = 3, 5, 11, 400
    H, x = _signal(41, hLen, x_len, np.complex64, np.float32)
    want, _, _ = _restated_stream(H, Fraction(L, M), x, x_len, 1)
    hr = np.ascontiguousarray(H[0].real)
    other = O.FIRFilter(hr, Fraction(L, M), tx=np.float32).filt(x[0])
    bank = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic=False)
    plain = pkg.FIRFilter(hr, Fraction(L, M))
    xd = torch.from_numpy(np.array(x)).cuda()
    ys = pkg.filt_multi([bank, plain], [xd, xd[0].contiguous()])
    assert_bit_equal(ys[0].cpu().numpy(), want[0], "the bank filter's stream")
    assert_bit_equal(ys[1].cpu().numpy(), other, "the other stream")
    assert bank.last_kernel_name() == TILED
    bank.reset(), plain.reset()
    ys = pkg.filt_multi([plain, bank], [xd[0].contiguous(), xd])   # (the plain filter leads: the eligibility loop meets the bank filter)
    assert_bit_equal(ys[1].cpu().numpy(), want[0], "the bank filter's stream, second")
    assert_bit_equal(ys[0].cpu().numpy(), other, "the other stream, first")
    assert bank.last_kernel_name() == TILED
    bank.close(), plain.close()


def test_taps_are_taps2pfb_per_channel_and_reset_set_state_set_history_continue_exactly(pkg, monkeypatch):
    L, M, hLen, x_len = 3, 5, 11, 400
    H, x = _signal(61, hLen, x_len, np.complex64, np.complex64)
    want, _, _ = _restated_stream(H, Fraction(L, M), x, x_len, 1)
    mid = [ComplexTapsRestated(H[c], Fraction(L, M), tx=np.complex64) for c in range(NCH)]
    head = np.stack([r.filt(x[c, :151]) for c, r in enumerate(mid)])
    for generic in (True, False):
        f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.complex64, generic)
        taps = f.taps()
        assert taps.shape == (NCH, f.tapsPerPhi, L) and taps.dtype == np.complex64
        for c in range(NCH):
            assert_bit_equal(taps[c], taps2pfb(H[c], L), f"taps of channel {c}")
        assert_bit_equal(f.filt(np.array(x)), want[0], "whole")
        f.reset()
        assert_bit_equal(f.filt(np.array(x)), want[0], "whole again after reset()")
        f.reset()
        f.set_state(mid[0].phiIdx, mid[0].inputDeficit)
        f.set_history(np.stack([r.history_array() for r in mid]))
        tail = f.filt(np.ascontiguousarray(x[:, 151:]))
        assert_bit_equal(np.concatenate([head, tail], axis=1), want[0], f"set_state + set_history, then the rest, generic={generic}")
        f.close()


def test_known_answer_running_sum_scaled_per_channel(pkg, monkeypatch):
    """H[k-1] = [(1+1im) k] * 3 for k = 1, 2, x = 1:12 on both channels, ratio 1//1: row k is k s (1+1im), s the running 3-sum"""
    x = np.arange(1, 13, dtype=np.float32)
    s = x + np.concatenate([[0], x[:-1]]) + np.concatenate([[0, 0], x[:-2]])
    H = np.stack([np.full(3, (1 + 1j) * k, dtype=np.complex64) for k in (1, 2)])
    for generic in (True, False):
        f = _filter(pkg, monkeypatch, H, 1, np.float32, generic)
        y = f.filt(np.stack([x, x]))
        assert y.dtype == np.complex64 and y.shape == (2, 12)
        for k in (1, 2):
            assert np.array_equal(y[k - 1], (k * s * (1 + 1j)).astype(np.complex64))
        f.close()


def test_contract_edges(pkg, monkeypatch):
    lib = pkg.load_library()
    F32, F64, C64 = 0, 1, 2
    H, _ = _signal(71, 8, 16, np.complex64, np.float32)
    f = pkg.FIRFilter.per_channel_complex_taps(H, Fraction(1, 2)).bind(np.float32, NCH)
    assert lib.mrhip_set_numerics(f._handle, 1) == 5            # FUSED: no fused form is defined
    assert lib.mrhip_set_numerics(f._handle, 0) == 0
    f.close()
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps(H, Fraction(1, 2)).bind(np.float32, NCH + 1)
    assert e.value.code == 1
    for th, hh in ((F32, np.ones((NCH, 8), np.float32)), (F64, np.ones((NCH, 8), np.float64))):
        out = C.c_void_p()
        assert lib.mrhip_create_rational_bank_ctaps(hh.ctypes.data_as(C.c_void_p), 8, th, 1, 2, F32, NCH, 0, C.byref(out)) == 1 and not out.value
    out = C.c_void_p()
    hc = np.array(H)
    assert lib.mrhip_create_rational_bank(hc.ctypes.data_as(C.c_void_p), 8, C64, 1, 2, F32, NCH, 0, C.byref(out)) == 5 and not out.value
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(hc, Fraction(1, 2))            # the real-tap constructor keeps refusing
    assert e.value.code == 5


def test_default_plan_takes_a_chip_filling_call_and_leaves_small_ones_to_the_universal_kernel(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen = 3, 5, 11
    H, x = _signal(81, hLen, 200_000, np.complex64, np.complex64)
    xd = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.delenv("MRHIP_BANK_CTAPS_GRID", raising=False)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "1")
    fg = pkg.FIRFilter.per_channel_complex_taps(H, Fraction(L, M)).bind(np.complex64, NCH)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.delenv("MRHIP_BANK_CTAPS_TILED", raising=False)
    ft = pkg.FIRFilter.per_channel_complex_taps(H, Fraction(L, M)).bind(np.complex64, NCH)
    # 3 x 120 000 outputs = 1407 tiles of 256: more than the chip has CUs -> the default plan takes the call
    y_t, y_g = ft.filt(xd), fg.filt(xd)
    assert ft.last_kernel_name() == TILED and fg.last_kernel_name() == GENERIC
    assert_bit_equal(y_t.cpu().numpy(), y_g.cpu().numpy(), "tiled == universal, chip-filling call")
    # 3 x 420 outputs: six tiles -> the default plan leaves the call to the universal kernel
    y_t, y_g = ft.filt(xd[:, :700].contiguous()), fg.filt(xd[:, :700].contiguous())
    assert ft.last_kernel_name() == GENERIC
    assert_bit_equal(y_t.cpu().numpy(), y_g.cpu().numpy(), "continuation on the universal kernel")
    monkeypatch.setenv("MRHIP_BANK_CTAPS_TILED", "0")              # switched off
    ft.filt(xd)
    assert ft.last_kernel_name() == GENERIC
    ft.close(), fg.close()


def test_an_oversized_bank_lands_on_the_universal_kernel(pkg, monkeypatch):
    """a bank of 13 000 pairs of Float32 (104 KB) does not fit the LDS plan even when the tiled kernel is forced"""
    rng = np.random.default_rng(12)
    hb = ((rng.standard_normal(13_000) + 1j * rng.standard_normal(13_000)) / 13_000).astype(np.complex64)
    xb = (rng.random((1, 300)) - 0.5).astype(np.float32)
    fb = _filter(pkg, monkeypatch, hb[None, :], 1, np.float32, generic=False)
    yb = fb.filt(xb)
    assert fb.last_kernel_name() == GENERIC and yb.shape == (1, 300)
    # (value check against NumPy's own complex dot: not bit-level, the restatement of 3.9e6 scalar products is too slow here; the bound is
    # the one tests/test_gpu_complex_taps.py uses for the same shape)
    ext = np.concatenate([np.zeros(12_999, np.float32), xb[0]])
    ref = np.array([np.dot(hb[::-1].astype(np.complex128), ext[k:k + 13_000]) for k in range(300)])
    assert np.max(np.abs(yb[0] - ref)) < 1e-4
    fb.close()
