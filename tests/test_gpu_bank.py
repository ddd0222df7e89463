"""GPU tests of the per-channel-taps kernels (csrc/kernels_bank.hip): FIRFilter.per_channel(H, ratio), one FIRFilter(H[c], ratio) per
channel behind one filter object.

Bar (include/multirate_hip.h, "Per-channel taps"): for every channel c the outputs, the per-call counts, the end state and the history are
BIT FOR BIT those of the oracle's FIRFilter(H[c], ratio) fed x[c] -- on poly_bank_generic_kernel (MRHIP_FORCE_GENERIC=1) and on
poly_bank_tiled_kernel (MRHIP_BANK_TILED=1), whole and chunked (a one-sample chunk, an empty one, chunks shorter than the history), STRICT
and FUSED, host- and device-planned.  No tolerance anywhere.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NCH = 3
# (L, M, hLen, x_len): FIRStandard, FIRDecimator, FIRInterpolator with hLen no multiple of L (padded zeros), two FIRRational, the headline ratio
SHAPES = [(1, 1, 5, 300), (1, 3, 7, 300), (3, 1, 10, 300), (3, 5, 11, 400), (7, 4, 30, 400), (147, 160, 147 * 3 + 5, 2000)]
ALL_TYPES = [(th, tx) for th in (np.float32, np.float64) for tx in (np.float32, np.float64, np.complex64, np.complex128)]
FEW_TYPES = [(np.float32, np.float32), (np.float32, np.complex64)]
CASES = [((3, 5, 11, 400), t) for t in ALL_TYPES] + [(s, t) for s in SHAPES if s[:2] != (3, 5) for t in FEW_TYPES]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
GENERIC, TILED = "poly_bank_generic_kernel", "poly_bank_tiled_kernel"


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


@functools.lru_cache(maxsize=None)
def _signal(seed, hLen, x_len, th, tx, nch=NCH):
    """rows that tell channels apart: row 0 random, row 1 a single 1 at tap 0 (the channel's output is its own input passed through the
    polyphase schedule), row 2 = row 0 reversed and negated; further rows random"""
    rng = np.random.default_rng(seed)
    H = (rng.standard_normal((nch, hLen)) / hLen).astype(th)
    if nch > 1:
        H[1] = 0
        H[1, 0] = 1
    if nch > 2:
        H[2] = -H[0][::-1]
    x = rng.random((nch, x_len)) - 0.5
    if np.dtype(tx).kind == "c":
        x = x + 1j * (rng.random((nch, x_len)) - 0.5)
    x = x.astype(tx)
    H.setflags(write=False), x.setflags(write=False)
    return H, x


_REFS = {}


def _reference(O, seed, L, M, hLen, x_len, th, tx, how, nch=NCH, fused=False):
    """the oracle per channel, one O.FIRFilter(H[c], ratio) fed x[c] in the pieces of `how`: (outputs [c][piece], (phiIdx, inputDeficit),
    histories [c]); computed once per case and shared"""
    key = (seed, L, M, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), nch, fused)
    if key not in _REFS:
        H, x = _signal(seed, hLen, x_len, th, tx, nch)
        O.set_fused(fused)
        try:
            refs = [O.FIRFilter(H[c], Fraction(L, M), tx=tx) for c in range(nch)]
            outs = [[r.filt(x[c, a:b]) for a, b in _chunks(x_len, how)] for c, r in enumerate(refs)]
        finally:
            O.set_fused(False)
        states = {(r.state.phiIdx, r.state.inputDeficit) for r in refs}
        assert len(states) == 1                                   # (the state does not depend on the taps)
        _REFS[key] = (outs, states.pop(), [r.history for r in refs])
    return _REFS[key]


def _filter(pkg, monkeypatch, H, ratio, tx, generic, fused=False, grid=None):
    """a bound bank filter on the universal kernel (MRHIP_FORCE_GENERIC is read when the device object is created) or with the tiled
    kernel wherever its LDS plan fits (MRHIP_BANK_TILED=1)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "1" if generic else "0")
    monkeypatch.setenv("MRHIP_BANK_TILED", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_BANK_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_BANK_GRID", str(grid))
    return pkg.FIRFilter.per_channel(H, ratio, numerics=pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT).bind(tx, H.shape[0])


def _run_case(pkg, O, monkeypatch, shape, th, tx, fused=False, nch=NCH, grid=None, chunkings=CHUNKINGS):
    L, M, hLen, x_len = shape
    seed = 1000 * L + M
    H, x = _signal(seed, hLen, x_len, th, tx, nch)
    want_dtype = np.dtype(O.FIRFilter(H[0], Fraction(L, M), tx=tx).ty)
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        want, state, hists = _reference(O, seed, L, M, hLen, x_len, th, tx, how, nch, fused)
        for generic in (True, False):
            f = _filter(pkg, monkeypatch, H, Fraction(L, M), tx, generic, fused, grid)
            assert f.output_dtype == want_dtype
            for i, (a, b) in enumerate(pieces):
                y = f.filt(np.ascontiguousarray(x[:, a:b]))
                assert y.dtype == want_dtype and y.shape == (nch, len(want[0][i])), (name, generic, a, b, y.shape)   # the per-call count
                for c in range(nch):
                    assert_bit_equal(y[c], want[c][i], f"{name} generic={generic} chunk [{a}, {b}) channel {c}")
                if y.shape[1] > 0:
                    assert f.last_kernel_name() == (GENERIC if generic else TILED)
            st = f.state
            assert (st.phiIdx, st.inputDeficit) == state, (name, generic)
            hist = f.history.reshape(nch, -1)
            assert hist.dtype == np.dtype(tx)
            for c in range(nch):
                assert_bit_equal(hist[c], hists[c], f"{name} generic={generic} history {c}")
            f.close()


@pytest.mark.parametrize("shape,types", CASES, ids=lambda v: "-".join(np.dtype(t).name for t in v) if isinstance(v[0], type) else "x".join(map(str, v)))
def test_both_kernels_equal_the_oracle_per_channel(pkg, O, monkeypatch, shape, types):
    _run_case(pkg, O, monkeypatch, shape, *types)


@pytest.mark.parametrize("shape", [(1, 3, 7, 300), (3, 5, 11, 400)], ids=lambda s: "x".join(map(str, s)))
def test_fused_equals_the_fused_oracle(pkg, O, monkeypatch, shape):
    _run_case(pkg, O, monkeypatch, shape, np.float32, np.float32, fused=True)


def test_a_workgroup_that_crosses_channel_boundaries_reloads_its_bank(pkg, O, monkeypatch):
    """nch = 5 under MRHIP_BANK_GRID=2: each of the two workgroups walks tiles of at least two channels"""
    shape, nch = (3, 5, 11, 4000), 5
    L, M, hLen, x_len = shape
    _run_case(pkg, O, monkeypatch, shape, np.float32, np.float32, nch=nch, grid=2, chunkings={"whole": None})
    H, x = _signal(1000 * L + M, hLen, x_len, np.float32, np.float32, nch)
    capped = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic=False, grid=2)
    y_capped = capped.filt(x)
    assert capped.last_kernel_name() == TILED
    free = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic=False)
    y_free = free.filt(x)
    assert free.last_kernel_name() == TILED
    assert_bit_equal(y_capped, y_free, "two workgroups == the uncapped launch")
    capped.close(), free.close()


def _oracle_stream(O, H, ratio, x, chunk, n):
    refs = [O.FIRFilter(H[c], ratio, tx=x.dtype) for c in range(H.shape[0])]
    out = [np.stack([r.filt(x[c, i * chunk:(i + 1) * chunk]) for c, r in enumerate(refs)]) for i in range(n)]
    return out, (refs[0].state.phiIdx, refs[0].state.inputDeficit), np.stack([r.history for r in refs])


def test_async_calls_equal_the_oracles_chunk_loop(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 5, 11, 1000, 5
    H, x = _signal(21, hLen, chunk * n, np.float32, np.float32)
    want, state, hist = _oracle_stream(O, H, Fraction(L, M), x, chunk, n)
    f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic=False)
    xd = torch.from_numpy(np.array(x)).cuda()
    bound = f.outputlength_bound(chunk)
    ys = torch.zeros((n, NCH, bound), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i in range(n):
        f.filt_into_async(ys[i], xd[:, i * chunk:(i + 1) * chunk], cnt[i:i + 1])
    last = f.sync_state()
    assert f.last_kernel_name() == GENERIC                     # the device-planned path: the universal bank kernel
    counts = cnt.cpu().tolist()
    assert counts == [w.shape[1] for w in want] and last == counts[-1]
    for i in range(n):
        assert_bit_equal(ys[i, :, :counts[i]].cpu().numpy(), want[i], f"asynchronous call {i}")
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


def test_captured_call_replayed_three_times_equals_the_oracles_chunk_loop(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 5, 11, 1000, 4
    H, x = _signal(22, hLen, chunk * n, np.float32, np.float32)
    want, state, hist = _oracle_stream(O, H, Fraction(L, M), x, chunk, n)
    f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic=False)
    xd = torch.from_numpy(np.array(x)).cuda()
    assert_bit_equal(f.filt(xd[:, :chunk].contiguous()).cpu().numpy(), want[0], "the plain call in front of the capture")
    bound = f.outputlength_bound(chunk)
    xs = torch.zeros((NCH, chunk), dtype=torch.float32, device="cuda")
    ys = torch.zeros((NCH, bound), dtype=torch.float32, device="cuda")
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
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


def test_ring_is_not_resident_and_equals_the_plain_stream(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, chunk, n = 3, 5, 11, 96, 4
    H, x = _signal(31, hLen, chunk * n, np.float32, np.float32)
    want, state, _ = _oracle_stream(O, H, Fraction(L, M), x, chunk, n)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.delenv("MRHIP_BANK_TILED", raising=False)
    f = pkg.FIRFilter.per_channel(H, Fraction(L, M)).bind(np.float32, NCH)
    xd = torch.from_numpy(np.array(x)).cuda()
    total = sum(w.shape[1] for w in want)
    yb = torch.zeros((NCH, total), dtype=torch.float32, device="cuda")
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


def test_filt_multi_with_a_bank_filter_equals_the_single_calls(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    L, M, hLen, x_len = 3, 5, 11, 400
    H, x = _signal(41, hLen, x_len, np.float32, np.float32)
    want, _, _ = _oracle_stream(O, H, Fraction(L, M), x, x_len, 1)
    other = O.FIRFilter(H[0], Fraction(L, M), tx=np.float32).filt(x[0])
    bank = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic=False)
    plain = pkg.FIRFilter(H[0], Fraction(L, M))
    xd = torch.from_numpy(np.array(x)).cuda()
    ys = pkg.filt_multi([bank, plain], [xd, xd[0].contiguous()])
    assert_bit_equal(ys[0].cpu().numpy(), want[0], "the bank filter's stream")
    assert_bit_equal(ys[1].cpu().numpy(), other, "the other stream")
    assert bank.last_kernel_name() == TILED
    bank.close(), plain.close()


def test_taps_are_taps2pfb_per_channel_and_equal_rows_equal_the_shared_taps_filter(pkg, O, monkeypatch):
    L, M, hLen, x_len = 3, 5, 11, 400
    H, x = _signal(51, hLen, x_len, np.float32, np.float32)
    f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic=False)
    taps = f.taps()
    assert taps.shape == (NCH, f.tapsPerPhi, L)
    for c in range(NCH):
        assert_bit_equal(taps[c], O.taps2pfb(H[c], L), f"taps of channel {c}")
    f.close()
    same = np.ascontiguousarray(np.broadcast_to(H[0], (NCH, hLen)))
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    shared = pkg.FIRFilter(H[0], Fraction(L, M))
    want = shared.filt(np.array(x))
    for generic in (True, False):
        b = _filter(pkg, monkeypatch, same, Fraction(L, M), np.float32, generic)
        assert_bit_equal(b.filt(np.array(x)), want, f"equal rows == the shared-taps filter, generic={generic}")
        assert_bit_equal(b.history, shared.history, "history")
        b.close()
    shared.close()


def test_reset_then_set_state_and_set_history_in_mid_stream_continue_exactly(pkg, O, monkeypatch):
    L, M, hLen, x_len = 3, 5, 11, 400
    H, x = _signal(61, hLen, x_len, np.float32, np.float32)
    want, _, _ = _oracle_stream(O, H, Fraction(L, M), x, x_len, 1)
    mid = [O.FIRFilter(H[c], Fraction(L, M), tx=np.float32) for c in range(NCH)]
    head = np.stack([r.filt(x[c, :151]) for c, r in enumerate(mid)])
    for generic in (True, False):
        f = _filter(pkg, monkeypatch, H, Fraction(L, M), np.float32, generic)
        assert_bit_equal(f.filt(np.array(x)), want[0], "whole")
        f.reset()
        assert_bit_equal(f.filt(np.array(x)), want[0], "whole again after reset()")
        f.reset()
        f.set_state(mid[0].state.phiIdx, mid[0].state.inputDeficit)
        f.set_history(np.stack([r.history for r in mid]))
        tail = f.filt(np.ascontiguousarray(x[:, 151:]))
        assert_bit_equal(np.concatenate([head, tail], axis=1), want[0], f"set_state + set_history, then the rest, generic={generic}")
        f.close()
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(H, Fraction(L, M)).bind(np.float32, NCH + 1)
    assert e.value.code == 1
