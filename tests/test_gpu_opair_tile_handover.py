"""The tile hand-over of the loader-wave kernels, bit for bit against the oracle (needs one MI355X).

The loader wave publishes a tile's descriptor by an LDS write and the compute waves fetch it by an LDS read behind the tile barrier
(csrc/pair_device.h: desc_put / desc_get); the output-pair kernel keeps its lane constants in registers across tiles, walks a tile's
steps with one window address and a store base that advances on the scalar side, and stores under lane masks found once per tile
(csrc/opair_kernel.inc); the loader's interior tiles go by a lane-constant offset on a scalar base (csrc/pair_loader.h).  None of it
may move a bit: outputs, carried history and end state equal the oracle's for

  * the headline instantiation (MODE 1: 147//160, 24 x 147 taps, Float32, 64 channels x 72 000 samples = 12.5 tiles a channel, so the
    last tile takes the path of a tile that ends inside a step),
  * the small-call instantiation (MODE 3) at whole tiles, one sample more or fewer, one step, less than a step, one sample,
  * both again with a hand-over at every step (MRHIP_OPAIR_J=1), three pipeline stages (MRHIP_OPAIR_NS=3) and the tap columns gathered
    from global memory (MRHIP_OPAIR_BANK=0),
  * a stream continued over three calls (another u0, the history seam), a y whose rows are further apart than they are long,
  * and one case through every other user of the hand-over: ComplexF32, Float64 (three stages by the plan), fir_stream_kernel,
    fir_stream_rt_kernel and the resident ring's consumer."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

OPAIR = "rational_opair_kernel"
RATIO = Fraction(147, 160)
KNOBS = {"default": {}, "J1": {"MRHIP_OPAIR_J": "1"}, "NS3": {"MRHIP_OPAIR_NS": "3"}, "BANK0": {"MRHIP_OPAIR_BANK": "0"}}
SMALL_LENS = [5760 * k + d for k in (1, 2) for d in (0, 1, -1)] + [959, 960, 961, 1]
ROWS, REPS, N_BIG = 4, 16, 72_000                                   # 64 channels: four distinct rows, sixteen times


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def taps(pkg):
    return pkg.firdes(24 * 147, 0.5 / 147, beta=7.8562).astype(np.float32)       # the benchmark's filter


@pytest.fixture(scope="module")
def signals():
    rng = np.random.default_rng(1414)
    return {"big": (rng.random((ROWS, N_BIG), dtype=np.float32) - 0.5), "small": (rng.random((3, max(SMALL_LENS)), dtype=np.float32) - 0.5)}


@pytest.fixture(scope="module")
def reference(O, taps, signals):
    """the oracle's one-call result for a prefix of the rows of a signal: (outputs per row, histories, end state), computed once"""
    cache = {}

    def get(which, nrows, n):
        key = (which, nrows, n)
        if key not in cache:
            fs = [O.FIRFilter(taps, RATIO, tx=np.float32) for _ in range(nrows)]
            ys = [f.filt(signals[which][c, :n]) for c, f in enumerate(fs)]
            cache[key] = (np.stack(ys), np.stack([f.history for f in fs]), (fs[0].state.phiIdx, fs[0].state.inputDeficit))
        return cache[key]
    return get


def _set(monkeypatch, knobs):
    for k in ("MRHIP_OPAIR_J", "MRHIP_OPAIR_NS", "MRHIP_OPAIR_BANK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _check_end(f, hist, state, reps, what):
    st = f.state
    assert (st.phiIdx, st.inputDeficit) == state, what
    assert_bit_equal(np.asarray(f.history).reshape(hist.shape[0] * reps, -1), np.tile(hist, (reps, 1)), f"history: {what}")


@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
def test_headline_instantiation(pkg, torch_cuda, taps, signals, reference, monkeypatch, knobs):
    """64 channels x 72 000 samples: 66 150 outputs a channel are 12.5 tiles of 6 steps of 882 -- whole tiles and one that ends inside a step"""
    _set(monkeypatch, KNOBS[knobs])
    want, hist, state = reference("big", ROWS, N_BIG)
    assert want.shape[1] == 66_150 and want.shape[1] * ROWS * REPS >= 1 << 22
    xd = torch_cuda.from_numpy(np.tile(signals["big"], (REPS, 1))).cuda()
    f = pkg.FIRFilter(taps, RATIO)
    try:
        y = f.filt(xd)
        assert f.last_kernel_name() == OPAIR, f.last_kernel_name()
        assert_bit_equal(y.cpu().numpy(), np.tile(want, (REPS, 1)), f"headline, {knobs}")
        _check_end(f, hist, state, REPS, f"headline, {knobs}")
    finally:
        f.close()


@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
@pytest.mark.parametrize("nch", [3, 1])
def test_small_call_geometry(pkg, torch_cuda, taps, signals, reference, monkeypatch, knobs, nch):
    """MODE 3: whole tiles, one output more or fewer, one step, less than a step, a single sample"""
    _set(monkeypatch, KNOBS[knobs])
    xd = torch_cuda.from_numpy(signals["small"][:nch]).cuda()
    for n in SMALL_LENS:
        want, hist, state = reference("small", nch, n)
        f = pkg.FIRFilter(taps, RATIO)
        try:
            y = f.filt(xd[:, :n].contiguous())
            if want.shape[1] > 0:
                assert f.last_kernel_name() == OPAIR, (n, f.last_kernel_name())
            assert_bit_equal(y.cpu().numpy().reshape(nch, -1), want, f"{nch} ch x {n}, {knobs}")
            _check_end(f, hist, state, 1, f"{nch} ch x {n}, {knobs}")
        finally:
            f.close()


def test_continuing_stream(pkg, O, torch_cuda, taps):
    """three calls of 50 001, 1 and 49 999 samples on one filter: the second and third start at another u0, across the history seam"""
    nch, sizes = 2, [50_001, 1, 49_999]
    n = sum(sizes)
    rng = np.random.default_rng(1415)
    x = rng.random((nch, n), dtype=np.float32) - 0.5
    xd = torch_cuda.from_numpy(x).cuda()
    one, parts = pkg.FIRFilter(taps, RATIO), pkg.FIRFilter(taps, RATIO)
    try:
        whole = one.filt(xd).cpu().numpy()
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        got = np.concatenate([parts.filt(xd[:, a:b].contiguous()).cpu().numpy().reshape(nch, -1) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        assert_bit_equal(got, whole, "three calls against one")
        assert (parts.state.phiIdx, parts.state.inputDeficit) == (one.state.phiIdx, one.state.inputDeficit)
        assert_bit_equal(np.asarray(parts.history), np.asarray(one.history), "history: three calls against one")
    finally:
        one.close(); parts.close()
    for c in range(nch):
        fo = O.FIRFilter(taps, RATIO, tx=np.float32)
        assert_bit_equal(whole[c], fo.filt(x[c]), f"one call against the oracle, channel {c}")


@pytest.mark.parametrize("shape", ["headline", "small"])
def test_row_stride_larger_than_the_outputs(pkg, torch_cuda, taps, signals, reference, shape):
    """rows of y further apart than they are long: nothing between them, nor behind the last, is touched"""
    torch = torch_cuda
    which, rows, reps, n = ("big", ROWS, REPS, N_BIG) if shape == "headline" else ("small", 3, 1, 5761)
    want, _, _ = reference(which, rows, n)
    cnt, gap = want.shape[1], 37
    xd = torch.from_numpy(np.tile(signals[which][:rows, :n], (reps, 1))).cuda()
    sentinel = np.float32(-7.25)
    buf = torch.full((rows * reps, cnt + gap), float(sentinel), dtype=torch.float32, device="cuda")
    f = pkg.FIRFilter(taps, RATIO)
    try:
        assert f.filt_into(buf[:, :cnt], xd) == cnt
        assert f.last_kernel_name() == OPAIR
    finally:
        f.close()
    got = buf.cpu().numpy()
    assert_bit_equal(got[:, :cnt], np.tile(want, (reps, 1)), f"{shape}: outputs in a strided y")
    assert_bit_equal(got[:, cnt:], np.full((rows * reps, gap), sentinel), f"{shape}: the gaps of a strided y")


def _rand(rng, shape, tx):
    x = rng.random(shape) - 0.5
    if np.dtype(tx).kind == "c":
        x = x + 1j * (rng.random(shape) - 0.5)
    return x.astype(tx)


OTHERS = [
    # (id, ratio, taps, tap type, sample type, kernel)
    ("c64", RATIO, 24 * 147, np.float32, np.complex64, OPAIR),
    ("f64_three_stages", RATIO, 24 * 147, np.float64, np.float64, OPAIR),
    ("decimate_4", Fraction(1, 4), 128, np.float32, np.float32, "fir_stream_kernel"),
    ("decimate_32", Fraction(1, 32), 128, np.float32, np.float32, "fir_stream_rt_kernel"),
]


@pytest.mark.parametrize("case", OTHERS, ids=[c[0] for c in OTHERS])
def test_other_users_of_the_hand_over(pkg, O, torch_cuda, case):
    name, ratio, ntaps, th, tx, kernel = case
    rng = np.random.default_rng(1416)
    L = ratio.numerator
    h = (pkg.firdes(ntaps, 0.45 / max(L, ratio.denominator), beta=7.0) * L).astype(th)
    nch, sizes = 2, [20_003, 1, 9_997]
    x = _rand(rng, (nch, sum(sizes)), tx)
    xd = torch_cuda.from_numpy(x).cuda()
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    f = pkg.FIRFilter(h, ratio)
    fos = [O.FIRFilter(h, ratio, tx=tx) for _ in range(nch)]
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            y = f.filt(xd[:, a:b].contiguous()).cpu().numpy().reshape(nch, -1)
            if b - a > 1:
                assert f.last_kernel_name() == kernel, (name, f.last_kernel_name())
            for c in range(nch):
                assert_bit_equal(y[c], fos[c].filt(x[c, a:b]), f"{name}: samples {a}..{b}, channel {c}")
        assert (f.state.phiIdx, f.state.inputDeficit) == (fos[0].state.phiIdx, fos[0].state.inputDeficit)
        for c in range(nch):
            assert_bit_equal(np.asarray(f.history).reshape(nch, -1)[c], fos[c].history, f"{name}: history of channel {c}")
    finally:
        f.close()


def test_ring_of_twenty_chunks(pkg, O, torch_cuda, taps, monkeypatch):
    """the resident ring's consumer takes sixteen-word descriptors the same way: 20 chunks of 10 007 samples (every chunk another u0)"""
    torch = torch_cuda
    monkeypatch.setenv("MRHIP_RING_IDLE_MS", "500")
    nch, nchunks, n = 2, 20, 10_007
    rng = np.random.default_rng(1417)
    x = rng.random((nch, nchunks * n), dtype=np.float32) - 0.5
    fos = [O.FIRFilter(taps, RATIO, tx=np.float32) for _ in range(nch)]
    ref = [[fo.filt(x[c, i * n:(i + 1) * n]) for i in range(nchunks)] for c, fo in enumerate(fos)]
    xd = torch.from_numpy(x).cuda()
    f = pkg.FIRFilter(taps, RATIO).bind(np.float32, nch)
    try:
        ys = torch.zeros((nchunks, nch, f.outputlength_bound(n)), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with f.open_ring() as ring:
            assert ring.info()["resident"]
            counts = [ring.push(ys[i], xd[:, i * n:(i + 1) * n])[0] for i in range(nchunks)]
            ring.drain()
        got = ys.cpu().numpy()
        for i in range(nchunks):
            for c in range(nch):
                assert counts[i] == len(ref[c][i])
                assert_bit_equal(got[i, c, :counts[i]], ref[c][i], f"ring: chunk {i}, channel {c}")
        assert (f.state.phiIdx, f.state.inputDeficit) == (fos[0].state.phiIdx, fos[0].state.inputDeficit)
        for c in range(nch):
            assert_bit_equal(np.asarray(f.history).reshape(nch, -1)[c], fos[c].history, f"ring: history of channel {c}")
    finally:
        f.close()
