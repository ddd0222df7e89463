"""The output-pair kernel's end slots under a lane mask (csrc/opair_kernel.inc, pair_device.h: masked_mac and its kin), bit for bit
against the oracle (needs one MI355X).

A lane's two windows start offA in {0, 1} and SMIN + dB, dB in {0, 1, 2}, samples into its run; dB is offA or offA + 1, so a lane is in
one of four classes (offA, dB) = (0, 0), (0, 1), (1, 1), (1, 2).  The slots in front of a window's start and past its end run with
EXEC narrowed to the lanes they belong to (tapsPerPhi >= 3; below that the selects remain).  The shapes here are small -- a few tiles, a
partial last tile, the history seam of a chunked run -- and chosen by class: ratios whose waves hold all four classes, and ratios whose
waves hold two, where two of the masks are all zero and their groups must do nothing (checked on the CPU by test_lane_classes).

Every case runs once as one call and once over ragged chunks with a 1-sample call among them; the second half of the module puts
+-0.0, +-Inf, NaN and denormals at seeded positions and uses all-zero and all-negative tap sets -- the values the -0.0 select existed
for: outputs equal the oracle's words where the oracle is not NaN, and are NaN exactly where it is."""
import zlib
from fractions import Fraction

import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

OPAIR = "rational_opair_kernel"
F32, F64, C64 = np.float32, np.float64, np.complex64
N = 20_000                                                  # samples per channel
NCH = 2

# (id, ratio, tapsPerPhi, tap type, sample type)
CASES = [
    ("147_160x24_f32", Fraction(147, 160), 24, F32, F32),
    ("160_147x24_f32", Fraction(160, 147), 24, F32, F32),
    ("4_1x32_c64", Fraction(4, 1), 32, F32, C64),
    ("3_2x1_f32", Fraction(3, 2), 1, F32, F32),
    ("3_2x2_f32", Fraction(3, 2), 2, F32, F32),
    ("3_2x3_f32", Fraction(3, 2), 3, F32, F32),
    ("3_2x4_f32", Fraction(3, 2), 4, F32, F32),
    ("3_17x8_f32_smin5", Fraction(3, 17), 8, F32, F32),
    ("7_16x8_f32_smin2", Fraction(7, 16), 8, F32, F32),
    ("147_160x24_f64", Fraction(147, 160), 24, F64, F64),
    ("147_160x24_f64xf32", Fraction(147, 160), 24, F64, F32),
]
# the special-value half: one case per arithmetic / sample layout / select-or-mask form
SPECIAL = [c for c in CASES if c[0] in ("147_160x24_f32", "4_1x32_c64", "3_2x2_f32", "3_2x3_f32", "3_17x8_f32_smin5", "147_160x24_f64xf32")]
CHUNKS = [N // 3 + 5, 1, 17, N - (N // 3 + 5) - 18]        # ragged, a 1-sample call among them


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def _signal(rng, tx, shape):
    if np.dtype(tx).kind == "c":
        return ((rng.random(shape) - 0.5) + 1j * (rng.random(shape) - 0.5)).astype(tx)
    return (rng.random(shape) - 0.5).astype(tx)


def _real(x):
    return x.view(F64 if x.dtype in (np.dtype(F64), np.dtype(np.complex128)) else F32)


def _taps(rng, ratio, T, th, kind="normal"):
    n = T * ratio.numerator - (ratio.numerator // 2 if T > 1 else 0)     # a ragged last row of the polyphase bank
    if kind == "zero":
        return np.zeros(n, dtype=th)
    h = rng.standard_normal(n).astype(th)
    h[h == 0.0] = 1.0
    return -np.abs(h) if kind == "negative" else h


def _specials(rng, x, per_kind):
    """+-0.0, +-Inf, NaN and denormals (the smallest, and the largest of either sign) at seeded positions of the real view, in place"""
    xr = _real(x)
    fi = np.finfo(xr.dtype)
    values = [0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny * (1 - fi.eps), -fi.tiny * (1 - fi.eps)]
    for row in xr:
        pos = rng.choice(row.size, size=per_kind * len(values), replace=False)
        for k, v in enumerate(values):
            row[pos[k * per_kind:(k + 1) * per_kind]] = v


def _cuts(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def _oracle_chunks(O, h, ratio, tx, x, sizes):
    cuts = _cuts(sizes)
    fos = [O.FIRFilter(h, ratio, tx=tx) for _ in x]
    return [[fo.filt(r[a:b]) for a, b in zip(cuts[:-1], cuts[1:])] for fo, r in zip(fos, x)], fos


def _assert_words(got, want, what):
    """the oracle's words where it is not NaN, NaN exactly where it is"""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    g, w = _real(np.ascontiguousarray(got)), _real(np.ascontiguousarray(want))
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"NaN positions: {what}"
    ok = ~np.isnan(w)
    assert_bit_equal(g[ok], w[ok], what)


def _run(pkg, O, torch, case, h, x, sizes, numerics, what):
    _, ratio, T, th, tx = case
    ref, fos = _oracle_chunks(O, h, ratio, tx, x, sizes)
    xd = torch.from_numpy(x).cuda()
    cuts = _cuts(sizes)
    f = pkg.FIRFilter(h, ratio, numerics=numerics)
    try:
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            y = f.filt(xd[:, a:b].contiguous())
            if y.shape[-1] > 0:
                assert f.last_kernel_name() == OPAIR, (what, f.last_kernel_name())
            _assert_words(y.cpu().numpy(), np.stack([r[i] for r in ref]), f"{what}: chunk {i} of {sizes}")
        st, so = f.state, fos[0].state
        assert (st.phiIdx, st.inputDeficit) == (so.phiIdx, so.inputDeficit), what
    finally:
        f.close()
    return ref


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _classes(L, M, u0, lanes):
    """(offA, dB) of the lanes of a workgroup whose first output has phase numerator u0 (opair_kernel.inc, the lane's two outputs)"""
    out = []
    for t in range(lanes):
        qa, qb = (u0 + 2 * t * M) // L, (u0 + (2 * t + 1) * M) // L
        out.append((qa - (qa & ~1), qb - (qa & ~1) - M // L))
    return out


def test_lane_classes():
    """the premise of the table: 147//160 and 160//147 put all four classes into one wave (every mask has lanes in and lanes out), 4//1
    only two, (0, 0) and (1, 1) (no lane has dB = 2: the mask of B's slot T + 1 is all zero, that of B's slot 1 all ones), and a small
    call of 3//2 ends in a wave of one lane (129 lanes: every mask is all ones or all zero there)."""
    four = {(0, 0), (0, 1), (1, 1), (1, 2)}
    for L, M in ((147, 160), (160, 147)):
        for u0 in range(L):
            assert set(_classes(L, M, u0, 64)) == four, (L, M, u0)
    for u0 in (0, 2):                                       # (an interpolator's calls start at an even phase numerator: every input gives L outputs)
        assert set(_classes(4, 1, u0, 128)) == {(0, 0), (1, 1)}, u0
    assert all(len(set(_classes(3, 2, u0, 129)[128:])) == 1 for u0 in range(3))
    for L, M in ((3, 17), (7, 16)):
        assert set().union(*(set(_classes(L, M, u0, 128)) for u0 in range(L))) == four, (L, M)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_offset_classes(pkg, O, torch_cuda, case):
    """one call, and the same input in ragged chunks: several tiles, a partial last tile, the history seam"""
    name, ratio, T, th, tx = case
    rng = _rng("classes", name)
    h = _taps(rng, ratio, T, th)
    assert -(-len(h) // ratio.numerator) == T
    x = _signal(rng, tx, (NCH, N))
    whole = _run(pkg, O, torch_cuda, case, h, x, [N], pkg.NUMERICS_STRICT, f"{name}: one call")
    parts = _run(pkg, O, torch_cuda, case, h, x, CHUNKS, pkg.NUMERICS_STRICT, f"{name}: chunks")
    for w, p in zip(whole, parts):                          # (the oracle itself: chunking does not change a word)
        assert_bit_equal(np.concatenate(p), w[0], f"{name}: the oracle, chunked")


@pytest.mark.parametrize("taps", ["normal", "zero", "negative"])
@pytest.mark.parametrize("case", SPECIAL, ids=[c[0] for c in SPECIAL])
def test_special_values(pkg, O, torch_cuda, case, taps):
    """+-0.0, +-Inf, NaN, denormals among the samples; all-zero and all-negative taps: the sign of a zero sum, 0 * Inf = NaN, Inf - Inf"""
    name, ratio, T, th, tx = case
    rng = _rng("special", name, taps)
    h = _taps(rng, ratio, T, th, taps)
    x = _signal(rng, tx, (NCH, N))
    _specials(rng, x, per_kind=4)                            # 12 non-finite values per row: each reaches the outputs of one window length
    whole, _ = _oracle_chunks(O, h, ratio, tx, x, [N])
    nan = np.mean([np.isnan(_real(w[0])).mean() for w in whole])
    assert 0.0 < nan <= 0.5, f"{name}: {nan:.3f} of the oracle's output is NaN"      # (a propagating NaN would hide everything else)
    _run(pkg, O, torch_cuda, case, h, x, [N], pkg.NUMERICS_STRICT, f"{name} {taps} taps: one call")
    _run(pkg, O, torch_cuda, case, h, x, CHUNKS, pkg.NUMERICS_STRICT, f"{name} {taps} taps: chunks")


def test_fused(pkg, O, torch_cuda):
    """FUSED (one fma per tap; the tails are masked fmas, the heads keep their selects) against the oracle's fused switch"""
    case = CASES[0]
    name, ratio, T, th, tx = case
    rng = _rng("fused", name)
    h = _taps(rng, ratio, T, th)
    x = _signal(rng, tx, (NCH, N))
    _specials(rng, x, per_kind=2)
    O.set_fused(True)
    try:
        _run(pkg, O, torch_cuda, case, h, x, [N], pkg.NUMERICS_FUSED, f"{name} fused: one call")
        _run(pkg, O, torch_cuda, case, h, x, CHUNKS, pkg.NUMERICS_FUSED, f"{name} fused: chunks")
    finally:
        O.set_fused(False)


def test_ring(pkg, O, torch_cuda):
    """the resident ring's consumer (MODE 2): open, three pushes of unequal length -- none a multiple of M = 160, so each chunk starts at
    another phase u0 and the lanes' classes and masks move with it --, close"""
    torch = torch_cuda
    name, ratio, T, th, tx = CASES[0]
    rng = _rng("ring", name)
    h = _taps(rng, ratio, T, th)
    rows, reps, n = 4, 16, 24_000
    x = _signal(rng, tx, (rows, n))
    _specials(rng, x, per_kind=2)
    sizes = [n // 3 + 7, T - 2, n - (n // 3 + 7) - (T - 2)]
    assert all(s % ratio.denominator for s in sizes)
    ref, fos = _oracle_chunks(O, h, ratio, tx, x, sizes)
    xd = torch.from_numpy(np.tile(x, (reps, 1))).cuda()
    cuts = _cuts(sizes)
    f = pkg.FIRFilter(h, ratio).bind(tx, rows * reps)
    try:
        ys = [torch.zeros((rows * reps, max(f.outputlength_bound(s), 1)), dtype=torch.float32, device="cuda") for s in sizes]
        torch.cuda.synchronize()
        with f.open_ring() as ring:
            assert ring.info()["resident"]
            counts = [ring.push(y, xd[:, a:b])[0] for y, a, b in zip(ys, cuts[:-1], cuts[1:])]
            ring.drain()
        assert counts == [len(r) for r in ref[0]], counts
        for i, (y, k) in enumerate(zip(ys, counts)):
            _assert_words(y[:, :k].cpu().numpy(), np.tile(np.stack([r[i] for r in ref]), (reps, 1)), f"ring: chunk {i}")
        st, so = f.state, fos[0].state
        assert (st.phiIdx, st.inputDeficit) == (so.phiIdx, so.inputDeficit)
    finally:
        f.close()
