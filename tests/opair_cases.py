"""Case generation for test_gpu_opair_instantiations.py (no tests here): the table of rational_opair_kernel instantiations the
dispatcher can reach, the ratio / tap-count rotation, the two signal shapes with their edge patches, and a restatement of the
part of plan_rational_opair (csrc/kernels_rational_opair.hip) that fixes a call's tiling -- c, P = c*L outputs per step, J steps
per tile -- which sizes the shapes.  The restatement is checked against what the library prints (MRHIP_DEBUG=1) by the guard test."""
from fractions import Fraction

import numpy as np

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128

# (name, tap dtype, sample dtype, largest tapsPerPhi for SMIN <= 1, SMIN values that exist)
TYPES = [
    ("f32xf32", F32, F32, 64, (0, 1, 2, 3, 4, 5)),
    ("f32xc64", F32, C64, 64, (0, 1, 2, 3, 4, 5)),
    ("f64xf64", F64, F64, 48, (0, 1)),
    ("f64xf32", F64, F32, 48, (0, 1)),
    ("f64xc64", F64, C64, 32, (0, 1)),
    ("f64xc128", F64, C128, 32, (0, 1)),
]
TYPE_INDEX = {t[0]: i for i, t in enumerate(TYPES)}

# window distance SMIN = floor(M/L): a small even L, a small odd L, L >= 100 (L = 511 is left out: Float64 arithmetic with more
# than 32 taps per phase is planned for at most seven compute waves)
RATIOS = {
    0: [Fraction(2, 1), Fraction(3, 2), Fraction(7, 3), Fraction(160, 147)],
    1: [Fraction(2, 3), Fraction(5, 9), Fraction(147, 160)],
    2: [Fraction(2, 5), Fraction(3, 8), Fraction(160, 441)],
    3: [Fraction(3, 10), Fraction(2, 7), Fraction(101, 350)],
    4: [Fraction(2, 9), Fraction(3, 13), Fraction(101, 450)],
    5: [Fraction(2, 11), Fraction(3, 17), Fraction(101, 600)],
}

MANY_CHANNELS, MANY_ROWS = 64, 4
SHORT_CHANNELS = 3
NUM_CUS = 256                                   # MI355X


def strict_params():
    """[(type name, SMIN)]: 2 * 6 + 4 * 2 = 20"""
    return [(t[0], s) for t in TYPES for s in t[4]]


def strict_taps(tname, smin):
    """every tapsPerPhi the dispatcher can reach for (type, SMIN), STRICT"""
    tmax = TYPES[TYPE_INDEX[tname]][3] if smin <= 1 else 32
    return list(range(1, tmax + 1))


def fused_params():
    return [(t[0], s) for t in TYPES for s in (0, 1)]


def fused_taps(tname, smin):
    return [T for T in strict_taps(tname, smin) if T % 4 == 0]


def mode_params():
    return [(t[0], s, T) for t in TYPES for s in (0, 1) for T in (24, 32)]


# the table of the issue, written out (not derived from the functions above, nor from the library)
STRICT_COUNT = {("f32xf32", 0): 64, ("f32xf32", 1): 64, ("f32xf32", 2): 32, ("f32xf32", 3): 32, ("f32xf32", 4): 32, ("f32xf32", 5): 32,
                ("f32xc64", 0): 64, ("f32xc64", 1): 64, ("f32xc64", 2): 32, ("f32xc64", 3): 32, ("f32xc64", 4): 32, ("f32xc64", 5): 32,
                ("f64xf64", 0): 48, ("f64xf64", 1): 48, ("f64xf32", 0): 48, ("f64xf32", 1): 48,
                ("f64xc64", 0): 32, ("f64xc64", 1): 32, ("f64xc128", 0): 32, ("f64xc128", 1): 32}
FUSED_COUNT = {("f32xf32", 0): 16, ("f32xf32", 1): 16, ("f32xc64", 0): 16, ("f32xc64", 1): 16,
               ("f64xf64", 0): 12, ("f64xf64", 1): 12, ("f64xf32", 0): 12, ("f64xf32", 1): 12,
               ("f64xc64", 0): 8, ("f64xc64", 1): 8, ("f64xc128", 0): 8, ("f64xc128", 1): 8}
STRICT_TOTAL, FUSED_TOTAL, MODE_TOTAL = 832, 144, 24


def ratio_for(tname, smin, T):
    """rotated by T + index(type): every ratio class meets every T somewhere across the types"""
    r = RATIOS[smin]
    return r[(T + TYPE_INDEX[tname]) % len(r)]


def hlen_for(tname, smin, T, L):
    """hLen = T*L - r, r rotating over 0, 1, L//2, L-1: ceil(hLen / L) stays T while taps2pfb zero-pads a ragged last row.  The
    rotation advances once per turn of the ratio rotation, so every ratio meets every r."""
    r = (0, 1, L // 2, L - 1)[(T // len(RATIOS[smin]) + TYPE_INDEX[tname] + smin) % 4]
    return T * L - r


def sample_bytes(tx):
    return np.dtype(tx).itemsize


def plan(L, M, T, th, tx, n_out, nch, num_cus=NUM_CUS):
    """c, P, cM, J, ns and the tiles per channel plan_rational_opair gives a host-planned call of n_out outputs per channel; None where
    it refuses the shape."""
    r_f64 = np.dtype(th) == np.dtype(F64)
    cplx = np.dtype(tx).kind == "c"
    nc = 2 if cplx else 1
    es = sample_bytes(tx)
    smin = M // L
    if T < 1 or T > ((32 if cplx else 48) if r_f64 else 64) or L < 2 or smin > 5 or (smin >= 2 and (r_f64 or T > 32)):
        return None

    def sizes():
        c = 2
        while c * L // 2 <= 512 and c * L <= 1024:
            yield c
            c += 2
    best_c, best = 0, -1.0
    for ps in range(2):
        if best_c:
            break
        for c in sizes():
            lanes = c * L // 2
            padded = (lanes + 63) // 64 * 64
            if ps == 0 and (padded < 192 or padded > 448):
                continue
            score = lanes / padded * (0.5 + 0.5 * padded / 192.0 if padded < 192 else 1.0)
            if score > best + 1e-9:
                best, best_c = score, c
    if n_out * nch < (1 << 22):
        for c in sizes():
            if c * L // 2 >= 128:
                best_c = c
                break
    if not best_c:
        return None
    if r_f64 and T > 32 and (best_c * L // 2 + 63) // 64 > 7:
        return None
    c = best_c
    cM, cL = c * M, c * L
    nwaves = (cL // 2 + 63) // 64
    tail = T + smin + 4
    vgpr_est = (2 * T + (36 if nc == 2 else 30) + 7) // 8 * 8
    waves_per_cu = 12 if r_f64 else 4 * min(8, 512 // vgpr_est)
    wgpc = max(1, min(4, waves_per_cu // (nwaves + 1)))
    if nwaves + 1 == 6:
        wgpc = 1 if r_f64 else 3
    ns = 3 if wgpc == 1 else 2
    budget_kib = ((150 if wgpc <= 3 else 160) * 1024 // wgpc - 64) // ns // 1024
    J = max(1, (max(budget_kib, 1) * 1024 // es - tail) // cM)
    J = min(J, 64)
    while J > 2 and -(-n_out // (J * cL)) * nch < 4 * num_cus:
        J = (J + 1) // 2
    max_slots = 60 // (ns - 2 if ns > 2 else 1)

    def slots(j):
        return (((j * cM + tail + 3) // 4 * 4) * es // 16 + 63) // 64
    while J > 1 and slots(J) > max_slots:
        J -= 1
    if slots(J) > max_slots or ns * slots(J) * 1024 > 156 * 1024:
        return None
    # the workgroups a CU can hold at once, whatever the kernel's registers allow: by the LDS of the stages as planned (160 KiB per
    # CU) and by its 32 wave slots -- an upper bound of the occupancy launch_opair_kernel sizes the grid with (a tile that stops at the
    # 60-slot or the J <= 64 cap leaves LDS for more workgroups than the wgpc the stages were budgeted for)
    lds = ns * slots(J) * 1024 + 8 * ns
    wg_bound = max(1, min(160 * 1024 // lds, 32 // (nwaves + 1)))
    return {"c": c, "P": cL, "cM": cM, "J": J, "ns": ns, "tiles_per_channel": -(-n_out // (J * cL)), "block": (nwaves + 1) * 64, "wgpc": wgpc,
            "wg_bound": wg_bound}


def many_outputs(L, M, T, th, tx):
    """outputs per channel of the many-tiles shape's large chunk: the fewest (in steps of 10 %) at which the call's tiles outnumber
    three times the workgroups the chip can hold (plan(): wg_bound per CU) -- pair_grid then hands tiles out by dynamic grabs"""
    n_out = 25_000
    while True:
        pl = plan(L, M, T, th, tx, n_out, MANY_CHANNELS)
        if pl["tiles_per_channel"] * MANY_CHANNELS > 3 * NUM_CUS * pl["wg_bound"]:
            return n_out
        n_out += n_out // 10


def n_outputs(L, M, n_in):
    """outputs of a first call of n_in samples on a fresh FIRRational / FIRInterpolator (phiIdx = 1, inputDeficit = 1)"""
    return -(-n_in * L // M)


def _rand(rng, shape, tx):
    if np.dtype(tx).kind == "c":
        return ((rng.random(shape) - 0.5) + 1j * (rng.random(shape) - 0.5)).astype(tx)
    return (rng.random(shape) - 0.5).astype(tx)


def _real_view(x):
    return x.view(F64 if x.dtype in (np.dtype(F64), np.dtype(C128)) else F32)


def taps(rng, hlen, th):
    """standard-normal taps, min(3, hLen // 4) of them (distinct ones) exactly 0.0: at least max(1, hLen - 3) stay non-zero"""
    h = rng.standard_normal(hlen).astype(th)
    h[h == 0.0] = 1.0
    h[rng.choice(hlen, size=min(3, hlen // 4), replace=False)] = 0.0
    return h


def _patch(x, T, smin, zero_at, inf_at, nan_at):
    """the edge patches, in place: runs of -0.0 longer than a lane's run of samples (T + SMIN + 4) in all rows, +Inf and -Inf in
    row 0, a 3-sample NaN run in the last row"""
    k = 2 if np.iscomplexobj(x) else 1
    xr = _real_view(x)
    run = T + smin + 4 + 9
    for z in zero_at:
        xr[:, k * z:k * (z + run)] = -0.0
    xr[0, k * inf_at] = np.inf
    xr[0, k * (inf_at + 97) + (k - 1)] = -np.inf
    xr[-1, k * nan_at:k * (nan_at + 3)] = np.nan


def many_case(rng, tname, smin, T, n_out=None):
    """(ratio, h, the 4 distinct rows, chunk sizes [p, 1, 13, rest]): `rest` gives many_outputs() outputs per channel"""
    _, th, tx, _, _ = TYPES[TYPE_INDEX[tname]]
    ratio = ratio_for(tname, smin, T)
    L, M = ratio.numerator, ratio.denominator
    h = taps(rng, hlen_for(tname, smin, T, L), th)
    p = (1009, 2003, 3001, 4001)[(T + smin) % 4]
    rest = (n_out or many_outputs(L, M, T, th, tx)) * M // L
    sizes = [p, 1, 13, rest]
    x = _rand(rng, (MANY_ROWS, sum(sizes)), tx)
    # one run of -0.0 lies across the three short chunks' boundaries, one inside the large chunk
    _patch(x, T, smin, zero_at=(p - 7, p + 14 + rest // 7), inf_at=p + 14 + rest // 5, nan_at=p + 14 + rest // 3)
    return ratio, h, x, sizes


def short_case(rng, tname, smin, T):
    """(ratio, h, 3 rows, chunk sizes [n, T - 1]): n is a little over two tiles of the plan (a partial last step in a partial last
    tile), the second chunk is shorter than a window"""
    _, th, tx, _, _ = TYPES[TYPE_INDEX[tname]]
    ratio = ratio_for(tname, smin, T)
    L, M = ratio.numerator, ratio.denominator
    h = taps(rng, hlen_for(tname, smin, T, L), th)
    n = 3 * 256 * M // L                                    # (any small call: J ends at <= 2 and c*L/2 is the first size >= 128 lanes)
    pl = plan(L, M, T, th, tx, n_outputs(L, M, n), SHORT_CHANNELS)
    n = 2 * pl["J"] * pl["cM"] + (pl["J"] * pl["cM"]) // 2 + pl["cM"] // 3 + 1
    sizes = [n, T - 1]
    x = _rand(rng, (SHORT_CHANNELS, sum(sizes)), tx)
    _patch(x, T, smin, zero_at=(n // 9,), inf_at=n // 3, nan_at=n // 2)
    return ratio, h, x, sizes


# the guard's cases: per (type, SMIN) one T per ratio of the table (consecutive T: the rotation), other T for the short shape -- the
# library reports an instantiation's geometry once per process
GUARD_T_MANY, GUARD_T_SHORT = 17, 5


def guard_cases():
    for tname, smin in strict_params():
        for k in range(len(RATIOS[smin])):
            yield "many", tname, smin, GUARD_T_MANY + k
            yield "short", tname, smin, GUARD_T_SHORT + k


def _guard_child():
    """(run as a script by test_many_tiles_shape_takes_dynamic_grabs, MRHIP_DEBUG=1) the large chunk of the many-tiles shape and the
    first call of the short shape, each as the first launch of its instantiation; a CASE line in front of the library's own"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    rng = np.random.default_rng(4)
    for kind, tname, smin, T in guard_cases():
        _, th, tx, _, _ = TYPES[TYPE_INDEX[tname]]
        ratio, h, x, sizes = (many_case if kind == "many" else short_case)(rng, tname, smin, T)
        reps = MANY_CHANNELS // MANY_ROWS if kind == "many" else 1
        n = sizes[-1] if kind == "many" else sizes[0]
        xd = torch.from_numpy(np.tile(x[:, :n], (reps, 1))).cuda()
        f = pkg.FIRFilter(h, ratio)
        n_out = n_outputs(ratio.numerator, ratio.denominator, n)
        pl = plan(ratio.numerator, ratio.denominator, T, th, tx, n_out, xd.shape[0])
        sys.stderr.write(f"CASE {kind} {tname} {smin} {T} {n_out} {xd.shape[0]} {pl['P']} {pl['J']}\n")
        sys.stderr.flush()
        y = f.filt(xd)
        assert y.shape[-1] == n_out and f.last_kernel_name() == "rational_opair_kernel", (kind, tname, smin, T, y.shape, f.last_kernel_name())
        f.close()
    torch.cuda.synchronize()


if __name__ == "__main__":
    _guard_child()
