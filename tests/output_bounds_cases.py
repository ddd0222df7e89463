"""The case table and the checker of test_gpu_output_bounds.py / test_output_bounds_cpu.py (no tests here).

Contract under test (include/multirate_hip.h, "the hot path"): a call writes y[c][0 .. count) of every channel row and NOTHING else --
whatever y's alignment, whatever y_stride >= the required minimum, through every entry point, also when it fails with
MRHIP_ERR_BUFFER_TOO_SMALL.

CASES maps every kernel name of csrc ("[a-z_]+_kernel" string literals) to the smallest shapes that reach it, one per store path of
the kernel.  make_buffer / assert_only_written are the poisoned buffer and its host-side check.  Everything but make_buffer is numpy,
so the table and the checker are tested on a CPU-only box.
"""
import os
import re
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
POISON = 0xA5
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multirate.jl_amd", "csrc")


def kernel_names_in_csrc():
    """the set of string literals "[a-z_]+_kernel" under csrc: what last_kernel_name() can return"""
    names = set()
    for root, _, files in os.walk(CSRC):
        for fn in files:
            if fn.endswith((".hip", ".inc", ".h", ".cpp")):
                with open(os.path.join(root, fn), errors="replace") as fh:
                    names.update(re.findall(r'"([a-z_]+_kernel)"', fh.read()))
    return names


# ---- the case table ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    kernel: str                     # the expected last_kernel_name() of every call long enough for the kernel
    ctor: str                       # "shared" | "complex_taps" | "per_channel" | "per_channel_complex_taps"
    kind: str                       # "rational" | "arbitrary" | "farrow"
    th: type                        # tap dtype
    tx: type                        # sample dtype
    ratio: object                   # Fraction (rational family) or float (rate)
    hlen: int                       # tap count
    nch: int
    lengths: tuple                  # nominal lengths of the two long calls (plan_sizes moves them up to an odd / an even count)
    Nphi: int = 32
    polyorder: object = None
    env: tuple = ()                 # the MRHIP_* switches that force the kernel
    fused: bool = False             # the kernel has FUSED instantiations for this shape
    ring: bool = False              # open_ring() serves the shape with the resident kernel
    one_channel: bool = True        # the kernel also takes a single channel (1-D x and y)
    short_calls_elsewhere: bool = False   # calls below the kernel's minimum length run on another kernel (the lane kernels)
    min_count: int = 768            # both long calls have more outputs per channel than this (two tiles and a ragged third)
    async_kernel: object = None     # the kernel of the shape's device-planned calls where it is not ASYNC_KERNEL's

    @property
    def async_name(self):
        return self.async_kernel or ASYNC_KERNEL.get(self.kernel, self.kernel)

    @property
    def L(self):
        return self.ratio.numerator if self.kind == "rational" else None

    @property
    def M(self):
        return self.ratio.denominator if self.kind == "rational" else None

    @property
    def out_dtype(self):
        wide = np.dtype(self.th) in (np.dtype(F64), np.dtype(C128)) or np.dtype(self.tx) in (np.dtype(F64), np.dtype(C128))
        cplx = np.dtype(self.th).kind == "c" or np.dtype(self.tx).kind == "c"
        return np.dtype((C128 if wide else C64) if cplx else (F64 if wide else F32))


def _r(L, M):
    return Fraction(L, M)


# kernels that take host-planned calls only: a call planned on the device (filt_into_async, a HIP-graph capture) of their shapes
# runs on the kernel named here, which reads the call record
ASYNC_KERNEL = {"poly_tiled_kernel": "poly_generic_kernel", "poly_phase_stationary_kernel": "poly_generic_kernel",
                "interp_lane_kernel": "rational_opair_kernel", "poly_ctaps_tiled_kernel": "poly_ctaps_generic_kernel",
                "poly_bank_tiled_kernel": "poly_bank_generic_kernel", "poly_bank_ctaps_tiled_kernel": "poly_bank_ctaps_generic_kernel"}

GEN = (("MRHIP_FORCE_GENERIC", "1"),)
RATE = float(np.pi / 3)

_ALL = [
    # ---- the rational family, shared real taps (the reaching shapes: tests/test_gpu_parity.py) ----
    Case("generic-5_7-f32", "poly_generic_kernel", "shared", "rational", F32, F32, _r(5, 7), 33, 3, (2200, 2300), env=GEN, fused=True),
    Case("generic-3_2-c64", "poly_generic_kernel", "shared", "rational", F32, C64, _r(3, 2), 72, 2, (900, 1000), env=GEN),
    Case("generic-1_3-f64", "poly_generic_kernel", "shared", "rational", F64, F64, _r(1, 3), 31, 3, (3000, 3100), env=GEN),
    Case("tiled-2_3-f32", "poly_tiled_kernel", "shared", "rational", F32, F32, _r(2, 3), 140, 3, (2400, 2500), fused=True),      # 70 taps per phase
    Case("tiled-3_2-c64", "poly_tiled_kernel", "shared", "rational", F32, C64, _r(3, 2), 200, 2, (900, 1000)),                   # 67 taps per phase
    Case("tiled-2_3-f64", "poly_tiled_kernel", "shared", "rational", F64, F64, _r(2, 3), 100, 4, (2400, 2500)),                   # 50 taps per phase, Float64
    Case("tiled-1_7-c128", "poly_tiled_kernel", "shared", "rational", F64, C128, _r(1, 7), 129, 2, (5600, 5700), env=(("MRHIP_STREAM", "0"),)),
    Case("phase-3_17-f64", "poly_phase_stationary_kernel", "shared", "rational", F64, F64, _r(3, 17), 50, 3, (9000, 9500), fused=True),
    Case("phase-4_33-f32", "poly_phase_stationary_kernel", "shared", "rational", F32, F32, _r(4, 33), 19, 5, (13000, 13500),
         env=(("MRHIP_OPAIR", "0"),)),
    # rational_opair_kernel: NC = 1 and 2, Float32 and Float64 (the 8-byte pair: Float32 outputs), L > 512 (period blocks)
    Case("opair-147_160-f32", "rational_opair_kernel", "shared", "rational", F32, F32, _r(147, 160), 147 * 24, 3, (2000, 2100), fused=True, ring=True),
    Case("opair-3_2-c64", "rational_opair_kernel", "shared", "rational", F32, C64, _r(3, 2), 72, 2, (900, 1000), fused=True, ring=True),
    Case("opair-7_5-f64", "rational_opair_kernel", "shared", "rational", F64, F64, _r(7, 5), 7 * 24, 3, (1200, 1300), fused=True, ring=True),
    Case("opair-3_2-c128", "rational_opair_kernel", "shared", "rational", F64, C128, _r(3, 2), 3 * 32, 2, (900, 1000), fused=True, ring=True),
    Case("opair-2_5-f32", "rational_opair_kernel", "shared", "rational", F32, F32, _r(2, 5), 2 * 31, 3, (4000, 4100)),            # window distance 2
    Case("opair-625_512-f32", "rational_opair_kernel", "shared", "rational", F32, F32, _r(625, 512), 625 * 24, 2, (2000, 2100),
         async_kernel="poly_generic_kernel"),                                                                                       # L > 512: period blocks, planned on the host
    # fir_stream_kernel: an odd M, an even M (linear tile), a padded tile (pad_every > 0: 4-byte samples with M % 4 == 0), the
    # hand-scheduled ComplexF32 1//4 x 128 taps pair
    Case("stream-1_3-f32", "fir_stream_kernel", "shared", "rational", F32, F32, _r(1, 3), 48, 3, (3000, 3100), fused=True),
    Case("stream-1_2-f32", "fir_stream_kernel", "shared", "rational", F32, F32, _r(1, 2), 48, 3, (2000, 2100), fused=True),
    Case("stream-1_4-f32", "fir_stream_kernel", "shared", "rational", F32, F32, _r(1, 4), 128, 3, (4000, 4100), fused=True),
    Case("stream-1_1-f64", "fir_stream_kernel", "shared", "rational", F64, F64, _r(1, 1), 48, 2, (900, 1000), fused=True),
    Case("stream-1_4-c64-hand", "fir_stream_kernel", "shared", "rational", F32, C64, _r(1, 4), 128, 5, (4000, 4100), fused=True),
    # fir_stream_rt_kernel: two outputs per lane and one
    Case("stream_rt-1_24-c64-pair", "fir_stream_rt_kernel", "shared", "rational", F32, C64, _r(1, 24), 100, 3, (19000, 19500),
         env=(("MRHIP_STREAM_RT_SINGLE", "0"),)),
    Case("stream_rt-1_24-c64-single", "fir_stream_rt_kernel", "shared", "rational", F32, C64, _r(1, 24), 100, 3, (19000, 19500),
         env=(("MRHIP_STREAM_RT_SINGLE", "1"),)),
    Case("stream_rt-1_5-f32-pair", "fir_stream_rt_kernel", "shared", "rational", F32, F32, _r(1, 5), 24, 3, (4000, 4100),
         env=(("MRHIP_STREAM_RT", "2"),), fused=True),                                                                              # odd M, Float32: pairs
    # interp_lane_kernel: a full channel group and a partial one
    Case("interp_lane-64ch", "interp_lane_kernel", "shared", "rational", F32, C64, _r(4, 1), 128, 64, (1001, 1100),
         env=(("MRHIP_INTERP_LANE", "2"),), fused=True, one_channel=False, short_calls_elsewhere=True),
    Case("interp_lane-50ch", "interp_lane_kernel", "shared", "rational", F32, C64, _r(4, 1), 128, 50, (1001, 1100),
         env=(("MRHIP_INTERP_LANE", "2"),), one_channel=False, short_calls_elsewhere=True),
    # ---- FIRArbitrary, shared real taps ----
    Case("arb_generic-f32", "arb_generic_kernel", "shared", "arbitrary", F32, F32, 2.7, 8 * 5, 3, (400, 450), Nphi=8, env=GEN, fused=True),
    Case("arb_generic-c128", "arb_generic_kernel", "shared", "arbitrary", F64, C128, 0.9991, 48 * 17, 2, (1000, 1100), Nphi=48, env=GEN),
    Case("arb_tiled-c128", "arb_tiled_kernel", "shared", "arbitrary", F64, C128, 0.9991, 48 * 17, 3, (1000, 1100), Nphi=48, fused=True),
    Case("arb_tiled-f32", "arb_tiled_kernel", "shared", "arbitrary", F32, F32, 2.7, 8 * 5, 3, (400, 450), Nphi=8, env=(("MRHIP_ARB_PIPE", "0"),), fused=True),
    Case("arb_pipe-c64", "arb_pipe_kernel", "shared", "arbitrary", F32, C64, 0.37, 32 * 10, 3, (2600, 2700), fused=True),
    Case("arb_pipe-f64", "arb_pipe_kernel", "shared", "arbitrary", F64, F64, RATE, 32 * 32, 3, (900, 1000), fused=True),
    Case("arb_pipe-f32", "arb_pipe_kernel", "shared", "arbitrary", F32, F32, 2.7, 8 * 5, 5, (400, 450), Nphi=8, fused=True),
    Case("arb_lane-64ch", "arb_lane_kernel", "shared", "arbitrary", F64, F64, RATE, 32 * 32, 64, (900, 1000), fused=True, one_channel=False,
         short_calls_elsewhere=True),
    Case("arb_lane-50ch", "arb_lane_kernel", "shared", "arbitrary", F64, F64, 2.7, 32 * 32, 50, (400, 450), one_channel=False, short_calls_elsewhere=True),
    # ---- FIRFarrow, shared real taps ----
    Case("farrow_generic-f64", "farrow_kernel", "shared", "farrow", F64, F64, RATE, 32 * 12, 3, (900, 1000), polyorder=4, env=GEN, fused=True),
    Case("farrow_tiled-f64-40taps", "farrow_tiled_kernel", "shared", "farrow", F64, F64, RATE, 32 * 40, 3, (900, 1000), polyorder=4, fused=True),
    Case("farrow_tiled-c64", "farrow_tiled_kernel", "shared", "farrow", F32, C64, 2.7, 8 * 25, 3, (400, 450), Nphi=8, polyorder=3,
         env=(("MRHIP_FARROW_PIPE", "0"), ("MRHIP_FARROW_WAVE", "0"))),
    Case("farrow_pipe-c64", "farrow_pipe_kernel", "shared", "farrow", F32, C64, RATE, 32 * 17, 3, (900, 1000), polyorder=4,
         env=(("MRHIP_FARROW_WAVE", "0"),), fused=True),
    Case("farrow_pipe-f64", "farrow_pipe_kernel", "shared", "farrow", F64, F64, RATE, 32 * 32, 5, (900, 1000), polyorder=4,
         env=(("MRHIP_FARROW_WAVE", "0"),), fused=True),
    Case("farrow_wave-f64", "farrow_wave_kernel", "shared", "farrow", F64, F64, RATE, 32 * 12, 3, (900, 1000), polyorder=4, fused=True),
    Case("farrow_wave-f32", "farrow_wave_kernel", "shared", "farrow", F32, F32, 1.9, 32 * 7, 5, (500, 550), polyorder=4, fused=True),
    # ---- complex taps (tests/test_gpu_complex_taps*.py) ----
    Case("ctaps_generic-3_2", "poly_ctaps_generic_kernel", "complex_taps", "rational", C64, F32, _r(3, 2), 24, 3, (600, 650), env=GEN),
    Case("ctaps_tiled-3_2", "poly_ctaps_tiled_kernel", "complex_taps", "rational", C64, C64, _r(3, 2), 24, 3, (600, 650), env=(("MRHIP_CTAPS_TILED", "1"),)),
    Case("ctaps_tiled-1_2-c128", "poly_ctaps_tiled_kernel", "complex_taps", "rational", C128, F32, _r(1, 2), 17, 2, (1700, 1800), env=(("MRHIP_CTAPS_TILED", "1"),)),
    Case("arb_ctaps_generic", "arb_ctaps_generic_kernel", "complex_taps", "arbitrary", C64, F32, 1.37, 250, 3, (650, 700), env=(("MRHIP_CTAPS_TILED", "0"),)),
    Case("arb_ctaps_tiled", "arb_ctaps_tiled_kernel", "complex_taps", "arbitrary", C64, C64, 1.37, 250, 3, (650, 700), env=(("MRHIP_CTAPS_TILED", "1"),)),
    Case("farrow_ctaps_generic", "farrow_ctaps_generic_kernel", "complex_taps", "farrow", C64, F32, 1.37, 250, 3, (650, 700), polyorder=4, env=(("MRHIP_CTAPS_TILED", "0"),)),
    Case("farrow_ctaps_tiled", "farrow_ctaps_tiled_kernel", "complex_taps", "farrow", C64, C64, 1.37, 250, 3, (650, 700), polyorder=4, env=(("MRHIP_CTAPS_TILED", "1"),)),
    # ---- per-channel taps (tests/test_gpu_*bank*.py) ----
    Case("bank_generic-3_2", "poly_bank_generic_kernel", "per_channel", "rational", F32, F32, _r(3, 2), 24, 3, (600, 650), env=GEN, fused=True),
    Case("bank_tiled-3_2", "poly_bank_tiled_kernel", "per_channel", "rational", F32, F32, _r(3, 2), 24, 3, (600, 650), env=(("MRHIP_BANK_TILED", "1"),), fused=True),
    Case("bank_tiled-1_2-c128", "poly_bank_tiled_kernel", "per_channel", "rational", F64, C128, _r(1, 2), 17, 2, (1700, 1800), env=(("MRHIP_BANK_TILED", "1"),)),
    Case("bank_ctaps_generic-3_2", "poly_bank_ctaps_generic_kernel", "per_channel_complex_taps", "rational", C64, F32, _r(3, 2), 24, 3, (600, 650), env=GEN),
    Case("bank_ctaps_tiled-3_2", "poly_bank_ctaps_tiled_kernel", "per_channel_complex_taps", "rational", C64, C64, _r(3, 2), 24, 3, (600, 650),
         env=(("MRHIP_BANK_CTAPS_TILED", "1"),)),
    Case("arb_bank_generic", "arb_bank_generic_kernel", "per_channel", "arbitrary", F32, F32, 1.37, 250, 3, (650, 700), env=GEN, fused=True),
    Case("arb_bank_tiled", "arb_bank_tiled_kernel", "per_channel", "arbitrary", F32, C64, 1.37, 250, 3, (650, 700), env=(("MRHIP_ARB_BANK_TILED", "1"),), fused=True),
    Case("arb_bank_ctaps_generic", "arb_bank_ctaps_generic_kernel", "per_channel_complex_taps", "arbitrary", C64, F32, 1.37, 250, 3, (650, 700), env=GEN),
    Case("arb_bank_ctaps_tiled", "arb_bank_ctaps_tiled_kernel", "per_channel_complex_taps", "arbitrary", C64, C64, 1.37, 250, 3, (650, 700),
         env=(("MRHIP_ARB_BANK_CTAPS_TILED", "1"),)),
    Case("farrow_bank_generic", "farrow_bank_generic_kernel", "per_channel", "farrow", F32, F32, 1.37, 250, 3, (650, 700), polyorder=4, env=GEN, fused=True),
    Case("farrow_bank_tiled", "farrow_bank_tiled_kernel", "per_channel", "farrow", F32, C64, 1.37, 250, 3, (650, 700), polyorder=4,
         env=(("MRHIP_FARROW_BANK_TILED", "1"),), fused=True),
    Case("farrow_bank_ctaps_generic", "farrow_bank_ctaps_generic_kernel", "per_channel_complex_taps", "farrow", C64, F32, 1.37, 250, 3, (650, 700), polyorder=4),
    Case("farrow_bank_ctaps_generic-c128", "farrow_bank_ctaps_generic_kernel", "per_channel_complex_taps", "farrow", C128, C64, 1.37, 250, 2, (650, 700), polyorder=4),
]

CASES = {}
for _c in _ALL:
    CASES.setdefault(_c.kernel, []).append(_c)
ALL_CASES = list(_ALL)
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)

MAX_SIGNAL = 40_000                 # samples per channel, all calls of a case together
MAX_CHANNELS_OUTSIDE_LANE = 5

# layouts: name -> (oy in elements, parity of the row stride, ox in elements)
LAYOUTS = {"tight": (0, "tight", 0), "A": (1, "odd", 1), "B": (2, "even", 3), "C": (3, "odd", 2)}


def layouts_for(elemsize):
    """4-byte outputs: the four oy reach every residue of the base address modulo 16; 8-byte: oy = 2, 3 repeat residues; 16-byte: two"""
    return ["tight", "A", "B", "C"] if elemsize == 4 else ["tight", "A"]


def layouts_of(case):
    """the layouts of a case: by its output element size, and layout B (oy = 2, an even row stride: a 16-byte aligned row base at every
    row) for the lane kernels, whose 16-byte stores are chosen from the alignment of y and the parity of y_stride"""
    names = layouts_for(case.out_dtype.itemsize)
    if case.kernel in ("arb_lane_kernel", "interp_lane_kernel") and "B" not in names:
        names = names + ["B"]
    return names


def row_pad(layout, oy, cap, elemsize):
    """guard columns behind the view so that the row stride oy + cap + pad has the layout's parity (B: even, and stride * elemsize
    no multiple of 16 where the element size allows it, i.e. for 4-byte elements)"""
    parity = LAYOUTS[layout][1]
    if parity == "tight":
        return 0
    for pad in range(1, 9):
        s = oy + cap + pad
        if parity == "odd" and s % 2 == 1:
            return pad
        if parity == "even" and s % 2 == 0 and (elemsize != 4 or (s * elemsize) % 16 != 0):
            return pad
    raise AssertionError("no pad")


# ---- taps and signals ------------------------------------------------------------------------------------------------------------
def make_taps(case, nch=None):
    """a tap vector (shared constructors) or a (nch, hLen) matrix (per-channel constructors); up to three exact zeros per vector"""
    nch = case.nch if nch is None else nch
    rng = np.random.default_rng(sum(map(ord, case.id)))
    rows = nch if case.ctor.startswith("per_channel") else 1
    scale = max(case.hlen / (case.Nphi if case.kind != "rational" else case.L), 1.0)      # (about one tap per phase of unit size)
    H = rng.standard_normal((rows, case.hlen)) / scale
    if np.dtype(case.th).kind == "c":
        H = H + 1j * rng.standard_normal((rows, case.hlen)) / scale
    H = H.astype(case.th)
    for r in range(rows):
        H[r, rng.integers(0, case.hlen, 3)] = 0
    return H if case.ctor.startswith("per_channel") else H[0]


def make_signal(case, n, nch=None):
    """finite standard normals (no NaN: the interior is compared bit for bit)"""
    nch = case.nch if nch is None else nch
    rng = np.random.default_rng(7 + sum(map(ord, case.id)))
    x = rng.standard_normal((nch, n))
    if np.dtype(case.tx).kind == "c":
        x = x + 1j * rng.standard_normal((nch, n))
    return x.astype(case.tx)


# ---- call lengths ----------------------------------------------------------------------------------------------------------------
def _counter(O, case):
    """the per-call output counts depend on (L, M) or (rate, Nphi) and the call lengths only: a one-tap-per-phase oracle counts them"""
    if case.kind == "rational":
        return O.FIRFilter(np.ones(case.L, dtype=np.float32), case.ratio, tx=np.float32)
    return O.FIRFilter(np.ones(case.Nphi, dtype=np.float32), float(case.ratio), case.Nphi, tx=np.float32)


def call_counts(O, case, sizes):
    f = _counter(O, case)
    return [len(f.filt(np.zeros(s, dtype=np.float32))) for s in sizes]


_PLANS = {}


def plan_sizes(O, case):
    """[n_a, n_none, n_few, n_b]: a long call with an odd per-channel count, a call too short to produce any output (an empty one
    where every sample gives outputs), the shortest call that has outputs (ONE output wherever the kind allows it), a long call
    with an even count; neither long count a multiple of 64, both above case.min_count.  The nominal lengths of the table only
    move up, by a few samples."""
    if case.id in _PLANS:
        return _PLANS[case.id]

    # FIRInterpolator with an even L has no odd count: its "odd" call has an odd number of INPUTS (a count that is no multiple of 2 L)
    no_odd = case.kind == "rational" and case.M == 1 and case.L % 2 == 0

    def long_call(prefix, n, odd):
        for n in range(n, n + 4000):
            cnt = call_counts(O, case, prefix + [n])[-1]
            parity = n % 2 if no_odd else cnt % 2
            if parity == (1 if odd else 0) and cnt % 64 != 0 and cnt > case.min_count:
                return n
        raise AssertionError(f"{case.id}: no call length near {n} with an {'odd' if odd else 'even'} count")

    na = long_call([], case.lengths[0], True)
    n_none = 1 if call_counts(O, case, [na, 1])[-1] == 0 else 0
    n_few = next(n for n in range(1, 4096) if call_counts(O, case, [na, n_none, n])[-1] > 0)
    nb = long_call([na, n_none, n_few], case.lengths[1], False)
    _PLANS[case.id] = [na, n_none, n_few, nb]
    return _PLANS[case.id]


def odd_piece(O, case, n, start):
    """a piece length >= start (for filt_into_chunked / MRHIP_LAUNCH_MAX) whose first piece has an odd output count: the second piece
    then starts at an odd element of y.  FIRInterpolator with an even L has no such length: start."""
    for p in range(start, start + 256):
        if call_counts(O, case, [p])[0] % 2 == 1:
            return p
    return start


def pieces(n, p):
    return [min(p, n - a) for a in range(0, n, p)]


# ---- the poisoned buffer and its check ---------------------------------------------------------------------------------------------
def make_buffer(torch, dtype, nch, cap, oy, pad, device="cuda"):
    """(view, backing): bytes all 0xA5 seen as (nch + 2, oy + cap + pad) elements of ``dtype``; the view is [1:1 + nch, oy:oy + cap].
    The first and the last row, the oy columns in front and the pad columns behind are guards."""
    dt = np.dtype(dtype)
    tdt = {np.dtype(F32): torch.float32, np.dtype(F64): torch.float64, np.dtype(C64): torch.complex64, np.dtype(C128): torch.complex128}[dt]
    width = oy + cap + pad
    raw = torch.full(((nch + 2) * width * dt.itemsize,), POISON, dtype=torch.uint8, device=device)
    backing = raw.view(tdt).view(nch + 2, width)
    return backing[1:1 + nch, oy:oy + cap], backing


def backing_bytes(backing):
    """the backing store on the host as (rows, width * elemsize) bytes and the element size"""
    a = backing.detach().cpu().numpy() if hasattr(backing, "detach") else np.asarray(backing)
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1), a.dtype.itemsize


def first_stray(bytes2d, allowed):
    """(row, byte column) of the first byte that is not poison outside ``allowed`` (a boolean mask of the same shape), or None"""
    bad = (bytes2d != POISON) & ~allowed
    if not bad.any():
        return None
    r, b = np.argwhere(bad)[0]
    return int(r), int(b)


def assert_only_written(backing, nch, cap, oy, pad, count, what):
    """every byte outside rows 1 .. nch, columns oy .. oy + count of the backing store is still 0xA5; reports the first stray element's
    row and column relative to the view (row -1 / nch: the guard rows; column -1: the element in front of a row; column >= count: behind
    its last output)"""
    by, es = backing_bytes(backing)
    assert by.shape == (nch + 2, (oy + cap + pad) * es), (what, by.shape, nch, cap, oy, pad, es)
    assert 0 <= count <= cap, (what, count, cap)
    allowed = np.zeros(by.shape, dtype=bool)
    allowed[1:1 + nch, oy * es:(oy + count) * es] = True
    hit = first_stray(by, allowed)
    if hit is not None:
        r, b = hit
        n_bad = int(((by != POISON) & ~allowed).sum())
        raise AssertionError(f"{what}: wrote outside its outputs: first stray element at row {r - 1}, column {b // es - oy} of the view "
                             f"(byte {b % es} of the element; {nch} rows, count {count}, capacity {cap}, guards {oy} in front / {pad} behind); "
                             f"{n_bad} stray bytes in all")


# ---- references (never the library) and the filters under test ------------------------------------------------------------------
class Ref:
    """one channel of the reference: the C oracle for real taps, the restatement classes for complex taps"""

    def __init__(self, obj, kind, restated):
        self.obj, self.kind, self.restated = obj, kind, restated

    def filt(self, x):
        if self.restated and self.kind != "rational":
            return self.obj.filt(x, scalar=False)
        return self.obj.filt(x)

    def state(self):
        s = self.obj if self.restated else self.obj.state
        if self.kind == "rational":
            return (s.phiIdx, s.inputDeficit)
        if self.kind == "arbitrary":
            return (s.inputDeficit, s.phiAccumulator, s.phiIdx)
        return (s.inputDeficit, s.phiAccumulator)

    def history(self):
        return self.obj.history_array() if self.restated else self.obj.history


def library_state(f, kind):
    s = f.state
    if kind == "rational":
        return (s.phiIdx, s.inputDeficit)
    if kind == "arbitrary":
        return (s.inputDeficit, s.phiAccumulator, s.phiIdx)
    return (s.inputDeficit, s.phiAccumulator)


def _real_fit(pkg, O, h, Nphi, P):
    """pfb2pnfb with the library's per-row fit, stored in the tap type (what per_channel_farrow fits by itself)"""
    pfb = O.taps2pfb(h, Nphi)
    return np.stack([pkg.polyfit(pfb[i].astype(np.float64), P).astype(h.dtype).astype(np.float64) for i in range(pfb.shape[0])])


def make_refs(pkg, O, case, taps, nch):
    """([one Ref per channel], the polynomial bank to hand to the library or None)"""
    from complex_taps_arb_restatement import ComplexTapsArbitraryRestated
    from complex_taps_farrow_restatement import ComplexTapsFarrowRestated, fit_pnfb
    from complex_taps_restatement import ComplexTapsRestated
    bank = case.ctor.startswith("per_channel")
    cplx = np.dtype(case.th).kind == "c"
    refs, pnfb = [], None
    for c in range(nch):
        h = np.ascontiguousarray(taps[c] if bank else taps)
        if case.kind == "rational":
            obj = ComplexTapsRestated(h, case.ratio, tx=case.tx) if cplx else O.FIRFilter(h, case.ratio, tx=case.tx)
        elif case.kind == "arbitrary":
            obj = (ComplexTapsArbitraryRestated(h, float(case.ratio), case.Nphi, tx=case.tx) if cplx
                   else O.FIRFilter(h, float(case.ratio), case.Nphi, tx=case.tx))
        elif cplx:
            fit = fit_pnfb(h, case.Nphi, case.polyorder, pkg.polyfit)
            pnfb = None if bank else fit
            obj = ComplexTapsFarrowRestated(len(h), h.dtype, float(case.ratio), case.Nphi, case.polyorder, fit, tx=case.tx)
        else:
            fit = _real_fit(pkg, O, h, case.Nphi, case.polyorder) if bank else O.pfb2pnfb(O.taps2pfb(h, case.Nphi), case.polyorder)
            pnfb = None if bank else fit
            obj = O.FIRFilter(h, float(case.ratio), case.Nphi, tx=case.tx, polyorder=case.polyorder, pnfb=fit)
        refs.append(Ref(obj, case.kind, cplx))
    return refs, pnfb


def make_filter(pkg, case, taps, nch, pnfb=None, fused=False):
    """the bound filter of a case (the MRHIP_* switches of case.env must be set: MRHIP_FORCE_GENERIC is read here)"""
    F = pkg.FIRFilter
    num = {"numerics": pkg.NUMERICS_FUSED} if fused else {}
    ratio = case.ratio if case.kind == "rational" else float(case.ratio)
    if case.ctor == "shared":
        f = F(taps, ratio, **num) if case.kind == "rational" else F(taps, ratio, case.Nphi, case.polyorder, pnfb=pnfb, **num)
    elif case.ctor == "complex_taps":
        f = (F.complex_taps(taps, ratio) if case.kind == "rational" else F.complex_taps_arbitrary(taps, ratio, case.Nphi) if case.kind == "arbitrary"
             else F.complex_taps_farrow(taps, ratio, case.Nphi, case.polyorder, pnfb=pnfb))
    elif case.ctor == "per_channel":
        f = (F.per_channel(taps, ratio, **num) if case.kind == "rational" else F.per_channel_arbitrary(taps, ratio, case.Nphi, **num) if case.kind == "arbitrary"
             else F.per_channel_farrow(taps, ratio, case.Nphi, case.polyorder, **num))
    else:
        f = (F.per_channel_complex_taps(taps, ratio) if case.kind == "rational"
             else F.per_channel_complex_taps_arbitrary(taps, ratio, case.Nphi) if case.kind == "arbitrary"
             else F.per_channel_complex_taps_farrow(taps, ratio, case.Nphi, case.polyorder))
    return f.bind(case.tx, nch)
