"""CPU-only checks of per-channel rates for FIRArbitrary (FIRFilter.per_channel_rates, mrhip_create_arbitrary_rates,
csrc/kernels_rates_arb.hip): the four exported symbols and their declarations, the argument errors of the Python constructor, the
answers the older constructors keep, the build conditions of the kernel unit, the instantiations in the object the build made (the
two filter kernels for (Tx scalar, R) in {(f32,f32), (f32,f64), (f64,f64)} x real / complex samples x STRICT / FUSED = 12 each for
shared taps and 12 each for a bank per channel, the schedule kernel for a power-of-two N𝜙 and for any other; none with scratch memory
or AccVGPRs), the serial walk over the shared step header (csrc/sched_step.h) in a stand-alone program built by the host compiler with
-ffp-contract=off, against the oracle's schedule, and the tiled kernel's plan (csrc/host_logic.cpp: plan_arb_rates_tiled, which takes
either bank key) through a second stand-alone program, built with -fsanitize=address,undefined, against values computed here from the
plan's stated formulas."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _assert_rates_filter_kernel, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = 1024
SYMBOLS = ("mrhip_create_arbitrary_rates", "mrhip_filt_device_rates", "mrhip_get_channel_states", "mrhip_set_channel_states")


def test_the_library_exports_the_four_symbols_and_the_header_declares_them(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len([1 for n, _, _ in pkg.host.ABI if n == name]) == 1, name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_create_arbitrary_rates\(const void \*h, int64_t hLen, int tap_dtype, const double \*rates,\s*"
                     r"int64_t Nphi, int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)
    assert re.search(r"int mrhip_filt_device_rates\(mrhip_filter \*f, const void \*x, int64_t x_len, int64_t x_stride,\s*"
                     r"void \*y, int64_t y_capacity, int64_t y_stride, int64_t \*counts_out, void \*stream\);", hdr)
    assert re.search(r"int mrhip_get_channel_states\(mrhip_filter \*f, mrhip_channel_state \*out /\* \[nchannels\] \*/\);", hdr)
    assert re.search(r"int mrhip_set_channel_states\(mrhip_filter \*f, const int64_t \*inputDeficit, const double \*phiAccumulator\);", hdr)
    assert re.search(r"typedef struct \{ double rate, delta, phiAccumulator, alpha;\s*int64_t phiIdx, inputDeficit, xIdx, last_count; \} mrhip_channel_state;", hdr)
    assert "Per-channel rates for FIRArbitrary" in hdr
    assert "arb_rates_generic and arb_rates_tiled" in hdr                    # said at mrhip_last_kernel_name
    import ctypes as C
    assert C.sizeof(pkg.ChannelState) == 64 and [n for n, _ in pkg.ChannelState._fields_] == \
        ["rate", "delta", "phiAccumulator", "alpha", "phiIdx", "inputDeficit", "xIdx", "last_count"]
    # no new string literal of the suffixed form in the sources: the two names are reported without it
    src = open(os.path.join(CSRC, "kernels_rates_arb.hip")).read()
    assert '"arb_rates_generic"' in src and '"arb_rates_tiled"' in src and not re.search(r'"[a-z_]+_kernel"', src)


def test_argument_errors_of_the_python_constructor(pkg):
    h = np.ones(8, dtype=np.float32)
    for bad in ([0.0], [1.0, -2.0], [1.0, 0.0, 2.0], [float("nan")], [float("inf")]):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates(h, bad)                          # "rate must be greater than 0", Filters.jl:184, anywhere in rates
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates(h, [])                               # len(rates) == 0
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates(h, [[1.0, 2.0]])                     # not a vector
    assert e.value.code == 1
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates(h.astype(ct), [1.5])             # complex taps: left out
        assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates(np.ones(0, dtype=np.float32), [1.5])
    assert e.value.code == 1


def test_the_unbound_filter_describes_its_channels(pkg):
    h = np.arange(30, dtype=np.float64)
    f = pkg.FIRFilter.per_channel_rates(h, [0.47, 1.0, 2.123], 4)
    assert f.kind == pkg.host.ARBITRARY and f.Nphi == 4 and f.tapsPerPhi == 8 and f.historyLen == 7 and f.numerics == pkg.NUMERICS_STRICT
    assert pkg.FIRFilter.per_channel_rates(h, [1.5]).Nphi == 32              # Nphi defaults to 32
    sts = f.channel_states
    assert [(s.rate, s.delta, s.phiAccumulator, s.alpha, s.phiIdx, s.inputDeficit, s.xIdx, s.last_count) for s in sts] == \
        [(r, 4 / r, 1.0, 0.0, 1, 1, 1, 0) for r in (0.47, 1.0, 2.123)]
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.state                                                              # ONE state: not on this filter
    assert e.value.code == 5 and "channel_states" in str(e.value)
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.set_channel_states([1, 1, 1], [1.0, 1.0, 1.0])                     # needs a bound filter
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError):
        pkg.FIRFilter(h, 1.5).channel_states                                 # not a filter of per_channel_rates


def test_the_older_constructors_keep_their_answers(pkg):
    h = np.ones(8, dtype=np.float32)
    H = np.ones((3, 8), dtype=np.complex64)
    for rate in (-1.5, 0.0):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter(h, rate)
        assert e.value.code == 1
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_arbitrary(H.real.astype(np.float32), rate)
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter(H[0], 1.5)                                             # complex taps: complex_taps_arbitrary
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_arbitrary(H, 1.5)                          # complex taps: not through this constructor
    assert e.value.code == 5
    one = pkg.FIRFilter(h, 2.123, 4)
    st = one.state
    assert (st.kind, st.Nphi, st.tapsPerPhi, st.historyLen, st.rate, st.delta) == (4, 4, 2, 1, 2.123, 4 / 2.123)
    assert one._rates is None and pkg.FIRFilter.per_channel_arbitrary(H.real.astype(np.float32), 1.5)._rates is None


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_arb\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_rates_arb\.hip\.o.*:.*\bsched_step\.h\b", mk, flags=re.M)      # rebuilt when the shared step changes
    assert re.search(r"^.*kernels_schedule\.hip\.o.*:.*\bsched_step\.h\b", mk, flags=re.M)
    src = open(os.path.join(CSRC, "kernels_rates_arb.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src and '#include "sched_step.h"' in src and "RealTaps<TX, R, NCX, FUSED>" in src
    assert "sched_step_nb<POW2>(acc, x, step)" in src and "stage_window(" in src and "tile_run(" in src and "shiftin_by_last_workgroup" in src
    assert "asm" not in src                                                  # plain HIP
    assert not re.search(r"\bwhile\s*\([^)]*atomic", src) and "__hip_atomic" not in src          # no waits between workgroups, no spin loops
    step = open(os.path.join(CSRC, "sched_step.h")).read()
    assert "sched_step_nb" in step and "#pragma clang fp contract(off)" in step
    sched = open(os.path.join(CSRC, "kernels_schedule.hip")).read()
    assert '#include "sched_step.h"' in sched and "void sched_step_nb" not in sched             # ONE text of the step


def test_rates_kernels_use_no_scratch(pkg):
    obj = os.path.join(CSRC, "build", "kernels_rates_arb.hip.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in ("kernels_rates_arb.hip", "variant_device.h", "ctaps_device.h", "sched_step.h", "rates_arb.h"))
    if os.path.getmtime(obj) < newest:
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel in ("arb_rates_generic_kernel", "arb_rates_tiled_kernel"):       # 12 with BANK false and 12 with BANK true, none spilling
        _assert_rates_filter_kernel(sizes, kernel)
    for kernel, count in (("rates_schedule_kernel", 2), ("rates_reset_kernel", 1)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"


def test_the_row_checker_of_the_gpu_module_finds_a_stray_element():
    """a self-test of the write-only-own-outputs checker that tests/test_gpu_rates_arb.py applies to the two filter kernels: numpy
    buffers, no project code (the one new test that does not need the feature)"""
    from output_bounds_cases import POISON
    from test_gpu_rates_arb import _assert_rows_only_written
    back = np.full((5, 12), POISON * 0x01010101, dtype=np.uint32).view(np.float32)
    want = [np.arange(2, dtype=np.float32), np.zeros(0, dtype=np.float32), np.arange(3, dtype=np.float32) + 5]
    for c, w in enumerate(want):
        back[1 + c, 1:1 + len(w)] = w
    _assert_rows_only_written(back, 3, 9, 1, 2, [2, 0, 3], want, "clean")
    for r, col in ((0, 3), (2, 1), (1, 3), (3, 0), (4, 11), (3, 4)):      # guard rows, a row without outputs, behind a count, in front of a row
        bad = back.copy()
        bad[r, col] = 1.0
        with pytest.raises(AssertionError, match="outside its outputs"):
            _assert_rows_only_written(bad, 3, 9, 1, 2, [2, 0, 3], want, "stray")


# ---- the serial walk over the shared step header -----------------------------------------------------------------------------------
X_LEN = 1500
STEP_RATES = [0.01, 0.47, 1.0, 2.123, 32.0 / 3, math.pi / 3]
STEP_NPHI = [3, 4, 32]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}


def _chunks(n, how):
    if how is None:
        return [n]
    if isinstance(how, int):
        return [min(how, n - a) for a in range(0, n, how)]
    return list(how) + [n - sum(how)]


def _bits(v):
    return np.array([v], dtype=np.float64).view(np.uint64)[0]


def test_the_shared_step_walks_the_oracles_schedule(O, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rates_step_check")
    b = subprocess.run([cxx, "-std=c++20", "-O2", "-ffp-contract=off", "-w", "-I" + CSRC, os.path.join(ROOT, "tests", "rates_step_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows = [(Nphi, rate, _chunks(X_LEN, how)) for Nphi in STEP_NPHI for rate in STEP_RATES for how in CHUNKINGS.values()]
    text = "".join(f"{Nphi} {rate!r} {len(ch)} " + " ".join(map(str, ch)) + "\n" for Nphi, rate, ch in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-500:], p.stderr[-2000:])
    lines = p.stdout.strip().splitlines()
    assert len(lines) == sum(len(ch) for _, _, ch in rows)
    at = 0
    some_empty = some_short = False
    for Nphi, rate, ch in rows:
        ref = O.FIRFilter(np.ones(Nphi, dtype=np.float32), float(rate), Nphi, tx=np.float32)       # (one tap per phase: the schedule alone)
        for n in ch:
            y, sc = ref.filt(np.zeros(n, dtype=np.float32), return_schedule=True)
            v = [int(t) for t in lines[at].split()]
            at += 1
            what = (Nphi, rate, ch, n)
            count, deficit, xIdx, acc_bits = v[:4]
            st = ref.state
            assert count == len(y) == len(sc), what                                               # the count of every call
            assert (deficit, xIdx, acc_bits) == (st.inputDeficit, st.xIdx, _bits(st.phiAccumulator)), what    # the end state, in every bit
            acc = np.array(v[5::2], dtype=np.uint64).view(np.float64)
            assert np.array_equal(np.array(v[4::2], dtype=np.int64), sc["xIdx"]), what            # the entries
            assert np.array_equal(np.floor(acc).astype(np.int64), sc["phiIdx"]), what
            assert np.array_equal((acc - np.floor(acc)).view(np.uint64), np.ascontiguousarray(sc["alpha"]).view(np.uint64)), what
            assert (st.phiIdx, _bits(st.alpha)) == (int(math.floor(st.phiAccumulator)), _bits(st.phiAccumulator - math.floor(st.phiAccumulator))), what
            some_empty = some_empty or (count == 0 and n > 0)
            some_short = some_short or n == 0
    assert at == len(lines) and some_empty and some_short                   # (a call that only reduces the deficit; an empty call)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
# a row: x_f64 r_f64 complex_x complex_h bank Nphi T n_out nch rate_min num_cus mode
XF64, RF64, CX, CH, BANK, NPHI, T, NOUT, NCH, RATE, CUS, MODE = range(12)
# the default rule (mode -1) by the row's bank key, (from tiles, up to tiles a channel): the measured rows the tiled kernel won with
# shared taps and with a bank per channel (item 21)
RULE = {0: (225_024, 879), 1: (225_024, 879)}


def _expected(r):
    """the plan from its stated formulas, for either bank key: ONE pfb and dpfb in LDS (the shared pair, or one channel's),
    (2 Nphi (T+1) sizeof(R) + 15)/16*16 bytes, at most 78 KiB together with the samples; the samples take 40 KiB or what is left, in
    whole 16-byte units; one channel a lane; the span ceil(255/rate_min) + T + 2, cut to the room only when forced; a tile is 256
    outputs of one channel, the tiling goes by n_out (the call's bound); the default rule (mode -1) is the measured one of the row's
    bank key: from 225 024 tiles, up to 879 tiles a channel"""
    refused = [0] * 10
    min_tiles, max_per_channel = RULE[r[BANK]]
    if r[MODE] == 0 or r[CH] or r[NOUT] < 1 or r[T] < 1 or r[NPHI] < 1 or not r[RATE] > 0.0:
        return refused
    sample = (8 if r[XF64] else 4) * (2 if r[CX] else 1)
    tap = 8 if r[RF64] else 4
    pitch = r[T] + 1
    fixed = (2 * r[NPHI] * pitch * tap + 15) // 16 * 16
    if fixed > 78 * KB:
        return refused
    room = min(40 * KB, 78 * KB - fixed) // 16 * 16
    per_tile = math.ceil(255 / r[RATE]) + r[T] + 2
    span = min(room // sample, per_tile)
    if span < r[T] + 1:                                                     # not even one window
        return refused
    if per_tile > span and r[MODE] != 1:                                    # a cut span: only when forced
        return refused
    tpc = -(-r[NOUT] // 256)
    if r[MODE] != 1 and (tpc * r[NCH] < min_tiles or tpc > max_per_channel):
        return refused
    return [1, 1, pitch, r[NPHI] * pitch, fixed, span, 256, tpc, tpc * r[NCH], fixed + span * sample]


def _rows():
    rows, why = [], []
    for xf64, rf64 in ((0, 0), (0, 1), (1, 1)):
        for cx in (0, 1):
            for cus in (8, 256):
                base = [xf64, rf64, cx, 0, 0, 32, 8, 40_000, 33, 2.123, cus]
                for mode in (-1, 0, 1):
                    rows.append(base + [mode]), why.append("the span the slowest rate asks for" if mode == 1 else f"mode {mode}")
                    rows.append(base[:RATE] + [0.01, cus, mode]), why.append("cut span")
                    rows.append(base[:NOUT] + [257, 1, 2.123, cus, mode]), why.append("two tiles")
                    rows.append(base[:NOUT] + [225_002, 256, 2.0, cus, mode]), why.append("the smallest measured win")     # 879 x 256 tiles
                    rows.append(base[:NOUT] + [225_002, 255, 2.0, cus, mode]), why.append("a channel fewer")
                    rows.append(base[:NOUT] + [225_025, 4096, 2.0, cus, mode]), why.append("a tile a channel more")          # 880 a channel
                    rows.append(base[:NOUT] + [22_502, 4096, 2.0, cus, mode]), why.append("many short channels")            # 88 x 4096 tiles
                    rows.append(base[:NPHI] + [128 if rf64 else 256, 38, 5000, 3, 2.123, cus, mode]), why.append("not even one window")
                for change, name in (({NOUT: 0}, "n_out < 1"), ({T: 0}, "T < 1"), ({NPHI: 0}, "Nphi < 1"), ({RATE: 0.0}, "rate <= 0"),
                                     ({RATE: -1.0}, "rate <= 0"), ({CH: 1}, "complex taps"), ({BANK: 1}, "a bank"),
                                     ({NPHI: 32, T: 32}, "Nphi 32 x T 32"), ({NPHI: 512, T: 40}, "over 78 KiB")):
                    row = base + [1]
                    for k, v in change.items():
                        row[k] = v
                    rows.append(row), why.append(name)
    return rows, why


def test_the_plan_of_the_tiled_kernel(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "arb_rates_plan_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "arb_rates_plan_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows, why = _rows()
    want = [_expected(r) for r in rows]
    named = lambda name: [(r, w) for r, w, n in zip(rows, want, why) if n == name]
    # the rows reach every return, the default rule from both sides of both of its limits
    assert all(w[0] == (r[MODE] != 0) for r, w in named("the smallest measured win") + named("many short channels"))
    assert all(w[8] == 225_024 and w[7] == 879 for _, w in named("the smallest measured win") if w[0])
    assert all(w[0] == (r[MODE] == 1) for r, w in named("a channel fewer") + named("a tile a channel more"))
    for name in ("mode 0", "mode -1", "n_out < 1", "T < 1", "Nphi < 1", "rate <= 0", "complex taps", "over 78 KiB", "not even one window"):
        assert named(name) and all(not w[0] for _, w in named(name)), name
    # a bank key is no refusal: the plan of the per-channel-taps kernel, whose LDS geometry is the shared pair's
    assert named("a bank") and all(r[BANK] and w == _expected(r[:BANK] + [0] + r[BANK + 1:]) and w[0] for r, w in named("a bank"))
    assert all(w[0] == (r[MODE] == 1) for r, w in zip(rows, want) if (r, w) in named("cut span") + named("two tiles"))
    assert all(w[0] and w[5] == math.ceil(255 / 2.123) + 8 + 2 == 131 for _, w in named("the span the slowest rate asks for"))
    assert all(w[5] == 40 * KB // ((8 if r[XF64] else 4) * (2 if r[CX] else 1)) < 25_510 for r, w in named("cut span") if w[0])
    assert all(w[7] == 2 and w[8] == 2 for _, w in named("two tiles") if w[0])
    # the (32, 1024) bank of the GPU tests: 2 * 32 * 33 taps, 8448 or 16896 bytes, and the whole 40 KiB for the samples
    assert all(w[0] and w[4] == (16_896 if r[RF64] else 8_448) and w[5] == 121 + 32 + 2 for r, w in named("Nphi 32 x T 32"))
    text = "".join(" ".join(repr(v) if i == RATE else str(v) for i, v in enumerate(r)) + "\n" for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    have = [[int(v) for v in line.split()] for line in p.stdout.strip().splitlines()]
    assert len(have) == len(rows)
    differing = [(n, r, h, w) for n, r, h, w in zip(why, rows, have, want) if h != w]
    assert not differing, differing[:5]
