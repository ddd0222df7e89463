"""CPU-only checks of per-channel complex taps for FIRArbitrary (FIRFilter.per_channel_complex_taps_arbitrary,
mrhip_create_arbitrary_bank_ctaps, csrc/kernels_bank_arb_ctaps.hip): the argument errors of the Python constructor, the refusals the
older constructors keep, the description of the unbound filter, the exported symbol and its declaration, the build conditions of the
kernel unit, the instantiations in the objects the build made (both new kernels for (Tx scalar, R) in {(f32,f32), (f32,f64),
(f64,f64)} x real / complex samples = 6 each, and the 12 + 12 of kernels_bank_arb.hip, the unit the new one was modelled on; none with
scratch memory or AccVGPRs), and the tiled kernel's plan (csrc/host_logic.cpp: plan_arb_bank_ctaps_tiled) through a
stand-alone program built by the host compiler with -fsanitize=address,undefined, against values computed here from the plan's
stated formulas."""
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = 1024


def test_argument_errors_of_the_python_constructor(pkg):
    H = np.ones((3, 8), dtype=np.complex64)
    for bad in (H[0], np.ones((2, 3, 4), dtype=np.complex64), np.ones((0, 4), dtype=np.complex64), np.ones((2, 0), dtype=np.complex64)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_arbitrary(bad, 1.5)     # not a (nchannels >= 1, hLen >= 1) matrix
        assert e.value.code == 1
    for rt in (np.float32, np.float64):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_arbitrary(H.real.astype(rt), 1.5)   # real taps: per_channel_arbitrary
        assert e.value.code == 1 and "per_channel_arbitrary" in str(e.value)
    for rate in (Fraction(3, 2), 2, (3, 2)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, rate)      # a ratio: per_channel_complex_taps
        assert e.value.code == 1 and "per_channel_complex_taps" in str(e.value)
    for rate in (-1.5, 0.0):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, rate)      # "rate must be greater than 0", Filters.jl:184
        assert e.value.code == 1
    with pytest.raises(TypeError):
        pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, 1.5, numerics=pkg.NUMERICS_FUSED)   # there is no numerics argument


def test_the_older_constructors_keep_their_refusals(pkg):
    H = np.ones((3, 8), dtype=np.complex64)
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_arbitrary(H.astype(ct), 1.5)         # complex taps: not through this constructor
        assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(H.real.astype(np.float32), 1.5)          # a float rate: not the rational family
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(H, 2)                                    # complex taps: per_channel_complex_taps
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps(H, 1.5)                     # a float rate: not the rational family
    assert e.value.code == 5


def test_the_unbound_filter_describes_one_channels_filter(pkg):
    H = (np.arange(3 * 30).reshape(3, 30) * (1 - 2j)).astype(np.complex128)
    f = pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, 2.123, 4)
    one = pkg.FIRFilter.complex_taps_arbitrary(H[0], 2.123, 4)
    st = f.state
    assert f.kind == one.kind == pkg.host.ARBITRARY and f.kernel_name == one.kernel_name
    assert (st.kind, st.Nphi, st.hLen, st.tapsPerPhi, st.historyLen) == (4, 4, 30, 8, 7)             # tapsPerPhi = ceil(hLen / Nphi)
    assert (st.rate, st.delta, st.phiAccumulator, st.inputDeficit, st.phiIdx, st.alpha, st.xIdx) == (2.123, 4 / 2.123, 1.0, 1, 1, 0.0, 1)
    assert f.numerics == pkg.NUMERICS_STRICT
    assert pkg.FIRFilter.per_channel_complex_taps_arbitrary(H.astype(np.complex64), 0.47).Nphi == 32     # Nphi defaults to 32
    assert np.array_equal(f._bank, H) and f._bank is not H and f._bank.dtype == np.complex128          # copied, in the tap type
    assert np.array_equal(f.h, H[0])


def test_the_library_exports_the_constructor_and_the_header_declares_it(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "mrhip_create_arbitrary_bank_ctaps")
    rows = [(res, args) for name, res, args in pkg.host.ABI if name == "mrhip_create_arbitrary_bank_ctaps"]
    same = [(res, args) for name, res, args in pkg.host.ABI if name == "mrhip_create_arbitrary_bank"]
    assert len(rows) == 1 and rows == same                                  # the signature of its real-tap neighbour
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(os.path.dirname(CSRC), "..", "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_create_arbitrary_bank_ctaps\(const void \*h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,\s*"
                     r"int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)
    assert "Per-channel complex taps for FIRArbitrary" in hdr


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_bank_arb_ctaps\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_bank_arb_ctaps\.hip\.o.*:\s*ctaps_device\.h\s*$", mk, flags=re.M)   # rebuilt when the shared arithmetic changes
    src = open(os.path.join(CSRC, "kernels_bank_arb_ctaps.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src and "ComplexTaps<TX, R, NCX>" in src
    assert "arb_variant_generic_body<ComplexTaps<TX, R, NCX>, true>" in src and "arb_variant_bank_tiled_body<ComplexTaps<TX, R, NCX>>" in src
    assert "asm" not in src                                                  # plain HIP
    shared = open(os.path.join(CSRC, "variant_device.h")).read()
    assert "#pragma clang fp contract(off)" in shared and "arb_variant_bank_tiled_body" in shared


def _scratch_of(src):
    obj = os.path.join(CSRC, "build", src + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in (src, "variant_device.h", "ctaps_device.h"))
    if os.path.getmtime(obj) < newest:
        pytest.skip("object older than its source")
    return _kernel_scratch(obj)


def test_arb_bank_ctaps_kernels_use_no_scratch(pkg):
    sizes = _scratch_of("kernels_bank_arb_ctaps.hip")
    for kernel, count in (("arb_bank_ctaps_generic_kernel", 6), ("arb_bank_ctaps_tiled_kernel", 6)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"


def test_the_real_tap_unit_keeps_its_instantiations_without_scratch(pkg):
    sizes = _scratch_of("kernels_bank_arb.hip")
    for kernel, count in (("arb_bank_generic_kernel", 12), ("arb_bank_tiled_kernel", 12)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"


# ---- the plan ------------------------------------------------------------------------------------------------------------------
# a row: x_f64 r_f64 complex_x complex_h bank Nphi T n_out nch rate num_cus mode
XF64, RF64, CX, CH, BANK, NPHI, T, NOUT, NCH, RATE, CUS, MODE = range(12)


def _default_rule(total_tiles, num_cus):
    """mode -1, the measured rule: from 20 tiles per CU -- 5312 tiles on 256 CUs was the smallest measured call
    at which the tiled kernel beat the universal one by more than the spread of the repeats, 664 tiles the largest at which it did not"""
    return total_tiles >= 20 * num_cus


def _expected(r):
    """the plan from its stated formulas: both banks of one channel in pairs, (2 Nphi (T+1) 2 sizeof(R) + 15)/16*16 bytes, at most
    78 KiB together with the samples; the samples take 40 KiB or what is left, in whole 16-byte units; one channel a lane; the span
    ceil(255/rate) + T + 2, cut to the room only when forced; a tile is 256 outputs of one channel"""
    refused = [0] * 10
    if r[MODE] == 0 or not r[BANK] or not r[CH] or r[NOUT] < 1 or r[T] < 1 or r[NPHI] < 1 or not r[RATE] > 0.0:
        return refused
    sample = (8 if r[XF64] else 4) * (2 if r[CX] else 1)
    pair = 2 * (8 if r[RF64] else 4)
    pitch = r[T] + 1
    fixed = (2 * r[NPHI] * pitch * pair + 15) // 16 * 16
    if fixed > 78 * KB:
        return refused
    room = min(40 * KB, 78 * KB - fixed) // 16 * 16
    per_tile = math.ceil(255 / r[RATE]) + r[T] + 2
    span = room // sample
    cut = per_tile > span
    if not cut:
        span = per_tile
    if span < r[T] + 1:                                                     # not even one window
        return refused
    if cut and r[MODE] != 1:
        return refused
    tpc = -(-r[NOUT] // 256)
    if r[MODE] != 1 and not _default_rule(tpc * r[NCH], r[CUS]):
        return refused
    return [1, 1, pitch, r[NPHI] * pitch, fixed, span, 256, tpc, tpc * r[NCH], fixed + span * sample]


def _rows():
    rows, why = [], []
    for xf64, rf64 in ((0, 0), (0, 1), (1, 1)):
        for cx in (0, 1):
            for cus in (8, 256):
                base = [xf64, rf64, cx, 1, 1, 32, 8, 40_000, 33, 2.123, cus]
                edge = 39 if rf64 else 78                                   # Nphi x 64 pairs: both banks are 78 KiB exactly, no room left
                for mode in (-1, 0, 1):
                    rows.append(base + [mode]), why.append("the span the rate asks for" if mode == 1 else f"mode {mode}")
                    slow = base[:RATE] + [1.0 / 50, cus, mode]
                    rows.append(slow), why.append("cut span")
                    rows.append(base[:NOUT] + [256 * 20 * cus, 1, 2.123, cus, mode]), why.append("twenty tiles a CU")
                    rows.append(base[:NOUT] + [256 * (20 * cus - 8), 1, 2.123, cus, mode]), why.append("eight tiles fewer")
                    rows.append(base[:NOUT] + [256 * 5 * cus - 255, 4, 2.123, cus, mode]), why.append("twenty tiles a CU")   # (a ragged last tile; 4 channels)
                    rows.append(base[:NOUT] + [256 * 5 * cus - 256, 4, 2.123, cus, mode]), why.append("eight tiles fewer")   # (20 cus - 4 tiles)
                    rows.append(base[:NPHI] + [edge, 63, 5000, 3, 2.123, cus, mode]), why.append("not even one window")
                for change, name in (({NOUT: 0}, "n_out < 1"), ({T: 0}, "T < 1"), ({NPHI: 0}, "Nphi < 1"), ({RATE: 0.0}, "rate <= 0"),
                                     ({RATE: -1.0}, "rate <= 0"), ({CH: 0}, "real taps"), ({BANK: 0}, "not a bank"),
                                     ({NPHI: 64, T: 32}, "Nphi 64 x T 32"), ({NPHI: 128, T: 40}, "over 78 KiB")):
                    row = base + [1]
                    for k, v in change.items():
                        row[k] = v
                    rows.append(row), why.append(name)
    return rows, why


def test_the_plan_of_the_tiled_kernel(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "arb_bank_ctaps_plan_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "arb_bank_ctaps_plan_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows, why = _rows()
    want = [_expected(r) for r in rows]
    # the rows reach every return, from both sides where there are two
    named = lambda name: [(r, w) for r, w, n in zip(rows, want, why) if n == name]
    for name in ("mode 0", "n_out < 1", "T < 1", "Nphi < 1", "rate <= 0", "real taps", "not a bank", "over 78 KiB", "not even one window"):
        assert named(name) and all(not w[0] for _, w in named(name)), name
    assert all(r[MODE] == 1 or not w[0] for r, w in named("not even one window"))                    # forced and refused
    assert all(w[0] and w[5] == math.ceil(255 / 2.123) + 8 + 2 == 131 for _, w in named("the span the rate asks for"))
    assert all(w[0] == (r[MODE] == 1) for r, w in named("cut span"))                                # the cut span: only when forced
    assert all(w[5] == 40 * KB // ((8 if r[XF64] else 4) * (2 if r[CX] else 1)) < 12_750 for r, w in named("cut span") if w[0])
    # Nphi 64 x T 32: both banks in pairs of Float64 are 2 * 64 * 33 * 16 bytes = 66 KiB, under the 78 KiB, so that bank is planned
    # (12 KiB are left for its samples); the bank that is over is Nphi 128 x T 40 (82 KiB in pairs of Float32)
    assert all(w[0] and w[4] == (67_584 if r[RF64] else 33_792) and w[5] == 121 + 32 + 2 for r, w in named("Nphi 64 x T 32"))
    # the default rule from both sides, on both chips: taken at exactly 20 tiles a CU, refused just below (and taken there when forced)
    assert all(w[0] == (r[MODE] != 0) and (not w[0] or w[8] == 20 * r[CUS]) for r, w in named("twenty tiles a CU"))
    assert all(w[0] == (r[MODE] == 1) and (not w[0] or 20 * r[CUS] - 8 <= w[8] < 20 * r[CUS]) for r, w in named("eight tiles fewer"))
    assert {(r[CUS], r[MODE]) for r, w in named("twenty tiles a CU") if w[0]} == {(8, -1), (8, 1), (256, -1), (256, 1)}
    text = "".join(" ".join(repr(v) if i == RATE else str(v) for i, v in enumerate(r)) + "\n" for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    have = [[int(v) for v in line.split()] for line in p.stdout.strip().splitlines()]
    assert len(have) == len(rows)
    differing = [(n, r, h, w) for n, r, h, w in zip(why, rows, have, want) if h != w]
    assert not differing, differing[:5]
