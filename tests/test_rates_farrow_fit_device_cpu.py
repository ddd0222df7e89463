"""CPU-only checks of the FIRFarrow fit on the device (mrhip_set_channel_taps_farrow_device, mrhip_set_channel_ctaps_farrow_device;
FIRFilter.set_channel_taps_farrow_device / .set_channel_ctaps_farrow_device; csrc/kernels_rates_farrow_fit.hip): through a stand-alone
program built with -fsanitize=address,undefined, polyfit_factor + polyfit_apply (the text the kernel compiles) against the untouched
polyfit_rows byte for byte, the rows the kernel's lanes read against taps2pfb, every lane of the kernel restated over a guard-padded
buffer (each word of the banks written once, nothing outside them), the launch plan on both sides of every boundary and the
pure argument checks of both calls against tables of (arguments -> status, message); the exported symbols, their declarations and their
places in host.ABI and in the Julia shim; the constructor table that stays at sixteen; the build conditions of the new unit and the
four instantiations in the object the build made, none with scratch memory; what the Python methods refuse without a GPU, and that a
refused call changes no mirror."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "kernels_rates_farrow_fit.hip"
SYMBOLS = ("mrhip_set_channel_taps_farrow_device", "mrhip_set_channel_ctaps_farrow_device")
SECTION = "The FIRFarrow fit on the device for the filters with per-channel rates"
# (Nphi, polyorder): constant and linear fits, m = n (exact interpolation), an odd Nphi, the measured shape, a high order, and one shape on
# the far side of each plan boundary; then what polyfit_rows refuses (n < m)
FITS = [(4, 0), (4, 1), (4, 3), (3, 2), (32, 4), (32, 7), (160, 3), (512, 4), (1024, 4)]
REFUSED_FITS = [(4, 4), (3, 5), (1, 1)]
ROWS = 200
MAPS = [(4, 4), (4, 30), (3, 40), (32, 250), (32, 1024)]      # (Nphi, hLen) of tests/test_gpu_rates_farrow.py (a GPU module: not imported here)
# (Nphi, hLen, polyorder, nch): every lane of the kernel restated on the host over a guard-padded buffer -- T = 1; zero padding and m = n; the
# division path; the measured shape with several waves and a partial last one; fewer lanes a workgroup (32, and 8 at the bound)
LANES = [(4, 4, 1, 3), (4, 30, 3, 67), (3, 40, 2, 67), (32, 250, 4, 67), (32, 1024, 4, 3), (160, 320, 3, 67), (1024, 2048, 4, 3)]
# Nphi -> (lanes, LDS bytes), None: refused.  64 lanes while 64 columns of Nphi Float64 fit 64 KiB, then the largest power of two, down to 8
PLANS = [(1, (64, 512)), (32, (64, 16384)), (128, (64, 65536)), (129, (32, 33024)), (160, (32, 40960)), (256, (32, 65536)), (257, (16, 32896)),
         (512, (16, 65536)), (513, (8, 32832)), (1024, (8, 65536)), (1025, None), (4096, None), (0, None), (-3, None)]

F32, F64, C64, C128 = range(4)
WHO_T, WHO_C = SYMBOLS
# (is_rates, is_farrow, h_is_null, hLen, tap_dtype, filter_hLen, filter_tap_dtype) -> (status, a piece of the message): the checks of
# mrhip_set_channel_taps_farrow, in its order, in the new name
TAPS_TABLE = [
    ((1, 1, 0, 250, F32, 250, F32), (0, "")),
    ((1, 1, 0, 250, F64, 250, F64), (0, "")),
    ((1, 0, 0, 250, F32, 250, F32), (1, WHO_T + ": a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_taps_device")),
    ((1, 0, 1, 3, C64, 250, F32), (1, "takes mrhip_set_channel_taps_device")),               # (the kind goes first)
    ((0, 1, 0, 250, F32, 250, F32), (1, WHO_T + " takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb")),
    ((0, 0, 0, 250, F32, 250, F32), (1, WHO_T + " takes a filter of mrhip_create_farrow_rates")),
    ((1, 1, 1, 250, F32, 250, F32), (1, WHO_T + ": h is NULL")),
    ((1, 1, 1, 249, C64, 250, F32), (1, "h is NULL")),
    ((1, 1, 0, 249, F32, 250, F32), (1, WHO_T + ": hLen must be the filter's (250 taps a channel; got 249)")),
    ((1, 1, 0, 249, 7, 250, F32), (1, "hLen must be the filter's")),
    ((1, 1, 0, 250, 4, 250, F32), (1, WHO_T + ": bad tap dtype")),
    ((1, 1, 0, 250, -1, 250, F32), (1, "bad tap dtype")),
    ((1, 1, 0, 250, C64, 250, F32), (5, WHO_T + ": complex taps with per-channel rates are left out")),
    ((1, 1, 0, 250, C128, 250, F64), (5, "complex taps with per-channel rates are left out")),
    ((1, 1, 0, 250, F64, 250, F32), (1, WHO_T + ": the taps must have the filter's tap dtype")),
    ((1, 1, 0, 250, F32, 250, F64), (1, "the filter's tap dtype")),
]
# (..., fused): the checks of mrhip_set_channel_ctaps_farrow, in its order, in the new name; the filter's tap dtype may be real or complex
CTAPS_TABLE = [
    ((1, 1, 0, 250, C64, 250, F32, 0), (0, "")),
    ((1, 1, 0, 250, C128, 250, F64, 0), (0, "")),
    ((1, 1, 0, 250, C64, 250, C64, 0), (0, "")),                                            # (a later call: the filter is complex already)
    ((1, 1, 0, 250, C128, 250, C128, 0), (0, "")),
    ((1, 0, 0, 250, C64, 250, F32, 0), (1, WHO_C + ": a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_ctaps_device")),
    ((1, 0, 1, 3, F32, 250, F32, 1), (1, "takes mrhip_set_channel_ctaps_device")),
    ((0, 1, 0, 250, C64, 250, F32, 0), (1, WHO_C + " takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb")),
    ((0, 0, 0, 250, C64, 250, F32, 0), (1, WHO_C + " takes a filter of mrhip_create_farrow_rates")),
    ((1, 1, 1, 250, C64, 250, F32, 0), (1, WHO_C + ": h is NULL")),
    ((1, 1, 0, 249, C64, 250, F32, 0), (1, WHO_C + ": hLen must be the filter's (250 taps a channel; got 249)")),
    ((1, 1, 0, 250, 4, 250, F32, 0), (1, WHO_C + ": bad tap dtype")),
    ((1, 1, 0, 250, F32, 250, F32, 0), (1, WHO_C + ": the taps must be Complex64 or Complex128 (real taps go through mrhip_set_channel_taps_farrow_device)")),
    ((1, 1, 0, 250, F64, 250, F64, 1), (1, "real taps go through mrhip_set_channel_taps_farrow_device")),
    ((1, 1, 0, 250, C128, 250, F32, 0), (1, WHO_C + ": the taps must be the complex type of the filter's tap precision")),
    ((1, 1, 0, 250, C64, 250, C128, 0), (1, "the complex type of the filter's tap precision")),
    ((1, 1, 0, 250, C64, 250, F32, 1), (5, WHO_C + ": the filter is in FUSED numerics and no FUSED form is defined for complex taps")),
    ((1, 1, 0, 249, C64, 250, F32, 1), (1, "hLen must be the filter's")),                   # (the argument errors first)
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """one build and one run of the stand-alone program for the whole module: {kind: [lines]} in the order of the tables above"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("fit") / "rates_farrow_fit_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "rates_farrow_fit_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows = [("fit", (n, p, ROWS)) for n, p in FITS + REFUSED_FITS]
    rows += [("map", (n, hLen, cplx)) for n, hLen in MAPS for cplx in (0, 1)]
    rows += [("lanes", shape + (cplx,)) for shape in LANES for cplx in (0, 1)]
    rows += [("plan", (n,)) for n, _ in PLANS]
    rows += [("taps", args) for args, _ in TAPS_TABLE] + [("ctaps", args) for args, _ in CTAPS_TABLE]
    text = "".join(kind + " " + " ".join(map(str, args)) + "\n" for kind, args in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows)
    out = {}
    for (kind, _), line in zip(rows, lines):
        out.setdefault(kind, []).append(line)
    return out


def test_factor_and_apply_are_polyfit_rows_byte_for_byte(answers):
    lines = answers["fit"]
    for (n, p), line in zip(FITS, lines):
        factored, refused, tested, bad, bad_in_place = map(int, line.split())
        assert (factored, refused, tested) == (1, 0, 4 * ROWS), (n, p, line)              # every kind of row was fitted by both
        assert (bad, bad_in_place) == (0, 0), (n, p, line)
    for (n, p), line in zip(REFUSED_FITS, lines[len(FITS):]):                               # n < m: polyfit_factor refuses exactly there
        factored, refused, tested, bad, bad_in_place = map(int, line.split())
        assert (factored, refused, tested) == (0, 4 * ROWS, 4 * ROWS), (n, p, line)
    assert all(n >= p + 1 for n, p in FITS) and all(n < p + 1 for n, p in REFUSED_FITS) and (4, 3) in FITS


def test_the_rows_the_lanes_read_are_taps2pfb_rows(answers):
    maps = [(n, hLen, cplx) for n, hLen in MAPS for cplx in (0, 1)]
    for (n, hLen, cplx), line in zip(maps, answers["map"]):
        T = -(-hLen // n)
        pad = (n * T - hLen) * (2 if cplx else 1) * 2                                      # (components; Float32 and Float64 taps)
        assert [int(v) for v in line.split()] == [T, 0, pad], (n, hLen, cplx, line)
    assert (-(-4 // 4), -(-30 // 4), -(-40 // 3)) == (1, 8, 14)                             # T = 1; zero padding; hLen no multiple of Nphi


def test_each_lane_writes_its_own_coefficients_and_nothing_else(answers):
    """the kernel's item map, row load, in-place fit, rounding and destination index, lane by lane on the host: the banks are those of
    create_farrow_banks after the install's rounding byte for byte, every word of the banks is written exactly once, no destination
    index lies outside them, and the poisoned words just before the first bank and just past the last one are unchanged"""
    cases = [shape + (cplx,) for shape in LANES for cplx in (0, 1)]
    for (n, hLen, p, nch, cplx), line in zip(cases, answers["lanes"]):
        T = -(-hLen // n)
        words = nch * T * (p + 1) * (2 if cplx else 1) * 2                                  # (Float32 and Float64 taps)
        assert [int(v) for v in line.split()] == [words, 0, 0, 0, 0], (n, hLen, p, nch, cplx, line)
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "farrow_fit_item(item, a.T, NC)" in src and "a.pnfb[farrow_fit_dst_index(it, k, a.T, a.m, NC)]" in src      # the kernel runs that text
    assert src.count("a.pnfb") == 1                                                          # ... and stores nowhere else


def test_the_launch_plan_on_both_sides_of_every_boundary(answers):
    for (n, want), line in zip(PLANS, answers["plan"]):
        ok, lanes, lds = map(int, line.split())
        assert (ok, lanes, lds) == ((1,) + want if want else (0, 0, 0)), (n, line)
        if want:
            assert lds == lanes * n * 8 <= 64 * 1024 and 8 <= lanes <= 64                  # two workgroups a CU
            assert lanes == 64 or 2 * lanes * n * 8 > 64 * 1024                            # ... and no fewer lanes than fit
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read().split(SECTION)[1]
    assert "Nphi up to 1024" in hdr                                                         # the bound is stated where the caller reads


def test_the_argument_checks(answers):
    for kind, table in (("taps", TAPS_TABLE), ("ctaps", CTAPS_TABLE)):
        for (args, (status, piece)), line in zip(table, answers[kind]):
            got_status, _, message = line.partition(" ")
            assert int(got_status) == status, (args, line)
            assert (piece in message) if status else message == "", (args, line)


def test_the_library_exports_the_two_symbols_and_the_header_declares_them(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len([1 for n, _, _ in pkg.host.ABI if n == name]) == 1, name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    c = r"(?: /\*[^*]*\*/)?"
    assert re.search(r"int mrhip_set_channel_taps_farrow_device\(mrhip_filter \*f, const void \*h" + c + r", int64_t hLen, int tap_dtype, void \*stream\);", hdr)
    assert re.search(r"int mrhip_set_channel_ctaps_farrow_device\(mrhip_filter \*f, const void \*h" + c + r", int64_t hLen, int tap_dtype,\s+void \*stream\);", hdr)
    block = re.sub(r"\s*\n \*\s+", " ", hdr.split(SECTION)[1].split("int mrhip_set_channel_taps_farrow_device")[0])      # (the comment's line breaks)
    for said in ("rank deficient", "capturing stream", "BIT FOR BIT", "mrhip_reset keeps the banks", "(polyorder+1) * (Nphi + polyorder + 2) Float64", "freed by mrhip_destroy"):
        assert said in block, said
    for left_out in ("the constructors", "graph capture", "one shared complex bank", "a FUSED form", "parallel schedule"):
        assert left_out in block, left_out
    older = hdr.split("Device-resident updates for the filters with per-channel rates")[1].split("int mrhip_set_channel_rates_device")[0]
    assert "fit on the device" in older and "mrhip_set_channel_taps_farrow_device below" in older       # kept, and "since added"
    assert len(set(re.findall(r"^int (mrhip_create_\w+)\(", hdr, flags=re.M))) == 16          # two calls, not a seventeenth constructor
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    for name in SYMBOLS:
        assert jl.count(":" + name + ",") == 1, name
        assert "function " + name[len("mrhip_"):] + "!(f::RatesFIRFilter" in jl, name


def test_the_unit_is_in_the_makefile_with_the_flags_of_its_sibling():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_farrow_fit\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_rates_farrow_fit\.hip\.o.*:.*\brates_arb\.h\b", mk, flags=re.M)
    assert not re.search(r"kernels_rates_farrow_fit\.hip\.o[^\n]*EXTRA", mk)                 # no flag of its own, as kernels_rates_bank_build.hip
    assert "fast-math" not in mk
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "#pragma clang fp contract(off)" in src and '#include "rates_arb.h"' in src
    assert "polyfit_apply(" in src and "farrow_fit_row_start(" in src                        # the shared statements, not a copy of them
    assert "asm" not in src and "atomic" not in src.lower() and "__syncthreads" not in src   # plain HIP; nobody waits for anybody
    hdr = open(os.path.join(CSRC, "rates_arb.h")).read()
    assert re.search(r"MRHIP_RATES_HD inline void polyfit_apply\(", hdr)                     # ONE text, for the kernel and the host program
    logic = open(os.path.join(CSRC, "host_logic.cpp")).read()
    assert "bool polyfit_factor(" in logic and "bool plan_rates_fit(" in logic
    asan = re.search(r"^\.\./libmultirate_host_asan\.so:.*$", mk, flags=re.M).group(0)
    assert "host_logic.cpp" in asan and "rates_arb.h" in asan and "create.h" in asan


def test_the_four_instantiations_are_in_the_object_and_use_no_scratch(pkg):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm tools")
    obj = os.path.join(CSRC, "build", UNIT + ".o")
    if not os.path.exists(obj):
        pytest.skip("no built object (the library came prebuilt)")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, s)) for s in (UNIT, "rates_arb.h")):
        pytest.skip("object older than its source")
    mine = {k: v for k, v in _kernel_scratch(obj).items() if "rates_farrow_fit_kernel" in k}
    assert len(mine) == 4, f"expected 4 instantiations of rates_farrow_fit_kernel (TAP in float, double; NC in 1, 2), found {sorted(mine)}"
    spilling = {k: v for k, v in mine.items() if v != 0}
    assert not spilling, f"instantiations with scratch or AccVGPRs: {list(spilling.items())}"


def test_what_the_python_methods_refuse_without_a_gpu(pkg):
    import torch
    h = np.ones(8, dtype=np.float32)
    H = np.arange(24, dtype=np.float32).reshape(3, 8)
    CH = (H + 1j * H[::-1]).astype(np.complex64)
    rates = [0.47, 1.0, 2.123]
    far = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)
    far_taps = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)
    far_taps.set_channel_taps_farrow(H)
    far_ctaps = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)
    far_ctaps.set_channel_ctaps_farrow(CH)
    arb = pkg.FIRFilter.per_channel_rates(h, rates, 4)
    one, bank, rational = pkg.FIRFilter(h, 1.5, 4, 2), pkg.FIRFilter.per_channel_farrow(H, 1.5, 4, 2), pkg.FIRFilter(h, Fraction(2, 3))
    calls = []
    for g in (far, far_taps, far_ctaps, arb, one, bank, rational):
        for value in (H, torch.from_numpy(H)):                                               # a host array, a CPU tensor; unbound filters
            calls.append((g, lambda g=g, v=value: g.set_channel_taps_farrow_device(v), 5 if g is far_ctaps else 1))
        for value in (CH, torch.from_numpy(CH)):
            calls.append((g, lambda g=g, v=value: g.set_channel_ctaps_farrow_device(v), 1))
    mirrors = lambda f: (None if f._rates is None else f._rates.tobytes(), f._chan_farrow if f._chan_farrow is None else (f._chan_farrow[0], f._chan_farrow[1].tobytes()),
                         f._farrow_ctaps, f.rate, f._handle)
    for f, call, code in calls:
        before = mirrors(f)
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert mirrors(f) == before                                          # a refused call changes no mirror
    with pytest.raises(pkg.MultirateHIPError, match="takes set_channel_taps_device"):
        arb.set_channel_taps_farrow_device(torch.from_numpy(H))
    with pytest.raises(pkg.MultirateHIPError, match="takes set_channel_ctaps_device"):           # (the sibling for a device tensor, as the library answers)
        arb.set_channel_ctaps_farrow_device(torch.from_numpy(CH))
    with pytest.raises(pkg.MultirateHIPError, match="going back to real taps is left out"):
        far_ctaps.set_channel_taps_farrow_device(torch.from_numpy(H))
    # the existing methods accept what they accepted, and answer a FIRFarrow filter as they did
    far.set_channel_taps_farrow(H)
    assert far._chan_farrow[0] == "taps"
    with pytest.raises(pkg.MultirateHIPError, match="takes set_channel_pnfb_device") as e:
        far.set_channel_taps_device(torch.from_numpy(H))
    assert e.value.code == 1
