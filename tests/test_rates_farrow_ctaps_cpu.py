"""CPU-only checks of complex per-channel taps on the FIRFarrow filter with per-channel rates (mrhip_set_channel_ctaps_farrow,
mrhip_set_channel_pnfb_ctaps, mrhip_set_channel_pnfb_ctaps_device; FIRFilter.set_channel_ctaps_farrow, .set_channel_pnfb_ctaps,
.set_channel_pnfb_ctaps_device, .per_channel_complex_taps_and_rates_farrow; csrc/kernels_rates_farrow_ctaps.hip): the three exported
symbols, their declarations and their place in host.ABI and in the Julia shim; the constructor table that stays at sixteen; the build
conditions of the kernel unit; the instantiations in the object the build made (both filter kernels for (Tx scalar, R) in {(f32,f32),
(f32,f64), (f64,f64)} x real / complex samples = 6 each, none with scratch memory or AccVGPRs, the sibling units' counts unchanged);
through a stand-alone program built by the host compiler with -ffp-contract=off and -fsanitize=address,undefined the argument checks
(check_channel_ctaps_farrow) against a table of (arguments -> status, message), the multi kernel's plan
(plan_farrow_rates_ctaps_multi), its live-slot rule and its grid against values computed here from their stated formulas, and the
banks of mrhip_set_channel_ctaps_farrow against the one-channel fit, bit for bit; and the refusals and mirrors of the Python methods on
unbound filters."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _assert_rates_filter_kernel, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "kernels_rates_farrow_ctaps.hip"
SYMBOLS = ("mrhip_set_channel_ctaps_farrow", "mrhip_set_channel_pnfb_ctaps", "mrhip_set_channel_pnfb_ctaps_device")
THREADS = 256


def _opl():
    """the multi kernel's outputs a lane: the constant of csrc/rates_arb.h (4 or 2 by the compiled kernels' registers and the
    measurement: DESIGN.md 5.24)"""
    m = re.search(r"^constexpr int kFarrowRatesCtapsOPL = (\d+);", open(os.path.join(CSRC, "rates_arb.h")).read(), flags=re.M)
    assert m and int(m.group(1)) in (2, 4)
    return int(m.group(1))


def test_the_library_exports_the_three_symbols_and_the_header_declares_them(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len([1 for n, _, _ in pkg.host.ABI if n == name]) == 1, name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int mrhip_set_channel_ctaps_farrow(mrhip_filter *f, const void *h /* [nchannels][hLen] (re, im) */, int64_t hLen, int tap_dtype);" in flat
    assert ("int mrhip_set_channel_pnfb_ctaps(mrhip_filter *f, const double *pnfb /* [nchannels][tapsPerPhi][polyorder+1] (re, im) Float64 */, "
            "int64_t tapsPerPhi, int64_t polyorder);") in flat
    assert ("int mrhip_set_channel_pnfb_ctaps_device(mrhip_filter *f, const double *pnfb /* DEVICE, same layout */, int64_t tapsPerPhi, "
            "int64_t polyorder, void *stream);") in flat
    assert "Complex per-channel taps with per-channel rates for FIRFarrow" in hdr
    # the quoted messages of the refusals that stay, and the one the new state brings
    assert "complex taps with per-channel rates for FIRFarrow are left out" in hdr and "going back to real taps is left out" in hdr
    section = hdr.split("/* Complex per-channel taps with per-channel rates for FIRFarrow")[1].split("*/")[0]
    for left_out in ("the FIRFarrow fit on the device", "one shared complex bank", "going back to real taps", "a FUSED form", "lengths on the device",
                     "graph capture, rings, cascades and sharding", "the parallel schedule for long channels"):
        assert left_out in re.sub(r"\s+\*\s+", " ", section), left_out
    assert "farrow_rates_ctaps_generic" in section and "farrow_rates_ctaps_multi" in section
    assert "MRHIP_FARROW_RATES_CTAPS_MULTI" in section and "MRHIP_FARROW_RATES_CTAPS_GRID" in section
    assert len(set(re.findall(r"^int (mrhip_create_\w+)\(", hdr, flags=re.M))) == 16          # three calls, not a seventeenth constructor
    assert len([1 for n, _, _ in pkg.host.ABI if n.startswith("mrhip_create_")]) == 16
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    for name in SYMBOLS:
        assert len(re.findall(rf":{name}\b", jl)) == 1, name
    for fn in ("set_channel_ctaps_farrow!", "set_channel_pnfb_ctaps!", "set_channel_pnfb_ctaps_device!"):
        assert f"function {fn}(f::RatesFIRFilter" in jl and re.search(rf"^export(.|\n)*?\b{re.escape(fn)}", jl, flags=re.M), fn


def test_the_unit_is_in_the_makefile_with_its_siblings_flags_and_dependencies():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_farrow_ctaps\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    dep = re.search(r"^.*kernels_rates_farrow_ctaps\.hip\.o.*:(.*)$", mk, flags=re.M)
    assert dep and all(re.search(rf"\b{h}\b", dep.group(1)) for h in (r"variant_device\.h", r"ctaps_device\.h", r"rates_arb\.h"))
    assert not [line for line in mk.splitlines() if "kernels_rates_farrow_ctaps" in line and "EXTRA" in line]      # no flag of its own
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src and '#include "rates_arb.h"' in src and "ComplexTaps<TX, R, NCX>" in src
    assert "A::template farrow_tap<PP>(" in src and "farrow_coef_t" in src and "kFarrowBankUnrolledP" in src
    assert "tile_run(" in src and "bank_tile<true>(" in src and "farrow_rates_ctaps_live_slots(" in src and "kFarrowRatesCtapsOPL" in src
    assert "asm" not in src                                                  # plain HIP
    assert "atomic" not in src.lower()                                       # no atomics: no workgroup waits for another, no spin loop
    assert "__shared__" not in src and "__syncthreads" not in src            # no LDS, no barrier
    assert '"farrow_rates_ctaps_generic"' in src and '"farrow_rates_ctaps_multi"' in src
    assert not re.search(r'"[a-z_]+_kernel"', src)
    assert '"MRHIP_FARROW_RATES_CTAPS_MULTI", -1' in src and '"MRHIP_FARROW_RATES_CTAPS_GRID", 0' in src
    # both filter kernels end with the epilogue, ragged and plain, and no return stands in front of it
    assert src.count("shiftin_by_last_workgroup") == 2 and src.count("shiftin_ragged_by_last_workgroup") == 2
    for kernel in ("farrow_rates_ctaps_generic_kernel(FarrowArgs a, RatesArgs r)", "farrow_rates_ctaps_multi_kernel(FarrowArgs a, RatesArgs r, ArbTileArgs ta)"):
        body = src.split(kernel)[1].split("dev::shiftin_by_last_workgroup")[0]
        assert "dev::shiftin_ragged_by_last_workgroup" in body and not re.search(r"\breturn;", body), kernel
        assert "n < a.seam_below" in body and "r.rec[ch].count" in body, kernel
    # the sibling unit keeps refusing a complex-tap key, and rates_call decides before the schedule kernel moves the state
    sib = open(os.path.join(CSRC, "kernels_rates_farrow.hip")).read()
    assert "if (tk.complex_h || a.dyn) return hipErrorInvalidValue;" in sib and "if (tk.complex_h) return hipErrorInvalidValue;" in sib and "ctaps" not in sib
    api = open(os.path.join(CSRC, "api.hip")).read()
    calls = api.split("static int rates_call(")[1].split("\nint mrhip_filt_device_rates(")[0]
    assert calls.index("plan_farrow_rates_ctaps_multi(") < calls.index("prepare_farrow_rates_ctaps_multi(") < calls.index("launch_rates_schedule(") \
        < calls.index("launch_farrow_rates_ctaps_multi(") < calls.index("launch_farrow_rates_ctaps_generic(") < calls.index("launch_arb_rates_ctaps_tiled(")
    assert api.count("launch_rates_pnfb_install(") == 2                      # the device install reuses the one kernel
    logic = open(os.path.join(CSRC, "host_logic.cpp")).read()
    assert "Refusal check_channel_ctaps_farrow(" in logic and "bool plan_farrow_rates_ctaps_multi(" in logic
    assert logic.index("Refusal check_channel_ctaps(") < logic.index("Refusal check_channel_taps_farrow(") < logic.index("Refusal check_channel_ctaps_farrow(")


def _built(unit, *headers):
    obj = os.path.join(CSRC, "build", unit + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, s)) for s in (unit,) + headers):
        pytest.skip("object older than its source")
    return obj


def test_the_unit_holds_the_instantiations_the_dispatcher_reaches_and_none_spills(pkg):
    sizes = _kernel_scratch(_built(UNIT, "variant_device.h", "ctaps_device.h", "rates_arb.h"))
    assert all("farrow_rates_ctaps_" in k for k in sizes), sorted(sizes)     # nothing else in the unit
    for kernel in ("farrow_rates_ctaps_generic_kernel", "farrow_rates_ctaps_multi_kernel"):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        # dispatch_variant: (Tx scalar, R) in {(f, f), (f, d), (d, d)} x NCX in {1, 2}
        want = {f"I{tx}{r}Li{ncx}E" for tx, r in ("ff", "fd", "dd") for ncx in (1, 2)}
        got = {re.search(r"kernelI(\w\wLi\dE)", k).group(1) for k in mine}
        assert len(mine) == 6 and got == {w[1:] for w in want}, (kernel, sorted(mine))
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"
    multi = [k for k in sizes if "farrow_rates_ctaps_multi_kernel" in k]
    assert all(re.search(rf"Li[12]ELi{_opl()}EEEv", k) for k in multi), multi  # ONE slot count, the constant's


def test_the_sibling_units_keep_their_instantiations(pkg):
    sizes = _kernel_scratch(_built("kernels_rates_farrow.hip", "variant_device.h", "ctaps_device.h", "rates_arb.h"))
    _assert_rates_filter_kernel(sizes, "farrow_rates_generic_kernel")
    _assert_rates_filter_kernel(sizes, "farrow_rates_multi_kernel")
    assert not [k for k in sizes if "ctaps" in k]
    arb = _kernel_scratch(_built("kernels_rates_arb_ctaps.hip", "variant_device.h", "ctaps_device.h", "rates_arb.h"))
    for kernel, count in (("arb_rates_ctaps_generic_kernel", 6), ("arb_rates_ctaps_tiled_kernel", 6), ("rates_cbank_build_kernel", 3)):
        assert len([k for k in arb if kernel in k]) == count, kernel
    build = _kernel_scratch(_built("kernels_rates_bank_build.hip", "rates_arb.h"))
    assert len([k for k in build if "rates_pnfb_install_kernel" in k]) == 2   # Float32 and Float64 taps: no second install kernel


# ---- the argument checks, the plan and the banks, through one stand-alone program -----------------------------------------------------
F32, F64, C64, C128 = range(4)
TAPS, PNFB, PNFB_DEV = range(3)
NAMES = ("mrhip_set_channel_ctaps_farrow", "mrhip_set_channel_pnfb_ctaps", "mrhip_set_channel_pnfb_ctaps_device")
POINTS_TO_ARB = "a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_ctaps"
TAKES = " takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb"
# (which, is_rates, is_farrow, src_is_null, len, polyorder, tap_dtype, filter_len, filter_polyorder, filter_tap_dtype, fused)
#   -> (status, pieces of the message): the header's contract, in its order -- the filter, then h / pnfb, the lengths, (taps only) the
#   tap dtype, the numerics
CHECK_TABLE = [
    ((TAPS, 1, 1, 0, 250, 4, C64, 250, 4, F32, 0), (0, ())),
    ((TAPS, 1, 1, 0, 250, 4, C128, 250, 4, F64, 0), (0, ())),
    ((TAPS, 1, 1, 0, 250, 4, C64, 250, 4, C64, 0), (0, ())),                  # a later call: the filter's tap type is complex already
    ((TAPS, 1, 1, 0, 250, 4, C128, 250, 4, C128, 0), (0, ())),
    ((PNFB, 1, 1, 0, 8, 4, -7, 8, 4, F32, 0), (0, ())),                      # (the pnfb calls take no dtype: it is not looked at)
    ((PNFB, 1, 1, 0, 8, 4, F32, 8, 4, C64, 0), (0, ())),
    ((PNFB_DEV, 1, 1, 0, 1, 0, F64, 1, 0, F64, 0), (0, ())),
    ((PNFB_DEV, 1, 1, 0, 32, 6, C128, 32, 6, C128, 0), (0, ())),
    # the filter kind goes first, whatever else is wrong
    ((TAPS, 1, 0, 0, 250, 4, C64, 250, 4, F32, 0), (1, (NAMES[TAPS] + ": ", POINTS_TO_ARB))),
    ((TAPS, 1, 0, 1, 3, 4, F32, 250, 4, F32, 1), (1, (NAMES[TAPS] + ": ", POINTS_TO_ARB))),
    ((PNFB, 1, 0, 1, 3, 1, F32, 8, 4, F32, 1), (1, (NAMES[PNFB] + ": ", POINTS_TO_ARB))),
    ((PNFB_DEV, 1, 0, 0, 8, 4, F32, 8, 4, F32, 0), (1, (NAMES[PNFB_DEV] + ": ", POINTS_TO_ARB))),
    ((TAPS, 0, 1, 0, 250, 4, C64, 250, 4, F32, 0), (1, (NAMES[TAPS] + TAKES,))),
    ((TAPS, 0, 0, 1, 3, 4, F32, 250, 4, F32, 1), (1, (NAMES[TAPS] + TAKES,))),
    ((PNFB, 0, 1, 0, 8, 4, F32, 8, 4, C64, 0), (1, (NAMES[PNFB] + TAKES,))),
    ((PNFB_DEV, 0, 0, 1, 8, 4, F32, 8, 4, F32, 1), (1, (NAMES[PNFB_DEV] + TAKES,))),
    # NULL before the lengths before the dtype before the numerics
    ((TAPS, 1, 1, 1, 249, 4, 7, 250, 4, F32, 1), (1, (NAMES[TAPS] + ": h is NULL",))),
    ((PNFB, 1, 1, 1, 7, 3, F32, 8, 4, F32, 1), (1, (NAMES[PNFB] + ": pnfb is NULL",))),
    ((PNFB_DEV, 1, 1, 1, 8, 4, F32, 8, 4, F32, 0), (1, (NAMES[PNFB_DEV] + ": pnfb is NULL",))),
    ((TAPS, 1, 1, 0, 249, 4, 7, 250, 4, F32, 1), (1, (NAMES[TAPS] + ": hLen must be the filter's (250 taps a channel; got 249)",))),
    ((TAPS, 1, 1, 0, 251, 4, C64, 250, 4, F32, 0), (1, (NAMES[TAPS] + ": hLen",))),
    ((TAPS, 1, 1, 0, 0, 4, C64, 250, 4, F32, 0), (1, (NAMES[TAPS] + ": hLen",))),
    ((PNFB, 1, 1, 0, 7, 4, F32, 8, 4, F32, 1), (1, (NAMES[PNFB] + ": tapsPerPhi and polyorder must be the filter's (8 polynomials of order 4 a channel; got 7 of order 4)",))),
    ((PNFB, 1, 1, 0, 8, 3, F32, 8, 4, F32, 0), (1, (NAMES[PNFB] + ": tapsPerPhi and polyorder", "got 8 of order 3"))),
    ((PNFB_DEV, 1, 1, 0, 9, 4, F32, 8, 4, C64, 1), (1, (NAMES[PNFB_DEV] + ": tapsPerPhi and polyorder",))),
    ((PNFB_DEV, 1, 1, 0, 8, 5, F32, 8, 4, F32, 0), (1, (NAMES[PNFB_DEV] + ": tapsPerPhi and polyorder",))),
    ((TAPS, 1, 1, 0, 250, 4, -1, 250, 4, F32, 0), (1, (NAMES[TAPS] + ": bad tap dtype",))),
    ((TAPS, 1, 1, 0, 250, 4, 4, 250, 4, F32, 1), (1, (NAMES[TAPS] + ": bad tap dtype",))),
    ((TAPS, 1, 1, 0, 250, 4, F32, 250, 4, F32, 0), (1, (NAMES[TAPS] + ":", "(real taps go through mrhip_set_channel_taps_farrow)"))),
    ((TAPS, 1, 1, 0, 250, 4, F64, 250, 4, F32, 1), (1, (NAMES[TAPS] + ":", "(real taps go through mrhip_set_channel_taps_farrow)"))),
    ((TAPS, 1, 1, 0, 250, 4, F64, 250, 4, C128, 0), (1, (NAMES[TAPS] + ":", "(real taps go through mrhip_set_channel_taps_farrow)"))),
    ((TAPS, 1, 1, 0, 250, 4, C128, 250, 4, F32, 0), (1, (NAMES[TAPS] + ":", "the complex type of the filter's tap precision"))),
    ((TAPS, 1, 1, 0, 250, 4, C64, 250, 4, F64, 1), (1, (NAMES[TAPS] + ":", "the complex type of the filter's tap precision"))),
    ((TAPS, 1, 1, 0, 250, 4, C128, 250, 4, C64, 0), (1, (NAMES[TAPS] + ":", "the complex type of the filter's tap precision"))),
    ((TAPS, 1, 1, 0, 250, 4, C64, 250, 4, F32, 1), (5, (NAMES[TAPS] + ":", "FUSED"))),
    ((TAPS, 1, 1, 0, 250, 4, C128, 250, 4, F64, 1), (5, (NAMES[TAPS] + ":", "FUSED"))),
    ((PNFB, 1, 1, 0, 8, 4, F32, 8, 4, F32, 1), (5, (NAMES[PNFB] + ":", "FUSED"))),
    ((PNFB_DEV, 1, 1, 0, 8, 4, F64, 8, 4, F64, 1), (5, (NAMES[PNFB_DEV] + ":", "FUSED"))),
]

# a plan row: x_f64 r_f64 complex_x complex_h bank T polyorder n_out nch num_cus mode
XF64, RF64, CX, CH, BANK, T_, P_, NOUT, NCH, CUS, MODE = range(11)
RULE = (90_112, 22)      # the default rule (mode -1), (from tiles, up to tiles a channel): the measured rows the multi kernel won


def _expected_plan(r, opl):
    """the plan from its stated formulas: a tile is ONE channel and opl runs of 256 outputs, the tiling goes by n_out (the call's
    bound); mode 0 never, 1 every call, -1 the default rule"""
    if r[MODE] == 0 or not r[CH] or not r[BANK] or r[NOUT] < 1 or r[T_] < 1 or r[P_] < 0 or r[NCH] < 1:
        return [0, 0, 0, 0, 0]
    tile = opl * THREADS
    tpc = -(-r[NOUT] // tile)
    if r[MODE] != 1 and (RULE is None or tpc * r[NCH] < RULE[0] or tpc > RULE[1]):
        return [0, 0, 0, 0, 0]
    return [1, 1, tile, tpc, tpc * r[NCH]]


def _plan_rows(opl):
    rows, why = [], []
    tile = opl * THREADS
    for xf64, rf64 in ((0, 0), (0, 1), (1, 1)):
        for cx in (0, 1):
            base = [xf64, rf64, cx, 1, 1, 8, 4, 22_502, 4096, 256]
            for mode in (-1, 0, 1):
                rows.append(base + [mode]), why.append(f"mode {mode}")
                for n_out, name in ((1, "one output"), (tile, "a full tile"), (tile + 1, "a tile and one")):
                    rows.append(base[:NOUT] + [n_out, 3, 256, mode]), why.append(name)
                rows.append(base[:NCH] + [RULE[0] // RULE[1] - 1, 256, mode]), why.append("a channel fewer")            # both sides of both limits
                rows.append(base[:NOUT] + [RULE[1] * tile + 1, 4096, 256, mode]), why.append("a tile a channel more")
                rows.append(base[:NOUT] + [225_002, 256, 256, mode]), why.append("the measured row that did not win")    # 256 ch x 1e5
                rows.append(base[:NOUT] + [2_250_002, 64, 256, mode]), why.append("the serial walk")                     # 64 ch x 1e6
            for change, name in (({NOUT: 0}, "n_out < 1"), ({T_: 0}, "T < 1"), ({P_: -1}, "polyorder < 0"), ({NCH: 0}, "nch < 1"), ({CH: 0}, "real taps"),
                                 ({BANK: 0}, "no bank"), ({CH: 0, BANK: 0}, "real shared taps"), ({P_: 0}, "polyorder 0"), ({T_: 1}, "T 1")):
                row = base + [1]
                for k, v in change.items():
                    row[k] = v
                rows.append(row), why.append(name)
    return rows, why


def _live(k0, tid, count, opl):
    """slot j of lane tid is output k0 + tid + 256 j: the slots in front of the count, which are the first ones"""
    return sum(1 for j in range(opl) if k0 + tid + THREADS * j < count)


BANKS = [(4, 4, 1), (4, 30, 3), (3, 40, 2), (32, 250, 4), (32, 250, 6), (32, 1024, 4), (5, 33, 2)]       # (Nphi, hLen, polyorder)


def test_the_argument_checks_the_plan_and_the_banks(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    opl = _opl()
    exe = str(tmp_path / "farrow_rates_ctaps_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, os.path.join(ROOT, "tests", "farrow_rates_ctaps_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows, why = _plan_rows(opl)
    want = [_expected_plan(r, opl) for r in rows]
    named = lambda name: [(r, w) for r, w, n in zip(rows, want, why) if n == name]
    tile = opl * THREADS
    for name in ("mode 0", "n_out < 1", "T < 1", "polyorder < 0", "nch < 1", "real taps", "no bank", "real shared taps"):
        assert named(name) and all(not w[0] for _, w in named(name)), name
    # the switch values: 0 never, 1 every call, -1 the rule -- the measured row it takes (4096 ch x 1e4: 22 tiles a channel, 90 112 tiles)
    # and, from both sides of both of its limits, the calls it leaves
    assert opl == 4 and all(w[0] == (r[MODE] != 0) and (not w[0] or w[3:] == [22, 90_112]) for r, w in named("mode -1") + named("mode 1"))
    for name in ("one output", "a full tile", "a tile and one", "a channel fewer", "a tile a channel more", "the measured row that did not win", "the serial walk"):
        assert named(name) and all(w[0] == (r[MODE] == 1) for r, w in named(name)), name
    assert all(w[3:] == [22, 90_090] for _, w in named("a channel fewer") if w[0]) and all(w[3:] == [23, 23 * 4096] for _, w in named("a tile a channel more") if w[0])
    assert all(w[3:] == [220, 56_320] for _, w in named("the measured row that did not win") if w[0]) and all(w[3:] == [2198, 140_672] for _, w in named("the serial walk") if w[0])
    assert all(w == [1, 1, tile, -(-22_502 // tile), -(-22_502 // tile) * 4096] for _, w in named("mode 1"))      # a tile is one channel
    assert all(w[2:] == [tile, 1, 3] for _, w in named("one output") + named("a full tile") if w[0])
    assert all(w[2:] == [tile, 2, 6] for _, w in named("a tile and one") if w[0])
    assert all(w[0] for _, w in named("polyorder 0") + named("T 1"))
    # the live slots at the edges of a tile and of a channel's count
    lives = [(k0, tid, count) for k0 in (0, tile, 7 * tile) for tid in (0, 1, 127, 255)
             for count in (0, 1, k0, k0 + 1, k0 + 255, k0 + 256, k0 + 257, k0 + tile - 256, k0 + tile - 1, k0 + tile, k0 + tile + 1, k0 + 3 * tile, 1 << 40)]
    assert {_live(*a, opl) for a in lives} == set(range(opl + 1))
    grids = [(10, 256, 0), (10_000, 256, 0), (0, 256, 0), (10, 256, 3), (10, 256, 2000), (10, 256, 100_000), (1, 0, 0)]
    text = "".join("plan " + " ".join(map(str, r)) + "\n" for r in rows)
    text += "".join("live " + " ".join(map(str, a)) + "\n" for a in lives)
    text += "".join("grid " + " ".join(map(str, a)) + "\n" for a in grids)
    text += "".join("check " + " ".join(map(str, args)) + "\n" for args, _ in CHECK_TABLE)
    text += "".join(f"banks {Nphi} {hLen} {P} {f64}\n" for Nphi, hLen, P in BANKS for f64 in (0, 1))
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)      # run directly: no preloaded runtime
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows) + len(lives) + len(grids) + len(CHECK_TABLE) + 2 * len(BANKS)
    have = [[int(v) for v in line.split()] for line in lines[:len(rows)]]
    differing = [(n, r, h, w) for n, r, h, w in zip(why, rows, have, want) if h != w]
    assert not differing, differing[:5]
    at = len(rows)
    for a, line in zip(lives, lines[at:]):
        assert int(line) == _live(*a, opl), (a, line)
    at += len(lives)
    for (total, chip, fixed), line in zip(grids, lines[at:]):
        assert int(line) == (min(fixed, 65535) if fixed > 0 else max(min(chip, total), 1)), (total, chip, fixed, line)
    at += len(grids)
    for (args, (status, pieces)), line in zip(CHECK_TABLE, lines[at:]):
        got_status, _, message = line.partition(" ")
        assert int(got_status) == status, (args, line)
        assert all(piece in message for piece in pieces) if status else message == "", (args, line)
        assert not status or re.match(re.escape(NAMES[args[0]]) + r"[: ]", message), (args, line)          # each message names the function
    at += len(CHECK_TABLE)
    for Nphi, hLen, P in BANKS:
        for f64 in (0, 1):
            Tp, ok, bad_rows, bad_comp = (int(v) for v in lines[at].split())
            at += 1
            assert (Tp, ok, bad_rows, bad_comp) == (-(-hLen // Nphi), 1, 0, 0), (Nphi, hLen, P, f64, lines[at - 1])


# ---- the Python methods on unbound filters ----------------------------------------------------------------------------------------
def _mirrors(f):
    m = f._chan_farrow
    return (None if m is None else (m[0], m[1].tobytes()), f._farrow_ctaps, None if f._chan_ctaps is None else f._chan_ctaps.tobytes(),
            f._rates.tobytes(), f.h.tobytes(), f._handle, f.numerics, f._tap_dtype)


def test_refusals_of_the_python_methods_on_unbound_filters_change_no_mirror(pkg):
    h = np.ones(8, dtype=np.float32)
    rng = np.random.default_rng(5)
    Hc = (rng.standard_normal((3, 8)) + 1j * rng.standard_normal((3, 8))).astype(np.complex64)
    PN = (rng.standard_normal((3, 2, 3)) + 1j * rng.standard_normal((3, 2, 3)))       # Nphi 4: T = 2; polyorder 2
    rates = [0.47, 1.0, 2.123]
    f = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)
    assert f._chan_farrow is None and not f._farrow_ctaps and f.output_dtype is None and f._tap_dtype == np.float32
    for filt in (f, pkg.FIRFilter.per_channel_taps_and_rates_farrow(Hc.real.copy(), rates, 4, 2)):
        before = _mirrors(filt)
        for bad in (Hc[:2], Hc[:, :7], Hc[0], Hc.reshape(3, 2, 4), Hc.real.copy(), Hc.astype(np.complex128)):
            with pytest.raises(pkg.MultirateHIPError) as e:
                filt.set_channel_ctaps_farrow(bad)
            assert e.value.code == 1, bad.shape
            assert _mirrors(filt) == before                                  # a refused call changes no mirror
        for bad in (PN[:2], PN[:, :1], PN[:, :, :2], PN[0], PN.real.copy()):
            with pytest.raises(pkg.MultirateHIPError) as e:
                filt.set_channel_pnfb_ctaps(bad)
            assert e.value.code == 1, bad.shape
            assert _mirrors(filt) == before
        with pytest.raises(pkg.MultirateHIPError) as e:
            filt.set_channel_pnfb_ctaps_device(PN)                           # not a device tensor (and the filter is not bound)
        assert e.value.code == 1 and _mirrors(filt) == before
    calls = lambda g: ((g.set_channel_ctaps_farrow, Hc), (g.set_channel_pnfb_ctaps, PN), (g.set_channel_pnfb_ctaps_device, PN))
    for other in (pkg.FIRFilter(h, 1.5, 4, 2), pkg.FIRFilter.per_channel_farrow(Hc.real.copy(), 1.5, 4, 2), pkg.FIRFilter.complex_taps_farrow(Hc[0], 1.5, 4, 2),
                  pkg.FIRFilter.per_channel_rates(h, rates, 4)):
        for call, arg in calls(other):
            with pytest.raises(pkg.MultirateHIPError) as e:
                call(arg)                                                    # not a filter of per_channel_rates_farrow
            assert e.value.code == 1 and other._chan_farrow is None and not other._farrow_ctaps
            if other._rates is not None:
                assert "takes set_channel_ctaps" in str(e.value)             # the FIRArbitrary filter is pointed to its own call
    fused = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2, numerics=pkg.NUMERICS_FUSED)
    for call, arg in calls(fused)[:2]:
        with pytest.raises(pkg.MultirateHIPError) as e:
            call(arg)                                                        # complex taps have no FUSED form
        assert e.value.code == 5 and "FUSED" in str(e.value) and fused._chan_farrow is None and not fused._farrow_ctaps
    with pytest.raises(pkg.MultirateHIPError) as e:
        fused.set_channel_ctaps_farrow(Hc[:2])                               # (the matrix is looked at first)
    assert e.value.code == 1
    # the install is remembered (whichever call came last), the taps may change, and going back is refused
    f.set_channel_ctaps_farrow(Hc)
    assert f._chan_farrow[0] == "ctaps" and np.array_equal(f._chan_farrow[1], Hc) and f._chan_farrow[1] is not Hc and f._farrow_ctaps
    assert f._handle is None and np.array_equal(f.h, h) and f._tap_dtype == np.complex64
    f.set_channel_pnfb_ctaps(PN)
    assert f._chan_farrow[0] == "cpnfb" and np.array_equal(f._chan_farrow[1], PN) and f._chan_farrow[1].dtype == np.complex128
    f.set_channel_ctaps_farrow(Hc[::-1])
    assert f._chan_farrow[0] == "ctaps" and np.array_equal(f._chan_farrow[1], Hc[::-1])
    before = _mirrors(f)
    for call, arg in ((f.set_channel_taps_farrow, Hc.real.copy()), (f.set_channel_pnfb, PN.real.copy())):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call(arg)
        assert e.value.code == 5 and "going back to real taps is left out" in str(e.value) and _mirrors(f) == before
    # what the entry points answered to complex taps before, they still answer, word for word
    g = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)
    with pytest.raises(pkg.MultirateHIPError) as e:
        g.set_channel_ctaps(Hc)
    assert e.value.code == 5 and "set_channel_ctaps: complex taps with per-channel rates for FIRFarrow are left out" in str(e.value)
    with pytest.raises(pkg.MultirateHIPError) as e:
        g.set_channel_ctaps_device(Hc)
    assert e.value.code == 5 and "complex taps with per-channel rates for FIRFarrow are left out" in str(e.value)
    with pytest.raises(pkg.MultirateHIPError) as e:
        g.set_channel_taps_farrow(Hc)
    assert e.value.code == 5 and "complex taps with per-channel rates are left out" in str(e.value)
    with pytest.raises(pkg.MultirateHIPError) as e:
        g.set_channel_pnfb(PN)
    assert e.value.code == 5 and "complex taps with per-channel rates are left out" in str(e.value)
    assert g._chan_farrow is None and not g._farrow_ctaps and g._chan_ctaps is None
    for ctor in (lambda: pkg.FIRFilter.per_channel_rates_farrow(Hc[0], rates, 4, 2), lambda: pkg.FIRFilter.per_channel_taps_and_rates_farrow(Hc, rates, 4, 2)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            ctor()
        assert e.value.code == 5 and "complex taps with per-channel rates are left out" in str(e.value)


def test_per_channel_complex_taps_and_rates_farrow_unbound(pkg):
    rng = np.random.default_rng(6)
    rates = [0.47, 1.0, 2.123]
    for ct, rt in ((np.complex64, np.float32), (np.complex128, np.float64)):
        H = (rng.standard_normal((3, 30)) + 1j * rng.standard_normal((3, 30))).astype(ct)
        g = pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(H, rates, 4, 3)
        assert g.kind == pkg.host.FARROW and g.Nphi == 4 and g.polyorder == 3 and g.tapsPerPhi == 8 and g.historyLen == 7 and g._handle is None
        assert g.h.dtype == rt and np.array_equal(g.h, H[0].real) and len(g.h) == 30       # the placeholder: real(H[0]), same length and precision
        assert g._chan_farrow[0] == "ctaps" and np.array_equal(g._chan_farrow[1], H) and g._chan_farrow[1] is not H and g._farrow_ctaps
        assert g._chan_ctaps is None and g._chan_taps is None and g._bank is None
        assert np.array_equal(g._rates, rates) and g.rate == 2.123 and g._tap_dtype == ct
        assert [(s.rate, s.phiAccumulator, s.inputDeficit) for s in g.channel_states] == [(r, 1.0, 1) for r in rates]
        for tx, ty in ((np.float32, ct), (np.complex64, ct), (np.float64, np.complex128), (np.complex128, np.complex128)):
            g._tx = np.dtype(tx)
            assert g.output_dtype == np.dtype(ty), (ct, tx)                  # complex, also over real samples
        g._tx = None
        PN = rng.standard_normal((3, 8, 4)) + 1j * rng.standard_normal((3, 8, 4))
        p = pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(H, rates, 4, 3, pnfb=PN)
        assert p._chan_farrow[0] == "cpnfb" and np.array_equal(p._chan_farrow[1], PN) and p._farrow_ctaps and p._tap_dtype == ct and p.h.dtype == rt
    assert pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(H, rates).Nphi == 32
    for bad_H, bad_rates, kw in ((H, rates[:2], {}), (H[0], rates, {}), (H, [1.0, 0.0, 2.0], {}), (H, [], {}), (H.real.copy(), rates, {}),
                                 (np.ones((3, 0), dtype=np.complex64), rates, {}), (H, rates, {"pnfb": PN.real.copy()}), (H, rates, {"pnfb": PN[0]}),
                                 (H, rates, {"pnfb": PN[:2]})):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(bad_H, bad_rates, 4, 3, **kw)
        assert e.value.code == 1, (bad_H.shape, bad_rates, list(kw))
