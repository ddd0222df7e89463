"""CPU-only checks of complex per-channel taps on the FIRArbitrary filter with per-channel rates (mrhip_set_channel_ctaps,
mrhip_set_channel_ctaps_device, FIRFilter.set_channel_ctaps, .set_channel_ctaps_device, .per_channel_complex_taps_and_rates,
csrc/kernels_rates_arb_ctaps.hip): the two exported symbols, their declarations and their place in host.ABI and in the Julia shim; the
constructor table that stays at sixteen; the build conditions of the kernel unit; the instantiations in the object the build made (both
filter kernels for (Tx scalar, R) in {(f32,f32), (f32,f64), (f64,f64)} x real / complex samples = 6 each, the bank build kernel for
(float,float), (float,double), (double,double) = 3, none with scratch memory or AccVGPRs); through a stand-alone program built by the host
compiler with -ffp-contract=off the argument checks (check_channel_ctaps) against a table of (arguments -> status, message), the tiled
kernel's plan (plan_arb_rates_ctaps_tiled) against values computed here from the plan's stated formulas, and the pair value functions
of the bank build kernel against create_pfb_banks, bit for bit; and the refusals and mirrors of the Python methods on unbound filters."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = 1024
UNIT = "kernels_rates_arb_ctaps.hip"
SYMBOLS = ("mrhip_set_channel_ctaps", "mrhip_set_channel_ctaps_device")


def test_the_library_exports_the_two_symbols_and_the_header_declares_them(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len([1 for n, _, _ in pkg.host.ABI if n == name]) == 1, name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_set_channel_ctaps\(mrhip_filter \*f, const void \*h /\* \[nchannels\]\[hLen\] \(re, im\) \*/, int64_t hLen, int tap_dtype\);", hdr)
    assert re.search(r"int mrhip_set_channel_ctaps_device\(mrhip_filter \*f, const void \*h /\* DEVICE, same layout \*/, int64_t hLen, int tap_dtype, void \*stream\);", hdr)
    assert "Complex per-channel taps with per-channel rates for FIRArbitrary" in hdr
    assert "complex taps with per-channel rates for FIRFarrow are left out" in hdr and "going back to real taps is left out" in hdr
    last = hdr.split("const char *mrhip_last_kernel_name")[0].rsplit("/*", 1)[1]
    assert "arb_rates_ctaps_generic" in last and "arb_rates_ctaps_tiled" in last
    assert len(set(re.findall(r"^int (mrhip_create_\w+)\(", hdr, flags=re.M))) == 16          # two calls, not a seventeenth constructor
    assert len([1 for n, _, _ in pkg.host.ABI if n.startswith("mrhip_create_")]) == 16
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    assert len(re.findall(r":mrhip_set_channel_ctaps\b", jl)) == 1 and len(re.findall(r":mrhip_set_channel_ctaps_device\b", jl)) == 1
    assert "function set_channel_ctaps!(f::RatesFIRFilter" in jl and "function set_channel_ctaps_device!(f::RatesFIRFilter" in jl


def test_the_unit_is_in_the_makefile_with_its_siblings_flags_and_dependencies():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_arb_ctaps\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    dep = re.search(r"^.*kernels_rates_arb_ctaps\.hip\.o.*:(.*)$", mk, flags=re.M)
    assert dep and all(re.search(rf"\b{h}\b", dep.group(1)) for h in (r"variant_device\.h", r"ctaps_device\.h", r"rates_arb\.h"))
    assert not [line for line in mk.splitlines() if "kernels_rates_arb_ctaps" in line and "EXTRA" in line]      # no flag of its own
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src and '#include "rates_arb.h"' in src and "ComplexTaps<TX, R, NCX>" in src
    assert "stage_window(" in src and "tile_run(" in src and "tile_span(" in src and "arb_dots_global<A>" in src and "ch_in_lds" in src
    assert "bank_tile<true>(" in src and "rates_channel_len(" in src and "rates_bank_tap_index(" in src
    assert "rates_cbank_pfb_value<TAP>(" in src and "rates_cbank_dpfb_value<TAP>(" in src
    assert "asm" not in src                                                  # plain HIP
    assert "atomic" not in src.lower()                                       # no atomics: no workgroup waits for another, no spin loop
    assert '"arb_rates_ctaps_generic"' in src and '"arb_rates_ctaps_tiled"' in src
    for name in os.listdir(CSRC):                                            # no new string literal of the suffixed form under csrc
        if name.endswith((".hip", ".h", ".cpp", ".inc")):
            assert not re.search(r'"[a-z_]*(rates_ctaps|cbank)[a-z_]*_kernel"', open(os.path.join(CSRC, name)).read()), name
    assert not re.search(r'"[a-z_]+_kernel"', src)
    # both filter kernels end with the epilogue, ragged and plain, and no return stands in front of it
    assert src.count("shiftin_by_last_workgroup") == 2 and src.count("shiftin_ragged_by_last_workgroup") == 2
    for kernel in ("arb_rates_ctaps_generic_kernel(ArbArgs a, RatesArgs r)", "arb_rates_ctaps_tiled_kernel(ArbArgs a, RatesArgs r, ArbTileArgs ta)"):
        body = src.split(kernel)[1].split("dev::shiftin_by_last_workgroup")[0]
        assert "dev::shiftin_ragged_by_last_workgroup" in body and not re.search(r"\breturn;", body), kernel
    tiled = src.split("arb_rates_ctaps_tiled_kernel(ArbArgs a, RatesArgs r, ArbTileArgs ta)")[1].split("dev::shiftin_by_last_workgroup")[0]
    loop = tiled.index("for (long long tile = run.begin")
    assert loop < tiled.index("if (t.k0 >= count) continue;") < tiled.index("__syncthreads();") < tiled.index("if (ch != ch_in_lds)") < tiled.index("stage_window(")
    # the sibling unit keeps refusing a complex-tap key, and rates_call decides before the schedule kernel moves the state
    sib = open(os.path.join(CSRC, "kernels_rates_arb.hip")).read()
    assert "if (tk.complex_h || a.dyn) return hipErrorInvalidValue;" in sib and "ctaps" not in sib
    api = open(os.path.join(CSRC, "api.hip")).read()
    calls = api.split("static int rates_call(")[1].split("\nint mrhip_filt_device_rates(")[0]
    assert calls.index("plan_arb_rates_ctaps_tiled(") < calls.index("prepare_arb_rates_ctaps_tiled(") < calls.index("launch_rates_schedule(") \
        < calls.index("launch_arb_rates_ctaps_tiled(") < calls.index("launch_arb_rates_ctaps_generic(")
    logic = open(os.path.join(CSRC, "host_logic.cpp")).read()
    assert "Refusal check_channel_ctaps(" in logic and "bool plan_arb_rates_ctaps_tiled(" in logic
    assert logic.index("Refusal check_channel_taps(") < logic.index("Refusal check_channel_ctaps(") < logic.index("Refusal check_channel_taps_farrow(")


def test_rates_ctaps_kernels_use_no_scratch(pkg):
    obj = os.path.join(CSRC, "build", UNIT + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in (UNIT, "variant_device.h", "ctaps_device.h", "rates_arb.h"))
    if os.path.getmtime(obj) < newest:
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel, count in (("arb_rates_ctaps_generic_kernel", 6), ("arb_rates_ctaps_tiled_kernel", 6), ("rates_cbank_build_kernel", 3)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"


# ---- the argument checks, the plan and the bank values, through one stand-alone program --------------------------------------------------
F32, F64, C64, C128 = range(4)
OWN = "mrhip_set_channel_ctaps"
# (device, is_rates, is_farrow, h_is_null, hLen, tap_dtype, filter_hLen, filter_tap_dtype, fused) -> (status, pieces of the message): the
# header's contract, in its order -- the filter, then h, hLen, the tap dtype, the numerics
CTAPS_TABLE = [
    ((0, 1, 0, 0, 250, C64, 250, F32, 0), (0, ())),
    ((0, 1, 0, 0, 250, C128, 250, F64, 0), (0, ())),
    ((0, 1, 0, 0, 250, C64, 250, C64, 0), (0, ())),                          # a later call: the filter's tap type is complex already
    ((0, 1, 0, 0, 250, C128, 250, C128, 0), (0, ())),
    ((1, 1, 0, 0, 1, C64, 1, F32, 0), (0, ())),
    ((0, 1, 1, 0, 250, C64, 250, F32, 0), (5, (OWN + ":", "complex taps with per-channel rates for FIRFarrow are left out"))),
    ((1, 1, 1, 1, 3, F32, 250, F32, 1), (5, (OWN + "_device:", "complex taps with per-channel rates for FIRFarrow are left out"))),      # (whatever else is wrong)
    ((0, 0, 0, 0, 250, C64, 250, F32, 0), (1, (OWN + " takes a filter of mrhip_create_arbitrary_rates",))),
    ((0, 0, 1, 0, 250, C64, 250, F32, 0), (1, (OWN + " takes a filter of mrhip_create_arbitrary_rates",))),
    ((1, 0, 0, 1, 3, F32, 250, F32, 1), (1, (OWN + "_device takes a filter of mrhip_create_arbitrary_rates",))),
    ((0, 1, 0, 1, 250, C64, 250, F32, 0), (1, (OWN + ": h is NULL",))),
    ((1, 1, 0, 1, 3, F32, 250, F32, 1), (1, (OWN + "_device: h is NULL",))),
    ((0, 1, 0, 0, 249, C64, 250, F32, 0), (1, (OWN + ": hLen",))),
    ((0, 1, 0, 0, 251, C64, 250, F32, 0), (1, (OWN + ": hLen",))),
    ((0, 1, 0, 0, 0, C64, 250, F32, 0), (1, (OWN + ": hLen",))),
    ((1, 1, 0, 0, 249, F32, 250, F32, 1), (1, (OWN + "_device: hLen",))),
    ((0, 1, 0, 0, 250, -1, 250, F32, 0), (1, (OWN + ": bad tap dtype",))),
    ((0, 1, 0, 0, 250, 4, 250, F32, 1), (1, (OWN + ": bad tap dtype",))),
    ((0, 1, 0, 0, 250, F32, 250, F32, 0), (1, (OWN + ":", "mrhip_set_channel_taps)"))),
    ((0, 1, 0, 0, 250, F64, 250, F32, 1), (1, (OWN + ":", "mrhip_set_channel_taps)"))),
    ((1, 1, 0, 0, 250, F64, 250, F64, 0), (1, (OWN + "_device:", "mrhip_set_channel_taps_device)"))),
    ((0, 1, 0, 0, 250, C128, 250, F32, 0), (1, (OWN + ":", "the complex type of the filter's tap precision"))),
    ((0, 1, 0, 0, 250, C64, 250, F64, 1), (1, (OWN + ":", "the complex type of the filter's tap precision"))),
    ((0, 1, 0, 0, 250, C128, 250, C64, 0), (1, (OWN + ":", "the complex type of the filter's tap precision"))),
    ((0, 1, 0, 0, 250, C64, 250, F32, 1), (5, (OWN + ":", "FUSED"))),
    ((1, 1, 0, 0, 250, C128, 250, F64, 1), (5, (OWN + "_device:", "FUSED"))),
]

# a plan row: x_f64 r_f64 complex_x complex_h bank Nphi T n_out nch rate_min num_cus mode
XF64, RF64, CX, CH, BANK, NPHI, T, NOUT, NCH, RATE, CUS, MODE = range(12)
RULE = (225_024, 879)      # the default rule (mode -1), (from tiles, up to tiles a channel): the measured rows the tiled kernel won


def _expected(r):
    """the plan from its stated formulas: ONE channel's pfb and dpfb as (re, im) pairs of R, (2 Nphi (T+1) 2 sizeof(R) + 15)/16*16 bytes,
    at most 78 KiB together with the samples; the samples take 40 KiB or what is left, in whole 16-byte units; one channel a lane; the
    span ceil(255/rate_min) + T + 2 (the slowest channel), cut to the room only when forced; a tile is 256 outputs of one channel, the
    tiling goes by n_out (the call's bound); the default rule (mode -1) as DESIGN.md 9 item 25 derives it: from 225 024 tiles, up to 879
    tiles a channel, never with a cut span"""
    refused = [0] * 10
    if r[MODE] == 0 or not r[CH] or not r[BANK] or r[NOUT] < 1 or r[T] < 1 or r[NPHI] < 1 or not r[RATE] > 0.0:
        return refused
    sample = (8 if r[XF64] else 4) * (2 if r[CX] else 1)
    pair = 2 * (8 if r[RF64] else 4)
    pitch = r[T] + 1
    fixed = (2 * r[NPHI] * pitch * pair + 15) // 16 * 16
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
    if r[MODE] != 1 and (RULE is None or tpc * r[NCH] < RULE[0] or tpc > RULE[1]):
        return refused
    return [1, 1, pitch, r[NPHI] * pitch, fixed, span, 256, tpc, tpc * r[NCH], fixed + span * sample]


def _rows():
    rows, why = [], []
    for xf64, rf64 in ((0, 0), (0, 1), (1, 1)):
        for cx in (0, 1):
            base = [xf64, rf64, cx, 1, 1, 32, 8, 40_000, 33, 2.123, 256]
            for mode in (-1, 0, 1):
                rows.append(base + [mode]), why.append("the span the slowest rate asks for" if mode == 1 else f"mode {mode}")
                rows.append(base[:RATE] + [0.01, 256, mode]), why.append("cut span")
                rows.append(base[:NOUT] + [257, 1, 2.123, 256, mode]), why.append("two tiles")
                rows.append(base[:NOUT] + [22_502, 4096, 2.0, 256, mode]), why.append("many short channels")            # 88 x 4096 tiles
                rows.append(base[:NOUT] + [225_002, 256, 2.0, 256, mode]), why.append("the smallest measured win")      # 879 x 256 tiles
                rows.append(base[:NOUT] + [225_002, 255, 2.0, 256, mode]), why.append("a channel fewer")
                rows.append(base[:NOUT] + [225_025, 4096, 2.0, 256, mode]), why.append("a tile a channel more")          # 880 a channel
                rows.append(base[:NOUT] + [2_250_002, 64, 2.0, 256, mode]), why.append("the measured row that did not win")   # 8790 a channel
            # the 78 KiB edge: 2 Nphi (T+1) pairs; Complex64 pairs (R = Float32): Nphi 128, T 38 is 79 872 bytes = 78 KiB exactly and leaves no
            # room for a window, T 37 is 77 824 and leaves 2048; Complex128 pairs (R = Float64): Nphi 64 gives the same byte counts
            nphi = 64 if rf64 else 128
            for t, name in ((38, "78 KiB exactly"), (37, "under 78 KiB"), (39, "over 78 KiB")):
                rows.append(base[:NPHI] + [nphi, t, 5000, 3, 2.123, 256, 1]), why.append(name)
            for change, name in (({NOUT: 0}, "n_out < 1"), ({T: 0}, "T < 1"), ({NPHI: 0}, "Nphi < 1"), ({RATE: 0.0}, "rate <= 0"),
                                 ({RATE: -1.0}, "rate <= 0"), ({CH: 0}, "real taps"), ({BANK: 0}, "no bank"), ({CH: 0, BANK: 0}, "real shared taps"),
                                 ({NPHI: 32, T: 32}, "Nphi 32 x T 32")):
                row = base + [1]
                for k, v in change.items():
                    row[k] = v
                rows.append(row), why.append(name)
    return rows, why


MAPS = [(4, 4), (4, 30), (3, 40), (32, 250), (32, 1024), (1, 5), (7, 1), (5, 2)]       # (Nphi, hLen): T = 1; zero padding; Nphi no power of two; one tap


def test_the_argument_checks_the_plan_and_the_bank_values(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "arb_rates_ctaps_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "arb_rates_ctaps_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows, why = _rows()
    want = [_expected(r) for r in rows]
    named = lambda name: [(r, w) for r, w, n in zip(rows, want, why) if n == name]
    # the rows reach every return; the refusals by name
    for name in ("mode 0", "mode -1", "n_out < 1", "T < 1", "Nphi < 1", "rate <= 0", "real taps", "no bank", "real shared taps", "78 KiB exactly", "over 78 KiB"):
        assert named(name) and all(not w[0] for _, w in named(name)), name
    # the default rule from both sides of both of its limits: the measured rows it takes and the one it leaves
    assert all(w[0] == (r[MODE] != 0) for r, w in named("the smallest measured win") + named("many short channels"))
    assert all(w[7:9] == [879, 225_024] for _, w in named("the smallest measured win") if w[0])
    assert all(w[0] == (r[MODE] == 1) for r, w in named("a channel fewer") + named("a tile a channel more") + named("the measured row that did not win"))
    assert all(w[0] == (r[MODE] == 1) for r, w in named("cut span") + named("two tiles"))
    assert all(w[0] and w[5] == math.ceil(255 / 2.123) + 8 + 2 == 131 for _, w in named("the span the slowest rate asks for"))
    assert all(w[5] == 40 * KB // ((8 if r[XF64] else 4) * (2 if r[CX] else 1)) < 25_510 for r, w in named("cut span") if w[0])
    assert all(w[7:9] == [2, 2] for _, w in named("two tiles") if w[0])
    assert all(w[7:9] == [88, 88 * 4096] for _, w in named("many short channels") if w[0])
    # the 78 KiB edge for Complex64 and Complex128 pairs: the banks alone fill it (no window left), one tap a phase fewer leaves 2 KiB
    assert all(w[0] and w[4] == 77_824 and w[9] <= 78 * KB and w[5] == min(2048 // ((8 if r[XF64] else 4) * (2 if r[CX] else 1)), 121 + 37 + 2)
               for r, w in named("under 78 KiB"))
    # the (32, 1024) bank of the GPU tests: 2 * 32 * 33 pairs, 16 896 or 33 792 bytes, and the whole 40 KiB for the samples
    assert all(w[0] and w[4] == (33_792 if r[RF64] else 16_896) and w[5] == 121 + 32 + 2 for r, w in named("Nphi 32 x T 32"))
    text = "".join("plan " + " ".join(repr(v) if i == RATE else str(v) for i, v in enumerate(r)) + "\n" for r in rows)
    text += "".join("ctaps " + " ".join(map(str, args)) + "\n" for args, _ in CTAPS_TABLE)
    text += "".join(f"map {Nphi} {hLen} {f64}\n" for Nphi, hLen in MAPS for f64 in (0, 1))
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows) + len(CTAPS_TABLE) + 2 * len(MAPS)
    have = [[int(v) for v in line.split()] for line in lines[:len(rows)]]
    differing = [(n, r, h, w) for n, r, h, w in zip(why, rows, have, want) if h != w]
    assert not differing, differing[:5]
    for (args, (status, pieces)), line in zip(CTAPS_TABLE, lines[len(rows):]):
        got_status, _, message = line.partition(" ")
        assert int(got_status) == status, (args, line)
        assert all(piece in message for piece in pieces) if status else message == "", (args, line)
        assert not status or message.startswith(OWN + ("_device" if args[0] else "") + (":" if ":" in pieces[0] else " ")), (args, line)
    at = len(rows) + len(CTAPS_TABLE)
    for Nphi, hLen in MAPS:
        for f64 in (0, 1):
            Tp, bad_p, bad_d, zero_p, zero_d = (int(v) for v in lines[at].split())
            at += 1
            Tw = -(-hLen // Nphi)
            assert (Tp, bad_p, bad_d) == (Tw, 0, 0), (Nphi, hLen, f64, lines[at - 1])
            assert zero_p == 3 * (Tw * Nphi - hLen) and zero_d == 3 * (Tw * Nphi - hLen + 1), (Nphi, hLen, f64, lines[at - 1])


# ---- the Python methods on unbound filters ----------------------------------------------------------------------------------------
def _mirrors(f):
    return (None if f._chan_taps is None else f._chan_taps.tobytes(), None if f._chan_ctaps is None else f._chan_ctaps.tobytes(),
            f._rates.tobytes(), f.h.tobytes(), f._handle, f.numerics)


def test_refusals_of_the_python_methods_on_unbound_filters_change_no_mirror(pkg):
    h = np.ones(8, dtype=np.float32)
    rng = np.random.default_rng(5)
    Hc = (rng.standard_normal((3, 8)) + 1j * rng.standard_normal((3, 8))).astype(np.complex64)
    rates = [0.47, 1.0, 2.123]
    f = pkg.FIRFilter.per_channel_rates(h, rates, 4)
    assert f._chan_ctaps is None and f.output_dtype is None
    for filt in (f, pkg.FIRFilter.per_channel_taps_and_rates(Hc.real.copy(), rates, 4)):
        before = _mirrors(filt)
        for bad, code in ((Hc[:2], 1), (Hc[:, :7], 1), (Hc[0], 1), (Hc.reshape(3, 2, 4), 1), (Hc.real.copy(), 1), (Hc.astype(np.complex128), 1)):
            with pytest.raises(pkg.MultirateHIPError) as e:
                filt.set_channel_ctaps(bad)
            assert e.value.code == code, bad.shape
            assert _mirrors(filt) == before                                  # a refused call changes no mirror
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.set_channel_ctaps_device(Hc)                                       # not a device tensor (and the filter is not bound)
    assert e.value.code == 1 and f._chan_ctaps is None
    for other in (pkg.FIRFilter(h, 1.5), pkg.FIRFilter.per_channel_arbitrary(Hc.real.copy(), 1.5), pkg.FIRFilter.complex_taps_arbitrary(Hc[0], 1.5)):
        for call in (other.set_channel_ctaps, other.set_channel_ctaps_device):
            with pytest.raises(pkg.MultirateHIPError) as e:
                call(Hc)                                                     # not a filter of per_channel_rates
            assert e.value.code == 1 and other._chan_ctaps is None
    farrow = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)
    for call in (farrow.set_channel_ctaps, farrow.set_channel_ctaps_device):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call(Hc)
        assert e.value.code == 5 and "FIRFarrow are left out" in str(e.value) and farrow._chan_ctaps is None
    fused = pkg.FIRFilter.per_channel_rates(h, rates, 4, numerics=pkg.NUMERICS_FUSED)
    with pytest.raises(pkg.MultirateHIPError) as e:
        fused.set_channel_ctaps(Hc)                                          # complex taps have no FUSED form
    assert e.value.code == 5 and fused._chan_ctaps is None
    with pytest.raises(pkg.MultirateHIPError) as e:
        fused.set_channel_ctaps(Hc[:2])                                      # (the matrix is looked at first)
    assert e.value.code == 1
    # the install is remembered, the taps may change, and going back is refused
    f.set_channel_ctaps(Hc)
    assert np.array_equal(f._chan_ctaps, Hc) and f._chan_ctaps is not Hc and f._handle is None and np.array_equal(f.h, h)
    f.set_channel_ctaps(Hc[::-1])
    assert np.array_equal(f._chan_ctaps, Hc[::-1])
    before = _mirrors(f)
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.set_channel_taps(Hc.real.copy())
    assert e.value.code == 5 and "going back to real taps is left out" in str(e.value) and _mirrors(f) == before
    # what per_channel_rates and set_channel_taps answered to complex taps, they still answer
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates(h, rates, 4).set_channel_taps(Hc)
    assert e.value.code == 5 and "complex taps with per-channel rates are left out" in str(e.value)
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates(Hc[0], rates, 4)
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_taps_and_rates(Hc, rates, 4)
    assert e.value.code == 5


def test_per_channel_complex_taps_and_rates_unbound(pkg):
    rng = np.random.default_rng(6)
    rates = [0.47, 1.0, 2.123]
    for ct, rt in ((np.complex64, np.float32), (np.complex128, np.float64)):
        H = (rng.standard_normal((3, 30)) + 1j * rng.standard_normal((3, 30))).astype(ct)
        g = pkg.FIRFilter.per_channel_complex_taps_and_rates(H, rates, 4)
        assert g.kind == pkg.host.ARBITRARY and g.Nphi == 4 and g.tapsPerPhi == 8 and g.historyLen == 7 and g._handle is None
        assert g.h.dtype == rt and np.array_equal(g.h, H[0].real) and len(g.h) == 30       # the placeholder: real(H[0]), same length and precision
        assert np.array_equal(g._chan_ctaps, H) and g._chan_ctaps is not H and g._chan_taps is None and g._bank is None
        assert np.array_equal(g._rates, rates) and g.rate == 2.123 and g._tap_dtype == ct
        assert [(s.rate, s.phiAccumulator, s.inputDeficit) for s in g.channel_states] == [(r, 1.0, 1) for r in rates]
        # the complex output type, once the sample type is known (no device object is needed to say it)
        for tx, ty in ((np.float32, ct), (np.complex64, ct), (np.float64, np.complex128), (np.complex128, np.complex128)):
            g._tx = np.dtype(tx)
            assert g.output_dtype == np.dtype(ty), (ct, tx)
        g._tx = None
    assert pkg.FIRFilter.per_channel_complex_taps_and_rates(H, rates).Nphi == 32
    for bad_H, bad_rates, code in ((H, rates[:2], 1), (H[0], rates, 1), (H, [1.0, 0.0, 2.0], 1), (H, [], 1), (H.real.copy(), rates, 1),
                                   (np.ones((3, 0), dtype=np.complex64), rates, 1)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_and_rates(bad_H, bad_rates, 4)
        assert e.value.code == code, (bad_H.shape, bad_rates)
