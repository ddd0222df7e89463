"""CPU-only checks of the device-resident updates of the filters with per-channel rates (mrhip_set_channel_rates_device,
mrhip_set_channel_taps_device, mrhip_set_channel_pnfb_device; FIRFilter.set_channel_rates_device / .set_channel_taps_device /
.set_channel_pnfb_device; csrc/kernels_rates_bank_build.hip and rates_set_kernel of csrc/kernels_rates_arb.hip): the exported symbols,
their declarations and their places in host.ABI and in the Julia shim; the constructor table that stays at sixteen; what the Python
methods refuse without a GPU (host arrays, unbound filters, the wrong filter kinds) and that a refused call changes no mirror; the build
conditions of the new unit and the instantiations in the object the build made (the bank build kernel for (tap, R) in {(f32,f32),
(f32,f64), (f64,f64)}, the coefficient kernel with and without the Float32 rounding, rates_set_kernel; none with scratch memory); and,
through a stand-alone program built with -fsanitize=address,undefined, the index map the bank build kernel compiles (csrc/rates_arb.h)
against taps2pfb of h and of [diff(h), 0] byte for byte, and the pure argument checks of the three calls (csrc/host_logic.cpp) against
tables of (arguments -> status, message)."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "kernels_rates_bank_build.hip"
SYMBOLS = ("mrhip_set_channel_rates_device", "mrhip_set_channel_taps_device", "mrhip_set_channel_pnfb_device")
BANKS = [(4, 4), (4, 30), (3, 40), (32, 250), (32, 1024)]     # (Nphi, hLen) of tests/test_gpu_rates_arb.py (a GPU module: not imported here)


def test_the_library_exports_the_three_symbols_and_the_header_declares_them(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len([1 for n, _, _ in pkg.host.ABI if n == name]) == 1, name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    c = r"(?: /\*[^*]*\*/)?"
    assert re.search(r"int mrhip_set_channel_rates_device\(mrhip_filter \*f, const double \*rates" + c + r", double rate_lo, double rate_hi, void \*stream\);", hdr)
    assert re.search(r"int mrhip_set_channel_taps_device\(mrhip_filter \*f, const void \*h" + c + r", int64_t hLen, int tap_dtype, void \*stream\);", hdr)
    assert re.search(r"int mrhip_set_channel_pnfb_device\(mrhip_filter \*f, const double \*pnfb" + c + r", int64_t tapsPerPhi,\s+int64_t polyorder, void \*stream\);", hdr)
    block = hdr.split("Device-resident updates for the filters with per-channel rates")[1].split("int mrhip_set_channel_rates_device")[0]
    for left_out in ("lengths that live on the device", "fit on the device", "a stream other than", "graph capture", "complex taps", "parallel schedule"):
        assert left_out in block, left_out
    assert "freed right after that one wait" in block                        # which of the two allocation rules was chosen
    assert len(set(re.findall(r"^int (mrhip_create_\w+)\(", hdr, flags=re.M))) == 16          # three calls, not a seventeenth constructor
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    for name in SYMBOLS:
        assert jl.count(":" + name + ",") == 1, name
        assert "function " + name[len("mrhip_"):] + "!(f::RatesFIRFilter" in jl, name


def test_what_the_python_methods_refuse_without_a_gpu(pkg):
    import torch
    h = np.ones(8, dtype=np.float32)
    H = np.arange(24, dtype=np.float32).reshape(3, 8)
    PN = np.arange(18, dtype=np.float64).reshape(3, 2, 3)
    rates = [0.47, 1.0, 2.123]
    arb = pkg.FIRFilter.per_channel_rates(h, rates, 4)
    far = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)
    arb_taps = pkg.FIRFilter.per_channel_taps_and_rates(H, rates, 4)
    r64 = np.array(rates)
    calls = []
    for f in (arb, far, arb_taps):
        for value in (r64, list(rates), torch.from_numpy(r64)):                              # host arrays, a CPU tensor
            calls.append((f, lambda f=f, v=value: f.set_channel_rates_device(v, 0.4, 2.2)))
    for value in (H, torch.from_numpy(H)):
        calls += [(g, lambda g=g, v=value: g.set_channel_taps_device(v)) for g in (arb, arb_taps, far)]
    for value in (PN, torch.from_numpy(PN)):
        calls += [(g, lambda g=g, v=value: g.set_channel_pnfb_device(v)) for g in (far, arb)]
    one, bank = pkg.FIRFilter(h, 1.5, 4), pkg.FIRFilter.per_channel_arbitrary(H, 1.5, 4)
    rational = pkg.FIRFilter(h, Fraction(2, 3))
    for g in (one, bank, rational):                                                          # not filters with per-channel rates
        calls += [(g, lambda g=g: g.set_channel_rates_device(torch.from_numpy(r64), 0.4, 2.2)),
                  (g, lambda g=g: g.set_channel_taps_device(torch.from_numpy(H))), (g, lambda g=g: g.set_channel_pnfb_device(torch.from_numpy(PN)))]
    mirrors = lambda f: (None if f._rates is None else f._rates.tobytes(), None if f._chan_taps is None else f._chan_taps.tobytes(), f._chan_farrow, f.rate, f._handle)
    for f, call in calls:
        before = mirrors(f)
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == 1
        assert mirrors(f) == before                                          # a refused call changes no mirror
    assert arb.rate == 2.123 and [s.rate for s in arb.channel_states] == rates
    # the existing methods accept what they accepted
    arb.set_channel_rates([1.0, 2.0, 3.0]), arb.set_channel_taps(H), far.set_channel_pnfb(PN)
    assert arb.rate == 3.0 and np.array_equal(arb._chan_taps, H) and far._chan_farrow[0] == "pnfb"


def test_the_unit_is_in_the_makefile_with_the_flags_of_its_sibling():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_bank_build\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_rates_bank_build\.hip\.o.*:.*\brates_arb\.h\b", mk, flags=re.M)
    assert not re.search(r"kernels_rates_bank_build\.hip\.o[^\n]*EXTRA", mk)                 # no flag of its own, as kernels_rates_arb.hip
    assert "fast-math" not in mk
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "#pragma clang fp contract(off)" in src and '#include "rates_arb.h"' in src
    assert "rates_bank_tap_index(" in src and "rates_bank_pfb_value<TAP>(" in src and "rates_bank_dpfb_value<TAP>(" in src
    assert "asm" not in src and "atomic" not in src.lower()                  # plain HIP; no workgroup waits for another
    hdr = open(os.path.join(CSRC, "rates_arb.h")).read()
    assert re.search(r"MRHIP_RATES_HD inline long long rates_bank_tap_index\(", hdr)         # ONE statement of the map, for the kernel and the host program
    rates = open(os.path.join(CSRC, "kernels_rates_arb.hip")).read()
    assert "void rates_set_kernel(" in rates and "void rates_reset_kernel(" in rates and "atomic" not in rates.lower()
    asan = re.search(r"^\.\./libmultirate_host_asan\.so:.*$", mk, flags=re.M).group(0)
    assert "host_logic.cpp" in asan and "rates_arb.h" in asan and "create.h" in asan         # `make asan` builds the new host checks too


def test_the_new_kernels_are_in_the_objects_and_use_no_scratch(pkg):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm tools")
    for unit, deps, kernels in ((UNIT, ("rates_arb.h",), (("rates_bank_build_kernel", 3), ("rates_pnfb_install_kernel", 2))),
                                ("kernels_rates_arb.hip", ("rates_arb.h", "sched_step.h", "variant_device.h"), (("rates_set_kernel", 1),))):
        obj = os.path.join(CSRC, "build", unit + ".o")
        if not os.path.exists(obj):
            pytest.skip("no built object (the library came prebuilt)")
        if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, s)) for s in (unit,) + deps):
            pytest.skip("object older than its source")
        sizes = _kernel_scratch(obj)
        for kernel, count in kernels:
            mine = {k: v for k, v in sizes.items() if kernel in k}
            assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
            spilling = {k: v for k, v in mine.items() if v != 0}
            assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())}"


# ---- the index map and the argument checks, through one stand-alone program -------------------------------------------------------
F32, F64, C64, C128 = range(4)
WHO_R = "mrhip_set_channel_rates_device"
# (is_rates, rates_is_null, rate_lo, rate_hi) -> (status, a piece of the message): the header's contract
RANGE_TABLE = [
    ((1, 0, "2.0", "2.25"), (0, "")),
    ((1, 0, "1.5", "1.5"), (0, "")),                                         # lo == hi
    ((1, 0, repr(2.0 ** -30), "1.0"), (0, "")),
    ((0, 0, "2.0", "2.25"), (1, WHO_R + " takes a filter of mrhip_create_arbitrary_rates")),
    ((1, 1, "2.0", "2.25"), (1, WHO_R + ": rates is NULL")),
    ((1, 0, "0.0", "2.25"), (1, WHO_R + ": rate_lo and rate_hi must be finite and greater than 0")),
    ((1, 0, "2.0", "0.0"), (1, "finite and greater than 0")),
    ((1, 0, "-1.0", "2.25"), (1, "finite and greater than 0")),
    ((1, 0, "2.0", "-2.25"), (1, "finite and greater than 0")),
    ((1, 0, "nan", "2.25"), (1, "finite and greater than 0")),
    ((1, 0, "2.0", "nan"), (1, "finite and greater than 0")),
    ((1, 0, "inf", "inf"), (1, "finite and greater than 0")),
    ((1, 0, "2.0", "inf"), (1, "finite and greater than 0")),
    ((1, 0, "2.25", "2.0"), (1, WHO_R + ": rate_hi < rate_lo")),
    ((1, 0, repr(2.0 ** -31), "1.0"), (5, WHO_R + ": a per-channel rate below 2^-30")),
    ((1, 0, repr(2.0 ** -31), repr(2.0 ** -32)), (1, "rate_hi < rate_lo")),  # (the argument errors first)
]
# (is_rates, is_farrow, h_is_null, hLen, tap_dtype, filter_hLen, filter_tap_dtype): a FIRFarrow filter is pointed to the pnfb call, then
# check_channel_taps unchanged
TAPS_TABLE = [
    ((1, 0, 0, 250, F32, 250, F32), (0, "")),
    ((1, 0, 0, 250, F64, 250, F64), (0, "")),
    ((1, 1, 0, 250, F32, 250, F32), (5, "mrhip_set_channel_pnfb_device")),
    ((1, 1, 1, 3, C64, 250, F32), (5, "mrhip_set_channel_pnfb_device")),
    ((0, 0, 0, 250, F32, 250, F32), (1, "takes a filter of mrhip_create_arbitrary_rates")),
    ((0, 1, 0, 250, F32, 250, F32), (1, "takes a filter of mrhip_create_arbitrary_rates")),
    ((1, 0, 1, 250, F32, 250, F32), (1, "h is NULL")),
    ((1, 0, 0, 249, F32, 250, F32), (1, "hLen")),
    ((1, 0, 0, 250, C64, 250, F32), (5, "complex taps with per-channel rates are left out")),
    ((1, 0, 0, 250, F64, 250, F32), (1, "the filter's tap dtype")),
    ((1, 0, 0, 250, 4, 250, F32), (1, "bad tap dtype")),
]
# (is_rates, is_farrow, pnfb_is_null, tapsPerPhi, polyorder, filter_T, filter_polyorder)
PNFB_TABLE = [
    ((1, 1, 0, 8, 4, 8, 4), (0, "")),
    ((1, 0, 0, 8, 4, 8, 4), (1, "mrhip_set_channel_taps_device")),
    ((1, 0, 1, 7, 3, 8, 4), (1, "mrhip_set_channel_taps_device")),
    ((0, 1, 0, 8, 4, 8, 4), (1, "takes a filter of mrhip_create_farrow_rates")),
    ((0, 0, 0, 8, 4, 8, 4), (1, "takes a filter of mrhip_create_farrow_rates")),
    ((1, 1, 1, 8, 4, 8, 4), (1, "pnfb is NULL")),
    ((1, 1, 0, 7, 4, 8, 4), (1, "tapsPerPhi and polyorder")),
    ((1, 1, 0, 8, 3, 8, 4), (1, "tapsPerPhi and polyorder")),
]


def test_the_index_map_and_the_argument_checks(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rates_device_updates_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "rates_device_updates_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    maps = [(Nphi, hLen, f64) for Nphi, hLen in BANKS for f64 in (0, 1)]
    text = "".join(f"map {Nphi} {hLen} {f64}\n" for Nphi, hLen, f64 in maps)
    text += "".join("range " + " ".join(map(str, args)) + "\n" for args, _ in RANGE_TABLE)
    text += "".join("taps " + " ".join(map(str, args)) + "\n" for args, _ in TAPS_TABLE)
    text += "".join("pnfb " + " ".join(map(str, args)) + "\n" for args, _ in PNFB_TABLE)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(maps) + len(RANGE_TABLE) + len(TAPS_TABLE) + len(PNFB_TABLE)
    for (Nphi, hLen, f64), line in zip(maps, lines):
        T = -(-hLen // Nphi)
        pad = Nphi * T - hLen                                               # the zero padding of the pfb bank; the dpfb bank has one zero more
        assert [int(v) for v in line.split()] == [T, 0, 0, pad, pad + 1], (Nphi, hLen, f64, line)
    assert (-(-4 // 4), -(-30 // 4), -(-40 // 3)) == (1, 8, 14)             # T = 1; zero padding; hLen no multiple of Nphi
    at = len(maps)
    for table in (RANGE_TABLE, TAPS_TABLE, PNFB_TABLE):
        for (args, (status, piece)), line in zip(table, lines[at:]):
            got_status, _, message = line.partition(" ")
            assert int(got_status) == status, (args, line)
            assert (piece in message) if status else message == "", (args, line)
        at += len(table)
