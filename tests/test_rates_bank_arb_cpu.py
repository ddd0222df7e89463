"""CPU-only checks of per-channel taps with per-channel rates for FIRArbitrary (mrhip_set_channel_taps, FIRFilter.set_channel_taps,
FIRFilter.per_channel_taps_and_rates, the BANK kernels of csrc/kernels_rates_arb.hip): the exported symbol, its declaration and its place in host.ABI
and in the Julia shim; the constructor table that stays at sixteen; the argument errors of the two Python methods on unbound filters;
the answers per_channel_rates and the older constructors keep; the build conditions of the kernel unit; the instantiations in the object
the build made (both filter kernels for (Tx scalar, R) in {(f32,f32), (f32,f64), (f64,f64)} x real / complex samples x STRICT / FUSED =
12 each with BANK true beside the 12 each with BANK false, none with scratch memory or AccVGPRs); and, through a stand-alone program
built with -fsanitize=address,undefined, the tiled kernel's plan (csrc/host_logic.cpp: plan_arb_rates_tiled on both bank keys) against values computed here from the plan's stated formulas and the pure
argument checks of mrhip_set_channel_taps (check_channel_taps) against a table of (arguments -> status, message)."""
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
UNIT = "kernels_rates_arb.hip"                                               # one unit for shared taps and for a bank per channel


def test_the_library_exports_the_symbol_and_the_header_declares_it(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "mrhip_set_channel_taps")
    assert len([1 for n, _, _ in pkg.host.ABI if n == "mrhip_set_channel_taps"]) == 1
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_set_channel_taps\(mrhip_filter \*f, const void \*h(?: /\*[^*]*\*/)?, int64_t hLen, int tap_dtype\);", hdr)
    assert "Per-channel taps with per-channel rates for FIRArbitrary" in hdr
    assert "arb_rates_bank_generic" in hdr and "arb_rates_bank_tiled" in hdr.split("const char *mrhip_last_kernel_name")[0].rsplit("/*", 1)[1]
    assert len(set(re.findall(r"^int (mrhip_create_\w+)\(", hdr, flags=re.M))) == 16          # a call, not a seventeenth constructor
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    assert "function set_channel_taps!(f::RatesFIRFilter" in jl and ":mrhip_set_channel_taps" in jl
    assert re.search(r"function FIRFilter\(H::Matrix\{Th\}, rates::Vector", jl)


def test_argument_errors_of_the_python_methods_on_unbound_filters(pkg):
    h = np.ones(8, dtype=np.float32)
    H = np.arange(24, dtype=np.float32).reshape(3, 8)
    rates = [0.47, 1.0, 2.123]
    f = pkg.FIRFilter.per_channel_rates(h, rates, 4)
    for bad in (H[:2], H[:, :7], H[0], H.reshape(3, 2, 4), H.astype(np.float64)):              # wrong shape; the other real class
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_taps(bad)
        assert e.value.code == 1
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_taps(H.astype(ct))
        assert e.value.code == 5
    assert f._chan_taps is None                                              # a refused call leaves nothing behind
    f.set_channel_taps(H)                                                    # remembered, installed at bind
    assert np.array_equal(f._chan_taps, H) and f._chan_taps is not H and f._handle is None
    f.set_channel_taps(H[::-1])                                              # taps may change
    assert np.array_equal(f._chan_taps, H[::-1])
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter(h, 1.5).set_channel_taps(H)                            # not a filter of per_channel_rates
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_arbitrary(H, 1.5).set_channel_taps(H)
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2).set_channel_taps(H)      # FIRFarrow: left out
    assert e.value.code == 5
    # per_channel_taps_and_rates: the filter of per_channel_rates(H[0], ...) with the matrix behind it
    g = pkg.FIRFilter.per_channel_taps_and_rates(H, rates, 4)
    assert g.kind == pkg.host.ARBITRARY and g.Nphi == 4 and g.tapsPerPhi == 2 and g.historyLen == 1 and np.array_equal(g.h, H[0])
    assert np.array_equal(g._chan_taps, H) and np.array_equal(g._rates, rates) and g._bank is None and g.rate == 2.123
    assert pkg.FIRFilter.per_channel_taps_and_rates(H, rates).Nphi == 32
    assert [(s.rate, s.phiAccumulator, s.inputDeficit) for s in g.channel_states] == [(r, 1.0, 1) for r in rates]
    for bad_H, bad_rates, code in ((H, rates[:2], 1), (H[0], rates, 1), (H, [1.0, 0.0, 2.0], 1), (H, [], 1), (H.astype(np.complex64), rates, 5),
                                   (np.ones((3, 0), dtype=np.float32), rates, 1)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_taps_and_rates(bad_H, bad_rates, 4)
        assert e.value.code == code, (bad_H.shape, bad_rates)


def test_per_channel_rates_and_the_older_constructors_keep_their_answers(pkg):
    h = np.arange(30, dtype=np.float64)
    f = pkg.FIRFilter.per_channel_rates(h, [0.47, 1.0, 2.123], 4)
    assert f._chan_taps is None and f._bank is None and f.kind == pkg.host.ARBITRARY and f.tapsPerPhi == 8 and f.historyLen == 7
    assert [(s.rate, s.delta, s.phiAccumulator, s.alpha, s.phiIdx, s.inputDeficit, s.xIdx, s.last_count) for s in f.channel_states] == \
        [(r, 4 / r, 1.0, 0.0, 1, 1, 1, 0) for r in (0.47, 1.0, 2.123)]
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates(h.astype(ct), [1.5])
        assert e.value.code == 5
    H = np.ones((3, 8), dtype=np.float32)
    one, bank = pkg.FIRFilter(H[0], 2.123, 4), pkg.FIRFilter.per_channel_arbitrary(H, 1.5)
    assert one._chan_taps is None and one._rates is None and bank._chan_taps is None and bank._rates is None and bank._bank is not None
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_arbitrary(H.astype(np.complex64), 1.5)
    assert e.value.code == 5


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_arb\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_rates_arb\.hip\.o.*:.*\bvariant_device\.h\b.*\brates_arb\.h\b", mk, flags=re.M)
    assert "kernels_rates_bank_arb" not in mk and not os.path.exists(os.path.join(CSRC, "kernels_rates_bank_arb.hip"))      # no second unit
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src and '#include "rates_arb.h"' in src and "RealTaps<TX, R, NCX, FUSED>" in src
    assert "stage_window(" in src and "tile_run(" in src and "tile_span(" in src and "arb_dots_global<A>" in src and "ch_in_lds" in src
    assert "shiftin_by_last_workgroup" in src and "shiftin_ragged_by_last_workgroup" in src and "rates_channel_len(" in src
    assert "asm" not in src                                                  # plain HIP
    assert "atomic" not in src.lower()                                       # no atomics: no workgroup waits for another, no spin loop
    assert '"arb_rates_bank_generic"' in src and '"arb_rates_bank_tiled"' in src and not re.search(r'"[a-z_]+_kernel"', src)
    # both kernels end with the epilogue, ragged and plain, and no return stands in front of it
    assert src.count("shiftin_by_last_workgroup") == 2 and src.count("shiftin_ragged_by_last_workgroup") == 2
    for kernel in ("arb_rates_generic_kernel(ArbArgs a, RatesArgs r)", "arb_rates_tiled_kernel(ArbArgs a, RatesArgs r, ArbTileArgs ta)"):
        body = src.split(kernel)[1].split("dev::shiftin_by_last_workgroup")[0]
        assert "dev::shiftin_ragged_by_last_workgroup" in body and not re.search(r"\breturn;", body), kernel
    # BANK is the kernels' last template argument and stands at the statements that differ: the column's bank base (stated ONCE), and in
    # the tiled kernel where the banks go into LDS -- in front of the tile loop, or behind the first barrier of a live tile of another
    # channel; the copy loop itself is stated once
    assert src.count("template <typename TX, typename R, int NCX, bool FUSED, bool BANK>\n__global__") == 2
    assert src.count("ch * bank_elems") == 1 and "if constexpr (BANK) col = ch * bank_elems + col;" in src
    tiled = src.split("arb_rates_tiled_kernel(ArbArgs a, RatesArgs r, ArbTileArgs ta)")[1].split("dev::shiftin_by_last_workgroup")[0]
    loop = tiled.index("for (long long tile = run.begin")
    assert tiled.index("if constexpr (!BANK)") < tiled.index("if (run.begin < run.end) rates_banks_to_lds(") < loop
    assert loop < tiled.index("__syncthreads();") < tiled.index("if constexpr (BANK)") < tiled.index("if (ch != ch_in_lds)") < tiled.index("stage_window(")
    assert tiled.count("rates_banks_to_lds(") == 2 and src.count("void rates_banks_to_lds(") == 1
    assert src.count("lpfb[phi * TP + i] = g0[e];") == 1 and src.count("ldpfb[phi * TP + i] = g1[e];") == 1


def test_the_bank_key_is_read_in_one_place_and_selects_argument_name_and_switch_together():
    """(was: the sibling unit's launches refuse a bank key.)  With one unit the key is the selector: TypeKey::bank is read in ONE function
    of the unit, which gives the kernels' BANK argument, the reported names and the switches of that key; nothing else of the unit reads
    it, and the launches keep their other refusals"""
    src = open(os.path.join(CSRC, UNIT)).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    key = code.split("static RatesKey rates_key(const TypeKey &tk)")[1].split("\n}\n")[0]
    assert code.count("tk.bank") == key.count("tk.bank") == 5
    assert 'RatesKey{tk.bank, tk.bank ? "arb_rates_bank_generic" : "arb_rates_generic", tk.bank ? "arb_rates_bank_tiled" : "arb_rates_tiled",' in key
    assert 'tk.bank ? MRHIP_ENV_INT("MRHIP_ARB_RATES_BANK_TILED", -1) : MRHIP_ENV_INT("MRHIP_ARB_RATES_TILED", -1)' in key
    assert 'tk.bank ? MRHIP_ENV_INT("MRHIP_ARB_RATES_BANK_GRID", 0) : MRHIP_ENV_INT("MRHIP_ARB_RATES_GRID", 0)' in key
    assert code.count("MRHIP_ENV_INT(") == 4                                  # the four switches, each a literal name at a site of its own
    assert code.count("dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>()") == 3 and "dispatch_variant(" not in code
    assert code.count("*kname = key.generic;") == 1 and code.count("*kname = key.tiled;") == 1 and code.count("*kname = ") == 2
    assert "rates_key(tk).tiled_mode" in code and code.count("key.grid_fixed") == 2
    assert "if (tk.complex_h || a.dyn) return hipErrorInvalidValue;" in code and "if (tk.complex_h) return hipErrorInvalidValue;" in code
    assert "if (tk.complex_h || a.dyn || grid < 1) return hipErrorInvalidValue;" in code
    assert '"arb_rates_generic"' in src and '"arb_rates_tiled"' in src and not re.search(r'"[a-z_]+_kernel"', src)
    assert "arb_rates_bank_generic_kernel" not in src and "arb_rates_bank_tiled_kernel" not in src       # no second kernel, no wrapper
    assert src.count("arb_rates_generic_kernel<TX, R, NCX, true, BANK>") == 1 and src.count("arb_rates_tiled_kernel<TX, R, NCX, true, BANK>") == 1
    hdr = open(os.path.join(CSRC, "rates_arb.h")).read()
    assert not re.search(r"\b\w+_rates_bank_(generic|tiled|multi)\(", hdr)   # one set of declarations per family
    api = open(os.path.join(CSRC, "api.hip")).read()
    calls = api.split("static int rates_call(")[1].split("\nint mrhip_filt_device_rates(")[0]
    assert not re.search(r"_rates_bank_(generic|tiled|multi)\(", calls)
    assert calls.index("prepare_arb_rates_tiled(") < calls.index("launch_rates_schedule(") < calls.index("launch_arb_rates_tiled(")   # what can fail: before the state moves


def test_rates_bank_kernels_use_no_scratch(pkg):
    obj = os.path.join(CSRC, "build", UNIT + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in (UNIT, "variant_device.h", "ctaps_device.h", "rates_arb.h"))
    if os.path.getmtime(obj) < newest:
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel in ("arb_rates_generic_kernel", "arb_rates_tiled_kernel"):       # 12 with BANK true beside the 12 with BANK false, none spilling
        _assert_rates_filter_kernel(sizes, kernel)


# ---- the plan and the argument checks, through one stand-alone program ------------------------------------------------------------
# a plan row: x_f64 r_f64 complex_x complex_h bank Nphi T n_out nch rate_min num_cus mode
XF64, RF64, CX, CH, BANK, NPHI, T, NOUT, NCH, RATE, CUS, MODE = range(12)
RULE_MIN_TILES, RULE_MAX_PER_CHANNEL = 225_024, 879    # the default rule (mode -1): the measured rows the tiled kernel won
SHARED_RULE = (225_024, 879)                           # ... and with shared taps: the rule of a row without a bank key


def _expected(r):
    """the plan from its stated formulas, the limits of the default rule by the row's bank key: ONE channel's pfb and dpfb (without a
    bank key: the shared pair, the same geometry), (2 Nphi (T+1) sizeof(R) + 15)/16*16 bytes, at most 78 KiB together with the samples; the samples take 40 KiB or what is left, in whole 16-byte units; one channel a lane; the span
    ceil(255/rate_min) + T + 2 (the slowest channel), cut to the room only when forced; a tile is 256 outputs of one channel, the tiling
    goes by n_out (the call's bound); the default rule (mode -1) as DESIGN.md 9 item 21 derives it"""
    refused = [0] * 10
    min_tiles, max_per_channel = (RULE_MIN_TILES, RULE_MAX_PER_CHANNEL) if r[BANK] else SHARED_RULE
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
    if r[MODE] != 1 and (min_tiles is None or tpc * r[NCH] < min_tiles or tpc > max_per_channel):
        return refused
    return [1, 1, pitch, r[NPHI] * pitch, fixed, span, 256, tpc, tpc * r[NCH], fixed + span * sample]


def _rows():
    rows, why = [], []
    for xf64, rf64 in ((0, 0), (0, 1), (1, 1)):
        for cx in (0, 1):
            for cus in (8, 256):
                base = [xf64, rf64, cx, 0, 1, 32, 8, 40_000, 33, 2.123, cus]
                for mode in (-1, 0, 1):
                    rows.append(base + [mode]), why.append("the span the slowest rate asks for" if mode == 1 else f"mode {mode}")
                    rows.append(base[:RATE] + [0.01, cus, mode]), why.append("cut span")
                    rows.append(base[:NOUT] + [257, 1, 2.123, cus, mode]), why.append("two tiles")
                    rows.append(base[:NOUT] + [22_502, 4096, 2.0, cus, mode]), why.append("many short channels")            # 88 x 4096 tiles
                    rows.append(base[:NOUT] + [225_002, 256, 2.0, cus, mode]), why.append("long channels")                  # 879 x 256 tiles
                    rows.append(base[:NPHI] + [128 if rf64 else 256, 38, 5000, 3, 2.123, cus, mode]), why.append("not even one window")
                    if RULE_MIN_TILES is not None:
                        tpc = RULE_MAX_PER_CHANNEL
                        nch = -(-RULE_MIN_TILES // tpc)
                        rows.append(base[:NOUT] + [tpc * 256, nch, 2.0, cus, mode]), why.append("at both limits")
                        rows.append(base[:NOUT] + [tpc * 256, nch - 1, 2.0, cus, mode]), why.append("a channel fewer")
                        rows.append(base[:NOUT] + [tpc * 256 + 1, nch, 2.0, cus, mode]), why.append("a tile a channel more")
                for change, name in (({NOUT: 0}, "n_out < 1"), ({T: 0}, "T < 1"), ({NPHI: 0}, "Nphi < 1"), ({RATE: 0.0}, "rate <= 0"),
                                     ({RATE: -1.0}, "rate <= 0"), ({CH: 1}, "complex taps"), ({BANK: 0}, "shared taps"),
                                     ({NPHI: 32, T: 32}, "Nphi 32 x T 32"), ({NPHI: 512, T: 40}, "over 78 KiB")):
                    row = base + [1]
                    for k, v in change.items():
                        row[k] = v
                    rows.append(row), why.append(name)
    return rows, why


F32, F64, C64, C128 = range(4)
# (is_rates, is_farrow, h_is_null, hLen, tap_dtype, filter_hLen, filter_tap_dtype) -> (status, a piece of the message): the header's
# contract, in its order -- the filter first, then h, hLen, the tap class, the tap type
TAPS_TABLE = [
    ((1, 0, 0, 250, F32, 250, F32), (0, "")),
    ((1, 0, 0, 250, F64, 250, F64), (0, "")),
    ((1, 0, 0, 1, F32, 1, F32), (0, "")),
    ((1, 1, 0, 250, F32, 250, F32), (5, "FIRFarrow")),
    ((1, 1, 1, 3, C64, 250, F32), (5, "FIRFarrow")),                        # (whatever else is wrong)
    ((0, 0, 0, 250, F32, 250, F32), (1, "mrhip_set_channel_taps takes a filter of mrhip_create_arbitrary_rates")),
    ((0, 1, 0, 250, F32, 250, F32), (1, "mrhip_set_channel_taps takes a filter of mrhip_create_arbitrary_rates")),
    ((0, 0, 1, 3, C64, 250, F32), (1, "mrhip_set_channel_taps takes a filter of mrhip_create_arbitrary_rates")),
    ((1, 0, 1, 250, F32, 250, F32), (1, "h is NULL")),
    ((1, 0, 1, 3, C64, 250, F32), (1, "h is NULL")),
    ((1, 0, 0, 249, F32, 250, F32), (1, "hLen")),
    ((1, 0, 0, 251, F32, 250, F32), (1, "hLen")),
    ((1, 0, 0, 0, F32, 250, F32), (1, "hLen")),
    ((1, 0, 0, 249, C64, 250, F32), (1, "hLen")),
    ((1, 0, 0, 250, C64, 250, F32), (5, "complex taps with per-channel rates are left out")),
    ((1, 0, 0, 250, C128, 250, F64), (5, "complex taps with per-channel rates are left out")),
    ((1, 0, 0, 250, F64, 250, F32), (1, "the filter's tap dtype")),
    ((1, 0, 0, 250, F32, 250, F64), (1, "the filter's tap dtype")),
    ((1, 0, 0, 250, -1, 250, F32), (1, "bad tap dtype")),
    ((1, 0, 0, 250, 4, 250, F32), (1, "bad tap dtype")),
]


def test_the_plan_of_the_tiled_kernel_and_the_argument_checks(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "arb_rates_bank_plan_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "arb_rates_bank_plan_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows, why = _rows()
    want = [_expected(r) for r in rows]
    named = lambda name: [(r, w) for r, w, n in zip(rows, want, why) if n == name]
    # the rows reach every return, the default rule from both sides of each of its limits
    for name in ("mode 0", "n_out < 1", "T < 1", "Nphi < 1", "rate <= 0", "complex taps", "over 78 KiB", "not even one window"):
        assert named(name) and all(not w[0] for _, w in named(name)), name
    # shared taps are no refusal: the plan of the shared-taps kernel, whose LDS geometry is one channel's
    assert named("shared taps") and all(not r[BANK] and w == _expected(r[:BANK] + [1] + r[BANK + 1:]) and w[0] for r, w in named("shared taps"))
    assert all(w[0] == (r[MODE] == 1) for r, w in named("cut span") + named("two tiles"))
    if RULE_MIN_TILES is None:
        assert all(not w[0] for _, w in named("mode -1") + [(r, w) for r, w in zip(rows, want) if r[MODE] == -1])
    else:
        assert all(w[0] == (r[MODE] != 0) and (not w[0] or (w[7], w[8] >= RULE_MIN_TILES) == (RULE_MAX_PER_CHANNEL, True)) for r, w in named("at both limits"))
        assert all(w[0] == (r[MODE] == 1) for r, w in named("a channel fewer") + named("a tile a channel more"))
    assert all(w[0] and w[5] == math.ceil(255 / 2.123) + 8 + 2 == 131 for _, w in named("the span the slowest rate asks for"))
    assert all(w[5] == 40 * KB // ((8 if r[XF64] else 4) * (2 if r[CX] else 1)) < 25_510 for r, w in named("cut span") if w[0])
    assert all(w[7] == 2 and w[8] == 2 for _, w in named("two tiles") if w[0])
    assert all(w[7:9] == [88, 88 * 4096] for _, w in named("many short channels") if w[0]) and any(w[0] for _, w in named("many short channels"))
    # the (32, 1024) bank of the GPU tests: 2 * 32 * 33 taps, 8448 or 16896 bytes, and the whole 40 KiB for the samples
    assert all(w[0] and w[4] == (16_896 if r[RF64] else 8_448) and w[5] == 121 + 32 + 2 for r, w in named("Nphi 32 x T 32"))
    text = "".join("plan " + " ".join(repr(v) if i == RATE else str(v) for i, v in enumerate(r)) + "\n" for r in rows)
    text += "".join("taps " + " ".join(map(str, args)) + "\n" for args, _ in TAPS_TABLE)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows) + len(TAPS_TABLE)
    have = [[int(v) for v in line.split()] for line in lines[:len(rows)]]
    differing = [(n, r, h, w) for n, r, h, w in zip(why, rows, have, want) if h != w]
    assert not differing, differing[:5]
    for (args, (status, piece)), line in zip(TAPS_TABLE, lines[len(rows):]):
        got_status, _, message = line.partition(" ")
        assert int(got_status) == status, (args, line)
        assert (piece in message) if status else message == "", (args, line)
