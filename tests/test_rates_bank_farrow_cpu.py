"""CPU-only checks of per-channel taps with per-channel rates for FIRFarrow (mrhip_set_channel_taps_farrow, mrhip_set_channel_pnfb,
FIRFilter.set_channel_taps_farrow, FIRFilter.set_channel_pnfb, FIRFilter.per_channel_taps_and_rates_farrow, the BANK kernels of
csrc/kernels_rates_farrow.hip): the exported symbols, their declarations and their place in host.ABI and in the Julia shim; the
constructor table that stays at sixteen; the argument errors of the Python methods on unbound filters and the remembered matrix; the
answers the older constructors and set_channel_taps keep; the build conditions of the kernel unit and the ONE text of the Horner chains
and the dots all FIRFarrow kernels with per-channel rates use; the instantiations in the object the build made (both filter kernels for
(Tx scalar, R) in {(f32,f32), (f32,f64), (f64,f64)} x real / complex samples x STRICT / FUSED = 12 each with BANK true beside the 12 each
with BANK false, none with scratch memory or AccVGPRs); and, through a stand-alone program built with -fsanitize=address,undefined, the
multi kernel's plan (csrc/host_logic.cpp: plan_farrow_rates_multi on both bank keys) against values computed here from the plan's stated formulas and the pure argument checks of the two calls
(check_channel_taps_farrow) against a table of (arguments -> status, message)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _assert_rates_filter_kernel, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "kernels_rates_farrow.hip"                                            # one unit for the one bank and for a bank per channel
SYMBOLS = ("mrhip_set_channel_taps_farrow", "mrhip_set_channel_pnfb")
OPL, LANES = 4, 256


def test_the_library_exports_the_two_symbols_and_the_header_declares_them(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len([1 for n, _, _ in pkg.host.ABI if n == name]) == 1, name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_set_channel_taps_farrow\(mrhip_filter \*f, const void \*h(?: /\*[^*]*\*/)?, int64_t hLen, int tap_dtype\);", hdr)
    assert re.search(r"int mrhip_set_channel_pnfb\(mrhip_filter \*f, const double \*pnfb(?: /\*[^*]*\*/)?, int64_t tapsPerPhi, int64_t polyorder\);", hdr)
    assert "Per-channel taps with per-channel rates for FIRFarrow" in hdr
    at_name = hdr.split("const char *mrhip_last_kernel_name")[0].rsplit("/*", 1)[1]
    assert "farrow_rates_bank_generic" in at_name and "farrow_rates_bank_multi" in at_name
    assert len(set(re.findall(r"^int (mrhip_create_\w+)\(", hdr, flags=re.M))) == 16          # two calls, not a seventeenth constructor
    for left_out in ("complex taps", "going back to shared taps", "stream-ordered update", "the fit on the device", "graph capture", "parallel schedule"):
        assert left_out in hdr.split("Per-channel taps with per-channel rates for FIRFarrow (")[1].split("int mrhip_set_channel_taps_farrow")[0], left_out
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    assert "function set_channel_taps_farrow!(f::RatesFIRFilter" in jl and ":mrhip_set_channel_taps_farrow" in jl
    assert "function set_channel_pnfb!(f::RatesFIRFilter" in jl and ":mrhip_set_channel_pnfb" in jl
    assert re.search(r"function FIRFilter\(H::Matrix\{Th\}, rates::Vector\{<:AbstractFloat\}, Nphi::Integer, polyorder::Integer", jl)


def test_argument_errors_of_the_python_methods_on_unbound_filters(pkg):
    h = np.ones(8, dtype=np.float32)
    H = np.arange(24, dtype=np.float32).reshape(3, 8) ** 2
    PN = np.arange(18, dtype=np.float64).reshape(3, 2, 3)
    rates = [0.47, 1.0, 2.123]
    f = pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)               # tapsPerPhi 2, polyorder 2
    for bad in (H[:2], H[:, :7], H[0], H.reshape(3, 2, 4), H.astype(np.float64)):              # wrong shape; the other real class
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_taps_farrow(bad)
        assert e.value.code == 1
    for bad in (PN[:2], PN[:, :1], PN[:, :, :2], PN[0], PN.reshape(3, 6)):                    # (nchannels, tapsPerPhi, polyorder+1) only
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_pnfb(bad)
        assert e.value.code == 1
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_taps_farrow(H.astype(ct))
        assert e.value.code == 5
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_pnfb(PN.astype(ct))
        assert e.value.code == 5
    assert f._chan_farrow is None                                            # a refused call leaves nothing behind
    f.set_channel_taps_farrow(H)                                             # remembered, installed at bind
    assert f._chan_farrow[0] == "taps" and np.array_equal(f._chan_farrow[1], H) and f._chan_farrow[1] is not H and f._handle is None
    f.set_channel_taps_farrow(H[::-1])                                       # taps may change
    assert np.array_equal(f._chan_farrow[1], H[::-1])
    f.set_channel_pnfb(PN)                                                   # the later call replaces the earlier one
    assert f._chan_farrow[0] == "pnfb" and np.array_equal(f._chan_farrow[1], PN) and f._chan_farrow[1].dtype == np.float64 and f._chan_farrow[1] is not PN
    assert f._chan_taps is None and f._bank is None
    for g in (pkg.FIRFilter(h, 1.5, 4, 2), pkg.FIRFilter.per_channel_farrow(H, 1.5, 4, 2), pkg.FIRFilter.per_channel_rates(h, rates, 4),
              pkg.FIRFilter(h, 1.5, 4)):                                     # not a filter of per_channel_rates_farrow
        with pytest.raises(pkg.MultirateHIPError) as e:
            g.set_channel_taps_farrow(H)
        assert e.value.code == 1
        with pytest.raises(pkg.MultirateHIPError) as e:
            g.set_channel_pnfb(PN)
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates(h, rates, 4).set_channel_taps_farrow(H)
    assert "set_channel_taps" in str(e.value)                                # FIRArbitrary: pointed to its own call
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.set_channel_taps(H)                                                # set_channel_taps keeps refusing FIRFarrow with status 5
    assert e.value.code == 5
    # per_channel_taps_and_rates_farrow: the filter of per_channel_rates_farrow(H[0], ...) with the matrix behind it
    g = pkg.FIRFilter.per_channel_taps_and_rates_farrow(H, rates, 4, 2)
    assert g.kind == pkg.host.FARROW and g.Nphi == 4 and g.polyorder == 2 and g.tapsPerPhi == 2 and g.historyLen == 1 and np.array_equal(g.h, H[0])
    assert g._chan_farrow[0] == "taps" and np.array_equal(g._chan_farrow[1], H) and np.array_equal(g._rates, rates) and g._bank is None and g.rate == 2.123
    d = pkg.FIRFilter.per_channel_taps_and_rates_farrow(np.ones((3, 250), dtype=np.float32), rates)
    assert d.Nphi == 32 and d.polyorder == 4                                 # the defaults
    assert [(s.rate, s.phiAccumulator, s.inputDeficit) for s in g.channel_states] == [(r, 1.0, 1) for r in rates]
    p = pkg.FIRFilter.per_channel_taps_and_rates_farrow(H, rates, 4, 2, pnfb=PN)
    assert p._chan_farrow[0] == "pnfb" and np.array_equal(p._chan_farrow[1], PN) and p._pnfb_in is not None and p._pnfb_in.shape == (2, 3)
    for bad_H, bad_rates, kw, code in ((H, rates[:2], {}, 1), (H[0], rates, {}, 1), (H, [1.0, 0.0, 2.0], {}, 1), (H, [], {}, 1),
                                       (H.astype(np.complex64), rates, {}, 5), (np.ones((3, 0), dtype=np.float32), rates, {}, 1),
                                       (H, rates, {"pnfb": PN[:2]}, 1), (H, rates, {"pnfb": PN[0]}, 1)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_taps_and_rates_farrow(bad_H, bad_rates, 4, 2, **kw)
        assert e.value.code == code, (bad_H.shape, bad_rates, kw)
    for Nphi, P in ((32, None), (32, -1), (32, 33), (4, 4)):                 # polyorder: the checks of per_channel_rates_farrow
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_taps_and_rates_farrow(H, rates, Nphi, P)
        assert e.value.code == 1


def test_the_older_constructors_and_set_channel_taps_keep_their_answers(pkg):
    h = np.arange(30, dtype=np.float64)
    f = pkg.FIRFilter.per_channel_rates_farrow(h, [0.47, 1.0, 2.123], 4, 3)
    assert f._chan_farrow is None and f._chan_taps is None and f._bank is None and f.kind == pkg.host.FARROW and f.tapsPerPhi == 8 and f.historyLen == 7
    assert [(s.rate, s.delta, s.phiAccumulator, s.alpha, s.phiIdx, s.inputDeficit, s.xIdx, s.last_count) for s in f.channel_states] == \
        [(r, 4 / r, 1.0, 0.0, 1, 1, 1, 0) for r in (0.47, 1.0, 2.123)]
    H = np.ones((3, 8), dtype=np.float32)
    one, bank, arb = pkg.FIRFilter(H[0], 2.123, 4, 2), pkg.FIRFilter.per_channel_farrow(H, 1.5, 4, 2), pkg.FIRFilter.per_channel_rates(H[0], [1.0, 2.0, 3.0], 4)
    for g in (one, bank, arb):
        assert g._chan_farrow is None
    arb.set_channel_taps(H)                                                  # the FIRArbitrary call is what it was
    assert np.array_equal(arb._chan_taps, H) and arb._chan_farrow is None
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates_farrow(H[0], [1.0, 2.0, 3.0], 4, 2).set_channel_taps(H)
    assert e.value.code == 5 and "FIRFarrow" in str(e.value)
    src = open(os.path.join(CSRC, "host_logic.cpp")).read()
    assert 'MRHIP_ERR_UNSUPPORTED, "mrhip_set_channel_taps: FIRFarrow' in src   # the C call's answer for a FIRFarrow filter: status 5, "FIRFarrow"


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_farrow\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_rates_farrow\.hip\.o.*:.*\bvariant_device\.h\b.*\brates_arb\.h\b", mk, flags=re.M)
    assert "kernels_rates_bank_farrow" not in mk and "rates_farrow_device" not in mk      # no second unit, no header for two
    assert not os.path.exists(os.path.join(CSRC, "kernels_rates_bank_farrow.hip")) and not os.path.exists(os.path.join(CSRC, "rates_farrow_device.h"))
    src = open(os.path.join(CSRC, UNIT)).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src and '#include "rates_arb.h"' in src and "#include \"rates_farrow_device.h\"" not in src
    assert "RealTaps<TX, R, NCX, FUSED>" in src
    assert "farrow_bank_horner<PP, 1>" in src and "typedef" not in src and "kFarrowBankUnrolledP =" not in src
    assert "tile_run(" in src and "bank_tile<true>(" in src and "farrow_rates_live_slots(" in src
    # both kernels end with the epilogue, ragged and plain, and no return stands in front of it
    assert src.count("shiftin_by_last_workgroup") == 2 and src.count("shiftin_ragged_by_last_workgroup") == 2
    for kernel in ("farrow_rates_generic_kernel(FarrowArgs a, RatesArgs r)", "farrow_rates_multi_kernel(FarrowArgs a, RatesArgs r, ArbTileArgs ta)"):
        body = src.split(kernel)[1].split("dev::shiftin_by_last_workgroup")[0]
        assert "dev::shiftin_ragged_by_last_workgroup" in body and not re.search(r"\breturn;", body), kernel
    assert "fma(" not in src                                                 # Horner is never fused; the dot's fma is RealTaps' (mac)
    assert "asm" not in src                                                  # plain HIP
    assert not re.search(r"\bwhile\s*\(", src) and "atomic" not in src.lower()      # no waits between workgroups, no spin loops, no atomics
    assert "__syncthreads" not in src and "__shared__" not in src            # no LDS staging (not measured ahead of plain reads)
    assert '"farrow_rates_bank_generic"' in src and '"farrow_rates_bank_multi"' in src and not re.search(r'"[a-z_]+_kernel"', src)
    # BANK is the kernels' last template argument and stands at the ONE statement a kernel that differs: the bank base of the channel
    assert src.count("template <typename TX, typename R, int NCX, bool FUSED, bool BANK>\n__global__") == 1
    assert src.count("template <typename TX, typename R, int NCX, bool FUSED, int OPL, bool BANK>\n__global__") == 1
    assert src.count("ch * bank_elems") == 2 and src.count("if constexpr (BANK) pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + ch * bank_elems;") == 2
    assert src.count("if constexpr (") - src.count("if constexpr (PP >= 0)") == 2


def test_the_horner_chains_and_the_dots_are_stated_once():
    src = open(os.path.join(CSRC, UNIT)).read()
    for text in ("void farrow_rates_horner(", "void farrow_rates_dots(", "R farrow_rates_round("):
        assert src.count(text) == 1, text
        others = [f for f in os.listdir(CSRC) if f != UNIT and os.path.isfile(os.path.join(CSRC, f)) and f.endswith((".hip", ".h", ".inc", ".cpp"))]
        assert others and not [f for f in others if text in open(os.path.join(CSRC, f)).read()], text
    # one kernel text for both bank keys: the dots are called once per polyorder path
    assert src.count("farrow_rates_dots<A, kFarrowBankUnrolledP, OPL>(") == 1 and src.count("farrow_rates_dots<A, -1, OPL>(") == 1
    assert "farrow_rates_round<R>(" in src
    # (was: the sibling's launches refuse a bank key, the new ones a filter without banks.)  The key is the selector: TypeKey::bank is read
    # in ONE function of the unit, which gives the kernels' BANK argument, the reported names and the switches of that key together
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    key = code.split("static RatesKey rates_key(const TypeKey &tk)")[1].split("\n}\n")[0]
    assert code.count("tk.bank") == key.count("tk.bank") == 5
    assert 'RatesKey{tk.bank, tk.bank ? "farrow_rates_bank_generic" : "farrow_rates_generic", tk.bank ? "farrow_rates_bank_multi" : "farrow_rates_multi",' in key
    assert 'tk.bank ? MRHIP_ENV_INT("MRHIP_FARROW_RATES_BANK_MULTI", -1) : MRHIP_ENV_INT("MRHIP_FARROW_RATES_MULTI", -1)' in key
    assert 'tk.bank ? MRHIP_ENV_INT("MRHIP_FARROW_RATES_BANK_GRID", 0) : MRHIP_ENV_INT("MRHIP_FARROW_RATES_GRID", 0)' in key
    assert code.count("MRHIP_ENV_INT(") == 4                                  # the four switches, each a literal name at a site of its own
    assert code.count("dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>()") == 3 and "dispatch_variant(" not in code
    assert code.count("*kname = key.generic;") == 1 and code.count("*kname = key.tiled;") == 1 and code.count("*kname = ") == 2
    assert "rates_key(tk).tiled_mode" in code and code.count("key.grid_fixed") == 1
    assert "if (tk.complex_h || a.dyn) return hipErrorInvalidValue;" in code and "if (tk.complex_h) return hipErrorInvalidValue;" in code
    assert "if (tk.complex_h || a.dyn || grid < 1 || ta.tile_out != static_cast<long long>(kFarrowRatesOPL) * kVariantThreads)" in code
    assert "farrow_rates_bank_generic_kernel" not in src and "farrow_rates_bank_multi_kernel" not in src      # no second kernel, no wrapper
    api = open(os.path.join(CSRC, "api.hip")).read()
    calls = api.split("static int rates_call(")[1].split("\nint mrhip_filt_device_rates(")[0]
    assert not re.search(r"_rates_bank_(generic|tiled|multi)\(", calls)      # the launches take either key
    assert calls.index("if (bound > 0 && !f->force_generic && farrow)") < calls.index("} else if (bound > 0 && !f->force_generic)")    # two plan branches
    assert calls.count("force_generic") == 2 and calls.count("MRHIP_CHECK_HIP(launch_") == 5            # ... the schedule and four filter launches
    assert calls.index("prepare_farrow_rates_multi(") < calls.index("launch_rates_schedule(") < calls.index("launch_farrow_rates_multi(")   # what can fail: before the state moves


def test_rates_bank_farrow_kernels_use_no_scratch(pkg):
    obj = os.path.join(CSRC, "build", UNIT + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in (UNIT, "variant_device.h", "ctaps_device.h", "rates_arb.h"))
    if os.path.getmtime(obj) < newest:
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel in ("farrow_rates_generic_kernel", "farrow_rates_multi_kernel"):  # 12 with BANK true beside the 12 with BANK false, none spilling
        _assert_rates_filter_kernel(sizes, kernel)


# ---- the plan and the argument checks, through one stand-alone program ------------------------------------------------------------
# a plan row: x_f64 r_f64 complex_x complex_h bank T polyorder n_out nch num_cus mode chip_grid grid_fixed count
XF64, RF64, CX, CH, BANK, T, P, NOUT, NCH, CUS, MODE, CHIP, FIXED, COUNT = range(14)
# the default rule (mode -1), from the measured rows (profiles/r13/farrow_rates_bank.txt): the multi kernel beat the
# universal one by more than the spread of the repeats at 4096 ch x 1e4 only (22 tiles a channel, 90 112 tiles)
RULE_MIN_TILES, RULE_MAX_PER_CHANNEL = 90_112, 22
SHARED_RULE = (90_112, 22)             # ... and over the one bank: the rule of a row without a bank key


def _expected(r):
    """from the stated formulas, the limits of the default rule by the row's bank key (with or without a bank per channel); a tile is OPL runs of 256 outputs of one channel, the tiling goes by
    n_out (the call's bound); the default rule (mode -1) as DESIGN.md 9 item 22 derives it (None: never); the grid is what the chip holds,
    at most a workgroup a tile, at least one, or a test's replacement (at most 65535).  Lane tid of the tile at k0 owns outputs
    k0 + tid + 256 j: those below the count are live."""
    refused = [0] * (7 + OPL + 1)
    min_tiles, max_per_channel = (RULE_MIN_TILES, RULE_MAX_PER_CHANNEL) if r[BANK] else SHARED_RULE
    if r[MODE] == 0 or r[CH] or r[NOUT] < 1 or r[T] < 1 or r[P] < 0 or r[NCH] < 1:
        return refused
    tile = OPL * LANES
    tpc = -(-r[NOUT] // tile)
    total = tpc * r[NCH]
    if r[MODE] != 1 and (min_tiles is None or total < min_tiles or tpc > max_per_channel):
        return refused
    grid = min(r[FIXED], 65535) if r[FIXED] > 0 else max(min(r[CHIP], total), 1)
    k0 = max([tau * tile for tau in range(tpc) if tau * tile < r[COUNT]], default=0)
    lanes = [0] * (OPL + 1)
    for tid in range(LANES):
        lanes[sum(1 for j in range(OPL) if k0 + tid + LANES * j < r[COUNT])] += 1
    return [1, 1, tile, tpc, total, grid, k0] + lanes


def _rows():
    base = [0, 0, 0, 0, 1, 8, 4, 2189, 3, 256, 1, 2048, 0, 1030]
    rows, why = [], []

    def add(name, **change):
        row = list(base)
        for k, v in change.items():
            row[globals()[k]] = v
        rows.append(row), why.append(name)

    add("1030 samples at rate 1.0: the count ends just inside the second span")       # bound ceil(1030 * 2.123) + 2, three spans
    add("2100 samples at 0.47: three live slots of four", NOUT=4461, COUNT=988)
    add("2100 samples at 2.123: two and one", NOUT=4461, COUNT=4459)
    add("a count of zero", COUNT=0)
    add("a count on a span's edge", COUNT=1024)
    add("one output", NOUT=1, NCH=1, COUNT=1)
    add("fewer tiles than workgroups", NOUT=1500, NCH=4, CHIP=2048)
    add("more tiles than workgroups", NOUT=22_502, NCH=4096, CHIP=2048)
    add("a chip that reports nothing", CHIP=0)
    for fixed in (1, 2, 3, 2000, 100_000):
        add("a test's grid", FIXED=fixed)
    for xf64, rf64 in ((0, 1), (1, 1)):
        for cx in (0, 1):
            add("every type", XF64=xf64, RF64=rf64, CX=cx)
    add("polyorder 0", P=0)
    for mode in (-1, 0, 1):
        add(f"mode {mode}", MODE=mode)                                                 # (mode -1: nine tiles)
        add("many short channels", MODE=mode, NOUT=22_502, NCH=4096, COUNT=22_500)     # 22 x 4096 = 90 112 tiles
        add("long channels", MODE=mode, NOUT=225_002, NCH=256, COUNT=225_000)          # 220 x 256 tiles
        add("few long channels", MODE=mode, NOUT=2_250_002, NCH=64, COUNT=2_125_000)   # 2198 x 64 tiles
        if RULE_MIN_TILES is not None:
            nch = -(-RULE_MIN_TILES // RULE_MAX_PER_CHANNEL)
            add("at both limits", MODE=mode, NOUT=RULE_MAX_PER_CHANNEL * 1024, NCH=nch, COUNT=1)
            add("a channel fewer", MODE=mode, NOUT=RULE_MAX_PER_CHANNEL * 1024, NCH=nch - 1, COUNT=1)
            add("a tile a channel more", MODE=mode, NOUT=RULE_MAX_PER_CHANNEL * 1024 + 1, NCH=nch, COUNT=1)
    for name, change in (("n_out < 1", {"NOUT": 0}), ("T < 1", {"T": 0}), ("polyorder < 0", {"P": -1}), ("no channel", {"NCH": 0}),
                         ("complex taps", {"CH": 1}), ("shared taps", {"BANK": 0})):
        add(name, **change)
    return rows, why


F32, F64, C64, C128 = range(4)
TAPS, PNFB = 0, 1
# (pnfb_call, is_rates, is_farrow, src_is_null, len, polyorder, tap_dtype, filter_len, filter_polyorder, filter_tap_dtype) -> (status, a
# piece of the message): the header's contract, in its order -- the filter first, then h / pnfb, then hLen or (tapsPerPhi, polyorder),
# then (mrhip_set_channel_taps_farrow) the tap type: out of range, complex, the other real one.  len: hLen or tapsPerPhi.
ARGS_TABLE = [
    ((TAPS, 1, 1, 0, 250, 4, F32, 250, 4, F32), (0, "")),
    ((TAPS, 1, 1, 0, 250, 4, F64, 250, 4, F64), (0, "")),
    ((TAPS, 1, 1, 0, 1, 0, F32, 1, 0, F32), (0, "")),
    ((PNFB, 1, 1, 0, 8, 4, F32, 8, 4, F32), (0, "")),
    ((PNFB, 1, 1, 0, 8, 4, F64, 8, 4, F64), (0, "")),
    ((TAPS, 1, 0, 0, 250, 4, F32, 250, 4, F32), (1, "mrhip_set_channel_taps_farrow: a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_taps")),
    ((PNFB, 1, 0, 0, 8, 4, F32, 8, 4, F32), (1, "mrhip_set_channel_pnfb: a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_taps")),
    ((TAPS, 1, 0, 1, 3, 4, C64, 250, 4, F32), (1, "takes mrhip_set_channel_taps")),                    # (whatever else is wrong)
    ((TAPS, 0, 1, 0, 250, 4, F32, 250, 4, F32), (1, "mrhip_set_channel_taps_farrow takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb")),
    ((TAPS, 0, 0, 0, 250, 4, F32, 250, 4, F32), (1, "mrhip_set_channel_taps_farrow takes a filter of mrhip_create_farrow_rates")),
    ((PNFB, 0, 1, 0, 8, 4, F32, 8, 4, F32), (1, "mrhip_set_channel_pnfb takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb")),
    ((PNFB, 0, 0, 1, 7, 3, F32, 8, 4, F32), (1, "mrhip_set_channel_pnfb takes a filter of mrhip_create_farrow_rates")),
    ((TAPS, 1, 1, 1, 250, 4, F32, 250, 4, F32), (1, "mrhip_set_channel_taps_farrow: h is NULL")),
    ((TAPS, 1, 1, 1, 3, 4, C64, 250, 4, F32), (1, "h is NULL")),
    ((PNFB, 1, 1, 1, 8, 4, F32, 8, 4, F32), (1, "mrhip_set_channel_pnfb: pnfb is NULL")),
    ((PNFB, 1, 1, 1, 7, 3, F32, 8, 4, F32), (1, "pnfb is NULL")),
    ((TAPS, 1, 1, 0, 249, 4, F32, 250, 4, F32), (1, "mrhip_set_channel_taps_farrow: hLen")),
    ((TAPS, 1, 1, 0, 251, 4, F32, 250, 4, F32), (1, "hLen")),
    ((TAPS, 1, 1, 0, 0, 4, F32, 250, 4, F32), (1, "hLen")),
    ((TAPS, 1, 1, 0, 249, 4, C64, 250, 4, F32), (1, "hLen")),
    ((TAPS, 1, 1, 0, 249, 4, 9, 250, 4, F32), (1, "hLen")),
    ((PNFB, 1, 1, 0, 7, 4, F32, 8, 4, F32), (1, "mrhip_set_channel_pnfb: tapsPerPhi and polyorder")),
    ((PNFB, 1, 1, 0, 9, 4, F32, 8, 4, F32), (1, "tapsPerPhi and polyorder")),
    ((PNFB, 1, 1, 0, 8, 3, F32, 8, 4, F32), (1, "tapsPerPhi and polyorder")),
    ((PNFB, 1, 1, 0, 8, 5, F32, 8, 4, F32), (1, "tapsPerPhi and polyorder")),
    ((PNFB, 1, 1, 0, 0, -1, F32, 8, 4, F32), (1, "tapsPerPhi and polyorder")),
    ((TAPS, 1, 1, 0, 250, 4, -1, 250, 4, F32), (1, "mrhip_set_channel_taps_farrow: bad tap dtype")),
    ((TAPS, 1, 1, 0, 250, 4, 4, 250, 4, F32), (1, "bad tap dtype")),
    ((TAPS, 1, 1, 0, 250, 4, C64, 250, 4, F32), (5, "mrhip_set_channel_taps_farrow: complex taps with per-channel rates are left out")),
    ((TAPS, 1, 1, 0, 250, 4, C128, 250, 4, F64), (5, "complex taps with per-channel rates are left out")),
    ((TAPS, 1, 1, 0, 250, 4, F64, 250, 4, F32), (1, "mrhip_set_channel_taps_farrow: the taps must have the filter's tap dtype")),
    ((TAPS, 1, 1, 0, 250, 4, F32, 250, 4, F64), (1, "the filter's tap dtype")),
]


def test_the_plan_of_the_multi_kernel_and_the_argument_checks(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "farrow_rates_bank_plan_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "farrow_rates_bank_plan_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows, why = _rows()
    want = [_expected(r) for r in rows]
    named = lambda name: [w for w, n in zip(want, why) if n == name]
    # the pinned shapes, written out: ok cpl tile_out tiles_per_channel total_tiles grid k0, lanes with 0 .. 4 live slots
    assert named("1030 samples at rate 1.0: the count ends just inside the second span") == [[1, 1, 1024, 3, 9, 9, 1024, 250, 6, 0, 0, 0]]
    assert named("2100 samples at 0.47: three live slots of four") == [[1, 1, 1024, 5, 15, 15, 0, 0, 0, 0, 36, 220]]
    assert named("2100 samples at 2.123: two and one") == [[1, 1, 1024, 5, 15, 15, 4096, 0, 149, 107, 0, 0]]
    assert named("a count of zero") == [[1, 1, 1024, 3, 9, 9, 0, 256, 0, 0, 0, 0]]
    assert named("a count on a span's edge") == [[1, 1, 1024, 3, 9, 9, 0, 0, 0, 0, 0, 256]]
    assert named("one output") == [[1, 1, 1024, 1, 1, 1, 0, 255, 1, 0, 0, 0]]
    assert named("fewer tiles than workgroups") == [[1, 1, 1024, 2, 8, 8, 1024, 250, 6, 0, 0, 0]]
    assert named("more tiles than workgroups")[0][3:6] == [22, 22 * 4096, 2048]
    assert named("a chip that reports nothing")[0][5] == 1
    assert [w[5] for w in named("a test's grid")] == [1, 2, 3, 2000, 65535]
    rule = lambda name: [(r[MODE], w) for r, w, n in zip(rows, want, why) if n == name]
    for name in ("many short channels", "long channels", "few long channels"):
        assert len(rule(name)) == 3 and all(w[0] for m, w in rule(name) if m == 1) and not any(w[0] for m, w in rule(name) if m == 0), name
    if RULE_MIN_TILES is None:                                              # never: mode -1 is mode 0
        assert not any(w[0] for r, w in zip(rows, want) if r[MODE] == -1)
    else:                                                                   # the default rule from both sides of both limits
        assert all(w[0] == (m != 0) for m, w in rule("at both limits")) and len(rule("at both limits")) == 3
        assert all(w[3] == RULE_MAX_PER_CHANNEL and w[4] >= RULE_MIN_TILES > w[4] - w[3] for _, w in rule("at both limits") if w[0])
        for name in ("a channel fewer", "a tile a channel more"):
            assert all(w[0] == (m == 1) for m, w in rule(name)) and len(rule(name)) == 3, name
        assert [w[3:5] for m, w in rule("many short channels") if m == -1] == [[22, 90_112]]          # the measured row the multi kernel won
        assert not any(w[0] for m, w in rule("long channels") + rule("few long channels") if m == -1)  # ... and the two it did not
    assert named("mode 1")[0][0] == 1
    for name in ("mode 0", "n_out < 1", "T < 1", "polyorder < 0", "no channel", "complex taps"):
        assert named(name) and all(not w[0] for w in named(name)), name
    # shared taps are no refusal: the plan of the one-bank kernel, the same tiling (the base row, whose mode is 1)
    assert named("shared taps") == named("mode 1") and named("shared taps")[0][0] == 1 and [r[BANK] for r, n in zip(rows, why) if n == "shared taps"] == [0]
    assert all(w[0] for w in named("every type") + named("polyorder 0"))
    text = "".join("plan " + " ".join(str(v) for v in r) + "\n" for r in rows)
    text += "".join("args " + " ".join(map(str, args)) + "\n" for args, _ in ARGS_TABLE)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows) + len(ARGS_TABLE)
    have = [[int(v) for v in line.split()] for line in lines[:len(rows)]]
    differing = [(n, r, h, w) for n, r, h, w in zip(why, rows, have, want) if h != w]
    assert not differing, differing[:5]
    for (args, (status, piece)), line in zip(ARGS_TABLE, lines[len(rows):]):
        got_status, _, message = line.partition(" ")
        assert int(got_status) == status, (args, line)
        assert (piece in message) if status else message == "", (args, line)
