"""CPU-only checks of per-channel rates for FIRFarrow (FIRFilter.per_channel_rates_farrow, mrhip_create_farrow_rates,
mrhip_create_farrow_rates_pnfb, csrc/kernels_rates_farrow.hip) and of mrhip_set_channel_rates: the three exported symbols and their
declarations, the argument errors of the Python constructor and of set_channel_rates, the description of the unbound filter, the
answers the older constructors keep, the build conditions of the kernel unit, the instantiations in the object the build made (both
filter kernels for (Tx scalar, R) in {(f32,f32), (f32,f64), (f64,f64)} x real / complex samples x STRICT / FUSED = 12 each for the one
bank and 12 each for a bank per channel; none with scratch memory or AccVGPRs), and the host side of the multi kernel
(csrc/host_logic.cpp: plan_farrow_rates_multi, which takes either bank key, farrow_rates_multi_grid; csrc/rates_arb.h: farrow_rates_live_slots, which the kernel evaluates per lane) through a stand-alone program
built with -fsanitize=address,undefined, against values computed here from the stated formulas."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _assert_rates_filter_kernel, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mrhip_create_farrow_rates", "mrhip_create_farrow_rates_pnfb", "mrhip_set_channel_rates")
OPL, LANES = 4, 256


def test_the_library_exports_the_three_symbols_and_the_header_declares_them(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert len([1 for n, _, _ in pkg.host.ABI if n == name]) == 1, name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_create_farrow_rates\(const void \*h, int64_t hLen, int tap_dtype, const double \*rates, int64_t Nphi, int64_t polyorder,\s*"
                     r"int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)
    assert re.search(r"int mrhip_create_farrow_rates_pnfb\(const double \*pnfb, int64_t hLen, int tap_dtype, const double \*rates, int64_t Nphi,\s*"
                     r"int64_t polyorder, int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)
    assert re.search(r"int mrhip_set_channel_rates\(mrhip_filter \*f, const double \*rates /\* \[nchannels\] \*/\);", hdr)
    assert "Per-channel rates for FIRFarrow" in hdr
    assert "farrow_rates_generic and\n * farrow_rates_multi" in hdr          # said at mrhip_last_kernel_name
    assert "KEEPS the current rates" in hdr                                  # mrhip_reset on a filter whose rates were changed
    # the two names are reported without the suffix, and no string literal of the suffixed form is in the source
    src = open(os.path.join(CSRC, "kernels_rates_farrow.hip")).read()
    assert '"farrow_rates_generic"' in src and '"farrow_rates_multi"' in src and not re.search(r'"[a-z_]+_kernel"', src)
    # every entry point that carries one state or one count names both constructors
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert "(mrhip_create_arbitrary_rates, mrhip_create_farrow_rates), so a state and a count per" in api


def test_argument_errors_of_the_python_constructor(pkg):
    h = np.ones(64, dtype=np.float32)
    for bad in ([0.0], [1.0, -2.0], [1.0, 0.0, 2.0], [float("nan")], [float("inf")]):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates_farrow(h, bad)                   # "rate must be greater than 0", Filters.jl:184, anywhere in rates
        assert e.value.code == 1
    for bad in ([], [[1.0, 2.0]]):                                           # len(rates) == 0; not a vector
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates_farrow(h, bad)
        assert e.value.code == 1
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates_farrow(h.astype(ct), [1.5])      # complex taps: left out
        assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates_farrow(np.ones(0, dtype=np.float32), [1.5])
    assert e.value.code == 1
    for Nphi, P in ((32, None), (32, -1), (32, 33), (4, 4)):                 # polyorder: in 0..min(32, Nphi-1)
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates_farrow(h, [1.5], Nphi, P)
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates_farrow(h, [1.5], 32, 4, pnfb=np.ones((3, 5)))     # tapsPerPhi = 2
    assert e.value.code == 1
    assert pkg.FIRFilter.per_channel_rates_farrow(h, [1.5], 32, 4, pnfb=np.ones((2, 5)))._pnfb_in.shape == (2, 5)


def test_the_unbound_filter_describes_its_channels(pkg):
    h = np.arange(30, dtype=np.float64)
    f = pkg.FIRFilter.per_channel_rates_farrow(h, [0.47, 1.0, 2.123], 4, 3)
    assert f.kind == pkg.host.FARROW and f.polyorder == 3 and f.Nphi == 4 and f.tapsPerPhi == 8 and f.historyLen == 7
    assert f.numerics == pkg.NUMERICS_STRICT and f.rate == 2.123
    g = pkg.FIRFilter.per_channel_rates_farrow(h, [1.5])
    assert g.Nphi == 32 and g.polyorder == 4                                 # the defaults
    sts = f.channel_states
    assert [(s.rate, s.delta, s.phiAccumulator, s.alpha, s.phiIdx, s.inputDeficit, s.xIdx, s.last_count) for s in sts] == \
        [(r, 4 / r, 1.0, 0.0, 1, 1, 1, 0) for r in (0.47, 1.0, 2.123)]
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.state                                                              # ONE state: not on this filter
    assert e.value.code == 5 and "channel_states" in str(e.value)
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.set_channel_states([1, 1, 1], [1.0, 1.0, 1.0])                     # needs a bound filter
    assert e.value.code == 1
    # set_channel_rates on an unbound filter: the filter will be created at the new rates
    for bad in ([1.0, 2.0], [1.0, 0.0, 2.0], [1.0, float("inf"), 2.0], [[1.0, 2.0, 3.0]]):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.set_channel_rates(bad)
        assert e.value.code == 1
    f.set_channel_rates([3.5, 0.25, 1.0])
    assert f.rate == 3.5 and [(s.rate, s.delta) for s in f.channel_states] == [(3.5, 4 / 3.5), (0.25, 16.0), (1.0, 4.0)]
    a = pkg.FIRFilter.per_channel_rates(h, [0.5, 2.0], 4)                    # the FIRArbitrary filter too
    a.set_channel_rates([4.0, 2.0])
    assert a.rate == 4.0 and [s.rate for s in a.channel_states] == [4.0, 2.0]
    for shared in (pkg.FIRFilter(h, 1.5), pkg.FIRFilter(h, 1.5, 4, 3)):      # not a filter with per-channel rates
        with pytest.raises(pkg.MultirateHIPError) as e:
            shared.set_channel_rates([1.0])
        assert e.value.code == 1
        with pytest.raises(pkg.MultirateHIPError):
            shared.channel_states


def test_the_older_constructors_keep_their_answers(pkg):
    h = np.ones(64, dtype=np.float32)
    H = np.ones((3, 64), dtype=np.complex64)
    for rate in (-1.5, 0.0):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter(h, rate, 32, 4)
        assert e.value.code == 1
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_farrow(H.real.astype(np.float32), rate)
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter(H[0], 1.5, 32, 4)                                      # complex taps: complex_taps_farrow
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_farrow(H, 1.5)                             # complex taps: not through this constructor
    assert e.value.code == 5
    for bad in ([0.0], [], [[1.0, 2.0]]):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_rates(h, bad)                          # (its checks moved into a shared helper)
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_rates(h, [[1.0, 2.0]])
    assert "per_channel_rates takes one rate per channel" in str(e.value)
    one = pkg.FIRFilter(h, 2.123, 4, 3)
    st = one.state
    assert (st.kind, st.Nphi, st.tapsPerPhi, st.historyLen, st.rate, st.delta) == (pkg.host.FARROW, 4, 16, 15, 2.123, 4 / 2.123)
    assert one._rates is None and pkg.FIRFilter.per_channel_farrow(H.real.astype(np.float32), 1.5)._rates is None
    r = pkg.FIRFilter.per_channel_rates(h, [0.5, 2.0])
    assert r.kind == pkg.host.ARBITRARY and r.polyorder is None and list(r._rates) == [0.5, 2.0]


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_rates_farrow\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_rates_farrow\.hip\.o.*:.*\bvariant_device\.h\b.*\brates_arb\.h\b", mk, flags=re.M)
    src = open(os.path.join(CSRC, "kernels_rates_farrow.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src and '#include "rates_arb.h"' in src and "RealTaps<TX, R, NCX, FUSED>" in src
    # ONE text of the coefficient type and of the single Horner chain: the shared header's, not a copy
    assert "farrow_bank_horner<PP, 1>" in src and "typedef" not in src and "kFarrowBankUnrolledP =" not in src
    shared = open(os.path.join(CSRC, "variant_device.h")).read()
    assert "address_space(4))) double *farrow_coef_t;" in shared and "void farrow_bank_horner(" in shared
    assert "tile_run(" in src and "bank_tile<true>(" in src and "farrow_rates_live_slots(" in src and src.count("shiftin_by_last_workgroup") == 2
    assert "fma(" not in src                                                 # Horner is never fused; the dot's fma is RealTaps' (mac)
    assert "asm" not in src                                                  # plain HIP
    assert not re.search(r"\bwhile\s*\(", src) and "atomic" not in src       # no waits between workgroups, no spin loops, no atomics
    assert "__syncthreads" not in src and "__shared__" not in src            # no LDS staging (not measured ahead of plain reads)
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert api.count("launch_rates_reset(") == 1                             # the constructor state is FIRArbitrary's: ONE reset kernel


def test_rates_farrow_kernels_use_no_scratch(pkg):
    obj = os.path.join(CSRC, "build", "kernels_rates_farrow.hip.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in ("kernels_rates_farrow.hip", "variant_device.h", "ctaps_device.h", "rates_arb.h"))
    if os.path.getmtime(obj) < newest:
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel in ("farrow_rates_generic_kernel", "farrow_rates_multi_kernel"):  # 12 with BANK false and 12 with BANK true, none spilling
        _assert_rates_filter_kernel(sizes, kernel)


# ---- the host side of the multi kernel -----------------------------------------------------------------------------------------
# a row: x_f64 r_f64 complex_x complex_h bank T polyorder n_out nch num_cus mode chip_grid grid_fixed count
XF64, RF64, CX, CH, BANK, T, P, NOUT, NCH, CUS, MODE, CHIP, FIXED, COUNT = range(14)
# the default rule (mode -1) by the row's bank key, (from tiles, up to tiles a channel): the measured rows the multi kernel won over the
# one bank and over a bank per channel (item 22)
RULE = {0: (90_112, 22), 1: (90_112, 22)}


def _expected(r):
    """from the stated formulas, for either bank key: a tile is OPL runs of 256 outputs of one channel, the tiling goes by n_out (the
    call's bound); the default rule (mode -1) is the measured one of the row's bank key: from 90 112 tiles, up to 22 tiles a channel; the grid is what the chip holds, at most a workgroup a tile, at least one, or a
    test's replacement (at most 65535).  Lane tid of the tile at k0 owns outputs k0 + tid + 256 j: those below the count are live."""
    refused = [0] * (7 + OPL + 1)
    min_tiles, max_per_channel = RULE[r[BANK]]
    if r[MODE] == 0 or r[CH] or r[NOUT] < 1 or r[T] < 1 or r[P] < 0 or r[NCH] < 1:
        return refused
    tile = OPL * LANES
    tpc = -(-r[NOUT] // tile)
    total = tpc * r[NCH]
    if r[MODE] != 1 and (total < min_tiles or tpc > max_per_channel):
        return refused
    grid = min(r[FIXED], 65535) if r[FIXED] > 0 else max(min(r[CHIP], total), 1)
    k0 = max([tau * tile for tau in range(tpc) if tau * tile < r[COUNT]], default=0)
    lanes = [0] * (OPL + 1)
    for tid in range(LANES):
        lanes[sum(1 for j in range(OPL) if k0 + tid + LANES * j < r[COUNT])] += 1
    return [1, 1, tile, tpc, total, grid, k0] + lanes


def _rows():
    base = [0, 0, 0, 0, 0, 8, 4, 2189, 3, 256, 1, 2048, 0, 1030]
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
    add("a full span", NOUT=1024, COUNT=1024)
    add("one output", NOUT=1, NCH=1, COUNT=1)
    add("fewer tiles than workgroups", NOUT=1500, NCH=4, CHIP=2048)                    # 2 x 4 = 8 tiles on a chip that holds 2048
    add("more tiles than workgroups", NOUT=22_502, NCH=4096, CHIP=2048)
    add("a chip that reports nothing", CHIP=0)
    for fixed in (1, 3, 1000, 100_000):
        add("a test's grid", FIXED=fixed)
    for xf64, rf64 in ((0, 1), (1, 1)):
        for cx in (0, 1):
            add("every type", XF64=xf64, RF64=rf64, CX=cx)
    add("polyorder 0", P=0)
    for mode in (-1, 0, 1):
        add(f"mode {mode}", MODE=mode)                                                 # (mode -1: nine tiles, far below the rule)
        add("the smallest measured win", MODE=mode, NOUT=22_502, NCH=4096, COUNT=22_500)          # 22 x 4096 tiles
        add("a channel fewer", MODE=mode, NOUT=22_502, NCH=4095, COUNT=22_500)
        add("a tile a channel more", MODE=mode, NOUT=22_529, NCH=4096, COUNT=22_500)   # 23 a channel
        add("few long channels", MODE=mode, NOUT=2_250_002, NCH=64, COUNT=2_125_000)   # 2198 x 64 = 140 672 tiles
    for name, change in (("n_out < 1", {"NOUT": 0}), ("T < 1", {"T": 0}), ("polyorder < 0", {"P": -1}), ("no channel", {"NCH": 0}),
                         ("complex taps", {"CH": 1}), ("a bank", {"BANK": 1})):
        add(name, **change)
    return rows, why


def test_the_plan_of_the_multi_kernel(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "farrow_rates_plan_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "farrow_rates_plan_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
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
    assert [w[5] for w in named("a test's grid")] == [1, 3, 1000, 65535]
    rule = lambda name: [(r[MODE], w) for r, w, n in zip(rows, want, why) if n == name]
    assert all(w[0] == (m != 0) for m, w in rule("the smallest measured win")) and len(rule("the smallest measured win")) == 3
    assert all(w[3:5] == [22, 90_112] for _, w in rule("the smallest measured win") if w[0])
    for name in ("a channel fewer", "a tile a channel more", "few long channels"):      # the default rule from both sides of both limits
        assert all(w[0] == (m == 1) for m, w in rule(name)) and len(rule(name)) == 3, name
    assert named("mode 1")[0][0] == 1
    for name in ("mode -1", "mode 0", "n_out < 1", "T < 1", "polyorder < 0", "no channel", "complex taps"):
        assert named(name) and all(not w[0] for w in named(name)), name
    # a bank key is no refusal: the plan of the bank-per-channel kernel, the same tiling (the base row in mode 1)
    assert named("a bank") == named("mode 1") and named("a bank")[0][0] == 1 and [r[BANK] for r, n in zip(rows, why) if n == "a bank"] == [1]
    assert all(w[0] for w in named("every type") + named("polyorder 0"))
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    have = [[int(v) for v in line.split()] for line in p.stdout.strip().splitlines()]
    assert len(have) == len(rows)
    differing = [(n, r, h, w) for n, r, h, w in zip(why, rows, have, want) if h != w]
    assert not differing, differing[:5]
