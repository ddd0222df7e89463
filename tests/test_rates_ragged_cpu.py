"""CPU-only checks of per-channel input lengths for the filters with per-channel rates (mrhip_filt_device_rates_ragged; FIRFilter.filt /
filt_into with ``lengths``): the symbol in the header, host.ABI, the library's exports and the Julia shim; the pure length checks
(csrc/host_logic.cpp: check_ragged_lengths) and the history index rule of the ragged shiftin! (csrc/rates_arb.h: rates_hist_source, the
text the kernels' epilogue runs) through the stand-alone program tests/rates_ragged_check.cpp, built with -fsanitize=address,undefined;
the serial walk with per-channel lengths against the oracle, by the program tests/test_rates_arb_cpu.py builds from the shared step; the
shape of the touched device code (no new spin loop, atomic, inline assembly), and no scratch memory or AccVGPRs in the gfx950 code
objects of the two touched kernel units."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _assert_rates_filter_kernel, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mrhip_filt_device_rates_ragged"
# the sequence of ragged calls of tests/test_gpu_rates_ragged.py: rates, the lengths of the five calls and the counts the oracle gives
R4 = [0.01, 32.0 / 3, 2.123, 2.123]
CALLS = [[257, 0, 5, 257], [3, 300, 0, 7], [1500, 1, 257, 2], [0, 0, 0, 0], [100, 100, 100, 100]]
COUNTS = [[3, 0, 11, 546], [0, 3200, 0, 15], [15, 11, 546, 4], [0, 0, 0, 0], [1, 1067, 212, 213]]


def test_the_symbol_is_in_the_header_the_binding_table_the_exports_and_the_shim(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, NAME)
    assert [a for n, _, a in pkg.host.ABI if n == NAME] == [[pkg.host._vp, pkg.host._vp, pkg.host._vp, pkg.host._i64, pkg.host._vp, pkg.host._i64,
                                                             pkg.host._i64, pkg.host._vp, pkg.host._vp]]
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_filt_device_rates_ragged\(mrhip_filter \*f, const void \*x, const int64_t \*x_lens /\* HOST, \[nchannels\] \*/, "
                     r"int64_t x_stride,\s*void \*y, int64_t y_capacity, int64_t y_stride, int64_t \*counts_out, void \*stream\);", hdr)
    assert "FOUR pinned staging slots" in hdr                                # the number of slots is stated
    assert re.search(r"constexpr int kRatesRaggedSlots = 4;", open(os.path.join(CSRC, "mrhip_filter.h")).read())
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    assert re.search(r"ccall\(\(:mrhip_filt_device_rates_ragged, libmr\), Cint,\s*"
                     r"\(Ptr\{Cvoid\}, Ptr\{Cvoid\}, Ptr\{Int64\}, Int64, Ptr\{Cvoid\}, Int64, Int64, Ptr\{Int64\}, Ptr\{Cvoid\}\)", jl)
    assert "function filt!(Y::Matrix, f::RatesFIRFilter, X::Matrix, lengths::Vector{<:Integer})" in jl
    assert re.search(r"^function filt\(f::RatesFIRFilter\{Th\}, X::Matrix\{Tx\}, lengths::Vector\{<:Integer\}\)", jl, flags=re.M)
    # no new constructor, and the older call keeps its declaration
    assert len(set(re.findall(r"\b(mrhip_create_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))) == 16
    assert "int mrhip_filt_device_rates(mrhip_filter *f, const void *x, int64_t x_len, int64_t x_stride," in hdr


def test_lengths_on_any_other_filter_is_an_argument_error(pkg):
    f = pkg.FIRFilter(np.ones(8, dtype=np.float32), 1.5)
    x = np.zeros(16, dtype=np.float32)
    for call in (lambda: f.filt(x, lengths=[16]), lambda: f.filt_into(np.zeros(40, dtype=np.float32), x, lengths=[16])):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == 1 and "per_channel_rates" in str(e.value)


@pytest.fixture(scope="module")
def ragged_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rates_ragged_check") / "rates_ragged_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "rates_ragged_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


BIG = 2 ** 31 - 1
# (nch, x is NULL, x_stride, x_lens is NULL, lengths) -> (status, len_max or -1, a word of the message)
LENGTH_CASES = [
    ((4, 0, 1500, 0, [257, 0, 5, 257]), (0, 257, "")),
    ((4, 0, 257, 0, [257, 0, 5, 257]), (0, 257, "")),                        # the stride may equal the largest length
    ((4, 0, 0, 0, [0, 0, 0, 0]), (0, 0, "")),                                # an all-empty call
    ((4, 1, 0, 0, [0, 0, 0, 0]), (0, 0, "")),                                # ... needs no x
    ((1, 0, 0, 0, [1500]), (0, 1500, "")),                                   # one channel: the stride is not looked at
    ((3, 0, BIG, 0, [BIG - 1, 0, 1]), (0, BIG - 1, "")),                     # the largest length a call takes
    ((4, 0, 1500, 1, [1, 1, 1, 1]), (1, -1, "x_lens is NULL")),
    ((4, 1, 1500, 1, [1, 1, 1, 1]), (1, -1, "x_lens is NULL")),              # ... comes first
    ((4, 0, 1500, 0, [257, -1, 5, 257]), (1, -1, "negative length")),
    ((4, 0, 1500, 0, [257, 0, 5, -2 ** 62]), (1, -1, "negative length")),
    ((4, 0, 2 ** 40, 0, [257, 0, BIG, 257]), (5, -1, "fewer than 2^31-1 samples")),
    ((4, 0, 2 ** 40, 0, [2 ** 40, 0, 5, 257]), (5, -1, "fewer than 2^31-1 samples")),
    ((4, 0, 2 ** 40, 0, [BIG, -1, 5, 257]), (5, -1, "fewer than 2^31-1 samples")),   # the first offending channel answers
    ((4, 0, 2 ** 40, 0, [-1, BIG, 5, 257]), (1, -1, "negative length")),
    ((4, 1, 1500, 0, [0, 0, 1, 0]), (1, -1, "x is NULL")),
    ((4, 0, 256, 0, [257, 0, 5, 257]), (1, -1, "x_stride <")),
    ((4, 0, -1, 0, [0, 0, 0, 0]), (1, -1, "x_stride <")),
    ((4, 1, 0, 0, [0, 3, 0, 0]), (1, -1, "x is NULL")),                      # x before the stride
]


def test_the_pure_length_checks(ragged_check):
    text = "".join(f"{nch} {xn} {xs} {ln} " + " ".join(map(str, lens)) + "\n" for (nch, xn, xs, ln, lens), _ in LENGTH_CASES)
    p = subprocess.run([ragged_check], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(LENGTH_CASES)
    for (case, (status, len_max, word)), line in zip(LENGTH_CASES, lines):
        got_status, got_max, message = line.split(" | ", 2)
        assert (int(got_status), int(got_max)) == (status, len_max), (case, line)
        if status:
            assert NAME in message and word in message, (case, line)         # every refusal names the entry point
        else:
            assert message == "", (case, line)
    assert {s for _, (s, _, _) in LENGTH_CASES} == {0, 1, 5}


def test_the_history_index_rule_is_the_last_H_of_the_concatenation(ragged_check):
    p = subprocess.run([ragged_check, "history"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "history ok" and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    # ONE text of the rule: the kernels call it through the ragged fold, nothing restates it
    hdr = open(os.path.join(CSRC, "rates_arb.h")).read()
    assert hdr.count("rates_hist_source(long long i, long long len, int H)") == 1 and "MRHIP_RATES_HD inline HistSource rates_hist_source" in hdr
    for unit in ("kernels_rates_arb.hip", "kernels_rates_farrow.hip"):
        src = open(os.path.join(CSRC, unit)).read()
        assert src.count("dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{})") == 2, unit
        assert src.count("dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch)") == 2, unit


def test_the_walk_with_per_channel_lengths_gives_the_oracles_counts_and_states(O, tmp_path):
    """channel c of the sequence of ragged calls: the walk of tests/rates_step_check.cpp (the step the schedule kernel compiles) over
    the channel's own lengths, against the oracle's one-channel filter fed as many samples call after call"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rates_step_check")
    b = subprocess.run([cxx, "-std=c++20", "-O2", "-ffp-contract=off", "-w", "-I" + CSRC, os.path.join(ROOT, "tests", "rates_step_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    rows = [(Nphi, rate, [call[c] for call in CALLS]) for Nphi in (3, 32) for c, rate in enumerate(R4)]
    text = "".join(f"{Nphi} {rate!r} {len(ch)} " + " ".join(map(str, ch)) + "\n" for Nphi, rate, ch in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-500:], p.stderr[-2000:])
    lines = p.stdout.strip().splitlines()
    assert len(lines) == len(rows) * len(CALLS)
    at = 0
    for Nphi, rate, ch in rows:
        ref = O.FIRFilter(np.ones(Nphi, dtype=np.float32), float(rate), Nphi, tx=np.float32)       # (one tap per phase: the schedule alone)
        c = R4.index(rate) if R4.count(rate) == 1 else None
        for i, n in enumerate(ch):
            before = ref.state
            y, sc = ref.filt(np.zeros(n, dtype=np.float32), return_schedule=True)
            v = [int(t) for t in lines[at].split()]
            at += 1
            st = ref.state
            assert v[0] == len(y), (Nphi, rate, i)
            assert (v[1], v[2], v[3]) == (st.inputDeficit, st.xIdx, np.array([st.phiAccumulator]).view(np.uint64)[0]), (Nphi, rate, i)
            assert np.array_equal(np.array(v[4::2], dtype=np.int64), sc["xIdx"]), (Nphi, rate, i)
            if n == 0:                                                       # a zero-length channel keeps its state
                assert (st.inputDeficit, st.xIdx, st.phiAccumulator) == (before.inputDeficit, before.xIdx, before.phiAccumulator)
            if Nphi == 32 and c is not None:
                assert v[0] == COUNTS[i][c], (rate, i)
    # the counts of the GPU module's sequence (N𝜙 32), all four channels
    refs = [O.FIRFilter(np.ones(32, dtype=np.float32), float(r), 32, tx=np.float32) for r in R4]
    assert [[len(r.filt(np.zeros(n, dtype=np.float32))) for r, n in zip(refs, call)] for call in CALLS] == COUNTS


def test_the_touched_device_code_is_plain_hip():
    """no new spin loop, atomic, inline assembly: the two kernel units hold none at all, and the ragged fold in pair_device.h -- the
    text between its template line and the next function -- none either (it elects the grid's last workgroup by index)"""
    for unit in ("kernels_rates_arb.hip", "kernels_rates_farrow.hip"):
        src = open(os.path.join(CSRC, unit)).read()
        assert "asm" not in src and "__hip_atomic" not in src and "atomic" not in src and not re.search(r"\bwhile\s*\([^)]*(volatile|ld_sc1)", src), unit
        assert "rates_channel_len(" in src or unit == "kernels_rates_farrow.hip"
    pd = open(os.path.join(CSRC, "pair_device.h")).read()
    m = re.search(r"template <typename TX, int NC, typename Source>\n__device__ __forceinline__ void shiftin_ragged_by_last_workgroup\(.*?\n}\n", pd, flags=re.S)
    assert m, "the ragged fold"
    body = m.group(0)
    assert "asm" not in body and "atomic" not in body and "__syncthreads" not in body and "while" not in body and "__shared__" not in body
    assert "blockIdx.x + 1u != gridDim.x || blockIdx.y != 0u || blockIdx.z != 0u" in body
    # the existing fold is as it was: the counting form and the last-workgroup form
    assert "__hip_atomic_fetch_add(sf.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total - 1u" in pd
    arb = open(os.path.join(CSRC, "kernels_rates_arb.hip")).read()
    assert "const long long len = RAGGED ? rates_channel_len(s.x_lens, s.x_len, c) : s.x_len;" in arb      # the walk: the channel's own length
    assert "rates_walk<POW2, false>(s)" in arb and "rates_walk<POW2, true>(s)" in arb      # the old call keeps instantiations of its own
    assert "if (len < deficit)" in arb and "while (x <= len && count < s.slice)" in arb and "rec->inputDeficit = x - len;" in arb
    assert "stage_window(lx, xc, hc, w.o, static_cast<int>(w.span), len, a.H, tid)" in arb  # the tiled kernel stages up to the channel's end


# (a filter kernel's count: (instantiations over shared taps, over a bank per channel) -- BANK is its last template argument)
@pytest.mark.parametrize("unit,kernels", [
    ("kernels_rates_arb.hip", (("arb_rates_generic_kernel", (12, 12)), ("arb_rates_tiled_kernel", (12, 12)), ("rates_schedule_kernel", 2),
                               ("rates_ragged_schedule_kernel", 2), ("rates_reset_kernel", 1))),
    ("kernels_rates_farrow.hip", (("farrow_rates_generic_kernel", (12, 12)), ("farrow_rates_multi_kernel", (12, 12))))])
def test_the_touched_units_use_no_scratch_and_no_accvgprs(pkg, unit, kernels):
    obj = os.path.join(CSRC, "build", unit + ".o")
    assert os.path.exists(obj), "the build leaves its objects in csrc/build"
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "no llvm tools"
    sizes = _kernel_scratch(obj)
    for kernel, count in kernels:
        if isinstance(count, tuple):
            assert count[0] == count[1]
            _assert_rates_filter_kernel(sizes, kernel, each=count[0])
            continue
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"
