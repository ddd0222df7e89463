"""CPU-only checks of input lengths from device memory, and chaining, for the filters with per-channel rates
(mrhip_filt_device_rates_lens_device, mrhip_filt_device_rates_chained; FIRFilter.filt_rates_async): the two symbols in the header,
host.ABI, the library's exports and the Julia shim; the pure checks of both calls (csrc/host_logic.cpp: check_device_lengths,
check_rates_chain) message by message, and the acceptance rule of a length the host never saw (csrc/rates_arb.h: rates_length_accepted,
the text the import kernel runs), through the stand-alone program tests/rates_device_lengths_check.cpp, built with
-fsanitize=address,undefined; what the Python method refuses without a GPU; the shape of the import kernel (plain HIP, guarded) and no
scratch memory or AccVGPRs in the gfx950 code object of the unit that holds it."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _assert_rates_filter_kernel, _kernel_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS, CHAINED = "mrhip_filt_device_rates_lens_device", "mrhip_filt_device_rates_chained"
SECTION = "Input lengths from device memory, and chaining, for the filters with per-channel rates"


def test_the_symbols_are_in_the_header_the_binding_table_the_exports_and_the_shim(pkg):
    lib, h = pkg.load_library(), pkg.host
    ten = [h._vp, h._vp, h._vp, h._i64, h._i64, h._vp, h._i64, h._i64, h._vp, h._vp]
    for name in (LENS, CHAINED):
        assert hasattr(lib, name), name
        assert [a for n, _, a in h.ABI if n == name] == [ten], name
        assert [r for n, r, _ in h.ABI if n == name] == [h._i], name
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_filt_device_rates_lens_device\(mrhip_filter \*f, const void \*x, const int64_t \*x_lens /\* DEVICE, \[nchannels\] \*/, "
                     r"int64_t x_len_max,\s+int64_t x_stride, void \*y, int64_t y_capacity, int64_t y_stride, int64_t \*counts_out, void \*stream\);", hdr)
    assert re.search(r"int mrhip_filt_device_rates_chained\(mrhip_filter \*f, const mrhip_filter \*prev, const void \*x, int64_t x_len_bound, "
                     r"int64_t x_stride,\s+void \*y, int64_t y_capacity, int64_t y_stride, int64_t \*counts_out, void \*stream\);", hdr)
    ragged = hdr.split("Per-channel input lengths for the filters with per-channel rates")[1].split("int mrhip_filt_device_rates_ragged")[0]
    assert "Since added" in ragged and LENS in ragged and CHAINED in ragged     # the older section points to what answers its "left out"
    block = hdr.split("/* " + SECTION)[1].split("int " + LENS)[0]
    for left_out in ("graph capture", "compacting the tiles", "BEHIND a filter with per-channel rates", "mrhip_cascade_*, rings and sharding",
                     "parallel\n *     schedule for long channels"):
        assert left_out in block.split("left out on purpose")[1], left_out
    assert "between that call of prev and prev's next one" in block          # how long the records hold the counts
    assert "No pinned staging slot" in block
    # no new constructor; the older calls keep their declarations and what they say about themselves
    assert len(set(re.findall(r"^int (mrhip_create_\w+)\(", hdr, flags=re.M))) == 16
    assert "int mrhip_filt_device_rates_ragged(mrhip_filter *f, const void *x, const int64_t *x_lens /* HOST, [nchannels] */, int64_t x_stride," in hdr
    assert "FOUR pinned staging slots" in hdr and "lengths that live on the device" in hdr
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    assert re.search(r"function filt_rates_lens_device!\(f::RatesFIRFilter, yptr::Ptr\{Cvoid\}, ycap::Integer, ystride::Integer, xptr::Ptr\{Cvoid\}, "
                     r"xlens::Ptr\{Int64\},\s+xlenmax::Integer, xstride::Integer", jl)
    assert re.search(r"ccall\(\(:mrhip_filt_device_rates_lens_device, libmr\), Cint,\s*"
                     r"\(Ptr\{Cvoid\}, Ptr\{Cvoid\}, Ptr\{Int64\}, Int64, Int64, Ptr\{Cvoid\}, Int64, Int64, Ptr\{Int64\}, Ptr\{Cvoid\}\)", jl)
    assert re.search(r"function filt_rates_chained!\(f::RatesFIRFilter, prev::Union\{RatesFIRFilter,FIRFilter\}, yptr::Ptr\{Cvoid\}", jl)
    assert re.search(r"ccall\(\(:mrhip_filt_device_rates_chained, libmr\), Cint,\s*"
                     r"\(Ptr\{Cvoid\}, Ptr\{Cvoid\}, Ptr\{Cvoid\}, Int64, Int64, Ptr\{Cvoid\}, Int64, Int64, Ptr\{Int64\}, Ptr\{Cvoid\}\)", jl)
    assert re.search(r"^export .*filt_rates_lens_device!, filt_rates_chained!", jl, flags=re.M)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rates_device_lengths_check") / "rates_device_lengths_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "rates_device_lengths_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def _run(exe, mode, rows):
    text = "".join(" ".join(map(str, r)) + "\n" for r in rows)
    p = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout.splitlines()


BIG = 2 ** 31 - 1
# (who, lens_is_null, len_max, x_is_null, nch, x_stride) -> (status, the message behind the function's name)
LENGTH_CASES = [
    ((0, 0, 1500, 0, 4, 1500), (0, "")),                                     # the stride may equal the declared maximum
    ((0, 0, 0, 0, 4, 0), (0, "")),                                           # an all-empty call
    ((0, 0, 0, 1, 4, 0), (0, "")),                                           # ... needs no x
    ((0, 0, 1500, 0, 1, 0), (0, "")),                                        # one channel: the stride is not looked at
    ((0, 0, BIG - 1, 0, 3, BIG), (0, "")),                                   # the largest maximum a call takes
    ((1, 0, 1500, 0, 4, 1500), (0, "")),
    ((0, 1, 1500, 0, 4, 1500), (1, ": x_lens is NULL")),
    ((0, 1, -1, 1, 4, 0), (1, ": x_lens is NULL")),                          # ... comes first
    ((0, 0, -1, 0, 4, 1500), (1, ": negative x_len_max (the declared maximum of the lengths must be >= 0)")),
    ((1, 0, -1, 0, 4, 1500), (1, ": negative x_len_bound (the declared maximum of the lengths must be >= 0)")),
    ((0, 0, -2 ** 62, 1, 4, 0), (1, ": negative x_len_max")),
    ((0, 0, BIG, 0, 4, 2 ** 40), (5, ": a call takes fewer than 2^31-1 samples per channel")),
    ((1, 0, 2 ** 40, 1, 4, 0), (5, ": a call takes fewer than 2^31-1 samples per channel")),      # the size before x and the stride
    ((0, 0, 1, 1, 4, 1500), (1, ": x is NULL")),
    ((1, 0, 1, 1, 4, 0), (1, ": x is NULL")),                                # x before the stride
    ((0, 0, 257, 0, 4, 256), (1, ": x_stride < x_len_max")),
    ((1, 0, 257, 0, 4, 256), (1, ": x_stride < x_len_bound")),
    ((0, 0, 0, 0, 4, -1), (1, ": x_stride < x_len_max")),
]


def test_the_pure_checks_of_the_lengths(check):
    lines = _run(check, "lengths", [c for c, _ in LENGTH_CASES])
    assert len(lines) == len(LENGTH_CASES)
    for (case, (status, text)), line in zip(LENGTH_CASES, lines):
        got, message = line.split(" | ", 1) if " | " in line else (line.rstrip(" |"), "")
        assert int(got) == status, (case, line)
        who = CHAINED if case[0] else LENS
        if status:
            assert message.startswith(who + text), (case, line)              # every refusal names its entry point
        else:
            assert message == "", (case, line)
    assert {s for _, (s, _) in LENGTH_CASES} == {0, 1, 5}


F32, F64, C64, C128 = range(4)
# (f_is_rates, same, prev_is_rates, f_nch, prev_nch, f_dev, prev_dev, f_tx, prev_ty, prev_called, prev_dev_planned) -> (status, message)
CHAIN_CASES = [
    ((1, 0, 1, 4, 4, 0, 0, F32, F32, 1, 0), (0, "")),                        # rates behind rates
    ((1, 0, 0, 4, 4, 0, 0, C64, C64, 0, 1), (0, "")),                        # rates behind a one-state filter's device-planned call
    ((1, 0, 1, 1, 1, 3, 3, F64, F64, 1, 1), (0, "")),
    ((0, 0, 1, 4, 4, 0, 0, F32, F32, 1, 1), (1, " takes a filter of mrhip_create_arbitrary_rates or mrhip_create_farrow_rates")),
    ((0, 1, 1, 4, 5, 0, 1, F32, F64, 0, 0), (1, " takes a filter of")),      # ... comes first
    ((1, 1, 1, 4, 4, 0, 0, F32, F32, 1, 0), (1, ": prev is the filter itself")),
    ((1, 0, 1, 4, 5, 0, 0, F32, F32, 1, 0), (1, ": the two filters have different numbers of channels")),
    ((1, 0, 0, 4, 1, 0, 0, F32, F32, 0, 1), (1, ": the two filters have different numbers of channels")),
    ((1, 0, 1, 4, 4, 0, 1, F32, F32, 1, 0), (1, ": the two filters live on different devices")),
    ((1, 0, 1, 4, 5, 0, 1, F32, F64, 0, 0), (1, ": the two filters have different numbers of channels")),      # channels before devices
    ((1, 0, 1, 4, 4, 0, 0, F32, C64, 1, 0), (1, ": the filter's sample dtype is not the previous filter's output dtype")),
    ((1, 0, 1, 4, 4, 0, 0, F32, F64, 1, 0), (1, ": the filter's sample dtype is not the previous filter's output dtype")),
    ((1, 0, 0, 4, 4, 0, 0, C128, C64, 0, 1), (1, ": the filter's sample dtype is not")),
    ((1, 0, 1, 4, 4, 0, 0, F32, F32, 0, 0), (1, ": the previous filter has not been called since its creation or mrhip_reset")),
    ((1, 0, 1, 4, 4, 0, 0, F32, F32, 0, 1), (1, ": the previous filter has not been called since")),          # (a flag of one-state filters)
    ((1, 0, 0, 4, 4, 0, 0, F32, F32, 0, 0), (1, ": the previous filter's latest call was not planned on the device")),
    ((1, 0, 0, 4, 4, 0, 0, F32, F32, 1, 0), (1, ": the previous filter's latest call was not planned on the device")),
]


def test_the_pure_checks_of_a_chain(check):
    lines = _run(check, "chain", [c for c, _ in CHAIN_CASES])
    assert len(lines) == len(CHAIN_CASES)
    for (case, (status, text)), line in zip(CHAIN_CASES, lines):
        got, message = line.split(" | ", 1) if " | " in line else (line.rstrip(" |"), "")
        assert int(got) == status, (case, line)
        assert message.startswith(CHAINED + text) if status else message == "", (case, line)


def test_the_acceptance_rule_and_the_import(check):
    """0 and x_len_max are accepted; -1, x_len_max + 1, 2^40 and INT64_MIN are refused -- at two maxima, one of them 0; then the import's
    statement over those values from each of its three sources: the accepted length or 0 in the array, the mark in the record, nothing
    else of the record moved"""
    M = 1500
    rows = [(0, M), (M, M), (-1, M), (M + 1, M), (2 ** 40, M), (-2 ** 63, M), (1, M), (M - 1, M),
            (0, 0), (1, 0), (-1, 0), (2 ** 63 - 1, BIG - 1), (BIG - 1, BIG - 1), (BIG, BIG - 1)]
    want = [1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 0]
    lines = _run(check, "accept", rows)
    assert lines[-1] == "import ok" and [int(v) for v in lines[:-1]] == want
    hdr = open(os.path.join(CSRC, "rates_arb.h")).read()
    # ONE text of the rule, compiled for both sides
    assert hdr.count("MRHIP_RATES_HD inline bool rates_length_accepted(long long l, long long len_max) { return l >= 0 && l <= len_max; }") == 1
    assert re.search(r"long long error;[^\n]*\n\s*long long len_refused;", hdr) and "static_assert(sizeof(RateChannel) == 64" in hdr


def test_what_the_python_method_refuses_without_a_gpu(pkg):
    import torch
    h = np.ones(8, dtype=np.float32)
    rates = [0.47, 1.0, 2.123]
    x, y = torch.zeros((3, 16)), torch.zeros((3, 40))
    lens = torch.tensor([16, 0, 5], dtype=torch.int64)
    for f in (pkg.FIRFilter.per_channel_rates(h, rates, 4), pkg.FIRFilter.per_channel_rates_farrow(h, rates, 4, 2)):
        other = pkg.FIRFilter.per_channel_rates(h, rates, 4)
        calls = {
            "neither source": lambda: f.filt_rates_async(y, x),
            "max_length alone": lambda: f.filt_rates_async(y, x, max_length=16),
            "both sources": lambda: f.filt_rates_async(y, x, lengths=lens, max_length=16, after=other),
            "a CPU tensor": lambda: f.filt_rates_async(y, x, lengths=lens, max_length=16),
            "a numpy array": lambda: f.filt_rates_async(y, x, lengths=lens.numpy(), max_length=16),
            "a list": lambda: f.filt_rates_async(y, x, lengths=[16, 0, 5], max_length=16),
            "an unbound prev": lambda: f.filt_rates_async(y, x, after=other),
            "not a filter": lambda: f.filt_rates_async(y, x, after=x),
        }
        for what, call in calls.items():
            with pytest.raises(pkg.MultirateHIPError) as e:
                call()
            assert e.value.code == 1 and "filt_rates_async" in str(e.value), what
            assert f._handle is None, what                                   # nothing was bound on the way
    # (a wrong dtype or shape on a host tensor: refused all the same -- in their own words in the test below)
    f = pkg.FIRFilter.per_channel_rates(h, rates, 4)
    for bad in (lens.to(torch.int32), lens[:2], lens.reshape(3, 1), lens.to(torch.float64)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.filt_rates_async(y, x, lengths=bad, max_length=16)
        assert e.value.code == 1
    # a filter without per-channel rates, whatever else is given
    for g in (pkg.FIRFilter(h, 1.5, 4), pkg.FIRFilter(h, Fraction(2, 3)), pkg.FIRFilter.per_channel_arbitrary(np.ones((3, 8), dtype=np.float32), 1.5, 4)):
        for kw in ({"lengths": lens, "max_length": 16}, {"after": f}, {}):
            with pytest.raises(pkg.MultirateHIPError) as e:
                g.filt_rates_async(y, x, **kw)
            assert e.value.code == 1 and "per_channel_rates" in str(e.value)
    # the older methods keep their signatures
    import inspect
    assert list(inspect.signature(pkg.FIRFilter.filt_into).parameters) == ["self", "buffer", "x", "lengths"]
    assert list(inspect.signature(pkg.FIRFilter.filt_into_async).parameters) == ["self", "buffer", "x", "count", "after"]
    sig = inspect.signature(pkg.FIRFilter.filt_rates_async)
    assert [n for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY] == ["lengths", "max_length", "after", "counts"]


def test_the_dtype_and_shape_checks_of_lengths_come_before_any_device_work(pkg, monkeypatch):
    """a wrong dtype or shape is refused in its own words: the checks run on a tensor that says it lives on the GPU (a stand-in object
    with the attributes the method reads), on a machine without one"""
    import torch
    f = pkg.FIRFilter.per_channel_rates(np.ones(8, dtype=np.float32), [0.47, 1.0, 2.123], 4)
    x, y = torch.zeros((3, 16)), torch.zeros((3, 40))

    class OnDevice:                                                          # what filt_rates_async reads of `lengths` ahead of x and buffer
        is_cuda = True

        def __init__(self, t):
            self.dtype, self.shape, self._t = t.dtype, t.shape, t

        def is_contiguous(self):
            return self._t.is_contiguous()

    monkeypatch.setattr(pkg.host, "_is_torch", lambda v: isinstance(v, (torch.Tensor, OnDevice)))
    good = torch.tensor([16, 0, 5], dtype=torch.int64)
    cases = [(good.to(torch.int32), 16, "must be int64"), (good.to(torch.float64), 16, "must be int64"), (good[:2], 16, "one per channel"),
             (good.reshape(3, 1), 16, "one per channel"), (torch.zeros(6, dtype=torch.int64)[::2], 16, "contiguous"),
             (good, None, "max_length"), (good, -1, "max_length"), (good, 2.5, "max_length")]
    for t, m, word in cases:
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.filt_rates_async(y, x, lengths=OnDevice(t), max_length=m)
        assert e.value.code == 1 and word in str(e.value), (word, str(e.value))
    with pytest.raises(pkg.MultirateHIPError) as e:                          # lengths in order; then x and buffer: host tensors
        f.filt_rates_async(y, x, lengths=OnDevice(good), max_length=16)
    assert e.value.code == 1 and "torch device tensors" in str(e.value) and f._handle is None


def test_the_import_kernel_is_plain_guarded_hip():
    src = open(os.path.join(CSRC, "kernels_rates_arb.hip")).read()
    m = re.search(r"__global__ __launch_bounds__\(kRatesSchedThreads\) void rates_lens_set_kernel\(RatesLensArgs a\)\n\{.*?\n\}\n", src, flags=re.S)
    assert m, "the import kernel, 64 lanes a workgroup like the schedule kernel"
    body = m.group(0)
    assert "if (c >= a.nch) return;" in body and body.index("if (c >= a.nch) return;") < body.index("a.src[c]")      # the guard, ahead of every access
    assert "rates_length_accepted(l, a.len_max)" in body                     # the rule: the header's one text
    for word in ("asm", "atomic", "__syncthreads", "while", "for (", "__shared__", "__builtin"):
        assert word not in body, word
    assert "asm" not in src and "atomic" not in src.lower()                  # the unit as a whole, as before
    # beside rates_set_kernel, and its own launch: 64 lanes a workgroup, ceil(nch / 64) workgroups
    assert src.index("void rates_set_kernel(") < src.index("void rates_lens_set_kernel(") < src.index("void arb_rates_generic_kernel(")
    assert re.search(r"hipError_t launch_rates_lens_set\(const RatesLensArgs &l, hipStream_t st\)\n\{\n\s*const dim3 grid\(static_cast<unsigned>\("
                     r"\(l\.nch \+ kRatesSchedThreads - 1\) / kRatesSchedThreads\)\);\n\s*hipLaunchKernelGGL\(rates_lens_set_kernel, grid, "
                     r"dim3\(kRatesSchedThreads\), 0, st, l\);", src)
    # the walk, the set kernel and the filter kernels keep their text
    assert "const long long len = RAGGED ? rates_channel_len(s.x_lens, s.x_len, c) : s.x_len;" in src
    assert "if (r >= lo && r <= hi) { rec[c].rate = r; rec[c].delta = N / r; }      // Filters.jl:113" in src
    api = open(os.path.join(CSRC, "api.hip")).read()
    one = re.search(r"static int rates_device_lengths_call\(.*?\n\}\n", api, flags=re.S).group(0)
    assert "rag_pin" not in one and "ragged_upload" not in one and "hipEventSynchronize" not in one and "hipStreamSynchronize" not in one
    assert "static int ragged_lengths_array(mrhip_filter *f)" in api         # the device array without the pinned slots
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^.*kernels_rates_arb\.hip\.o:.*\brates_arb\.h\b", mk, flags=re.M)


def test_the_unit_of_the_import_kernel_uses_no_scratch_and_no_accvgprs(pkg):
    unit = "kernels_rates_arb.hip"
    obj = os.path.join(CSRC, "build", unit + ".o")
    assert os.path.exists(obj), "the build leaves its objects in csrc/build"
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "no llvm tools"
    sizes = _kernel_scratch(obj)
    for kernel in ("arb_rates_generic_kernel", "arb_rates_tiled_kernel"):
        _assert_rates_filter_kernel(sizes, kernel, each=12)
    for kernel, count in (("rates_lens_set_kernel", 1), ("rates_set_kernel", 1), ("rates_reset_kernel", 1), ("rates_schedule_kernel", 2),
                          ("rates_ragged_schedule_kernel", 2)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"
