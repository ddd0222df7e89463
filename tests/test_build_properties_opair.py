"""Properties of the built output-pair kernel that its speed rests on (CPU only: reads the object the build made).

The headline instantiation rational_opair_kernel<24, false, 1, 1, float, float, 1> (147//160, 24 taps per phase, Float32, the PLAIN
mode of big launches) is bound by the vector ALU.  Its end slots run under a lane mask in EXEC (csrc/pair_device.h: masked_mac and its
kin) instead of selecting -0.0 for the lanes that skip them: the step loop holds the multiplies and adds of the taps and no select.
Six waves per SIMD need at most 80 VGPRs, and the hand-issued LDS reads with counted waits allow no scratch memory."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multirate.jl_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
UNIT = "kernels_rational_opair_f32_s1r.hip"
HEADLINE = "rational_opair_kernelILi24ELb0ELi1ELi1EffLi1EE"       # <T = 24, STRICT, NC = 1, SMIN = 1, float, float, MODE = 1>


def _code_object(obj, tmp):
    """the gfx950 code object bundled in a host object file (compressed: --offload-compress; clang-offload-bundler unpacks both kinds)"""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "co.o")
    got = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o")],
                         capture_output=True, text=True, timeout=300)
    assert got.returncode == 0 and os.path.exists(fat), "no device code bundled in " + obj
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True, text=True, timeout=300, check=True)
    assert os.path.getsize(co) > 0, "no device code object bundled in " + obj
    return co


def _metadata(co, kernel):
    """(mangled name, {field: value}) of the one kernel whose name contains `kernel`, from the code object's notes"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, timeout=300, check=True).stdout
    found = []
    for entry in notes.split("\n  - .agpr_count")[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry)
        if name and kernel in name.group(1):
            fields = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)\s*(?=\n)", entry)}
            fields["agpr_count"] = int(re.match(r":\s+(\d+)", entry).group(1))
            found.append((name.group(1), fields))
    assert len(found) == 1, [n for n, _ in found]
    return found[0]


def _innermost_loops(co, symbol):
    """the instruction lists of the loops of `symbol` that contain no other loop: a loop is what lies between a backward branch and its target"""
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + symbol, co], capture_output=True, text=True,
                         timeout=300, check=True).stdout
    start = int(re.search(r"^([0-9a-f]+) <" + re.escape(symbol) + ">:", dis, re.M).group(1), 16)
    insts = []                                               # (address, mnemonic, branch target or None)
    for ln in dis.splitlines():
        m = re.match(r"\s+(\S+).*//\s*([0-9A-Fa-f]+):", ln)
        if not m:
            continue
        t = re.search(r"<" + re.escape(symbol) + r"\+0x([0-9a-f]+)>\s*$", ln) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
        insts.append((int(m.group(2), 16), m.group(1), start + int(t.group(1), 16) if t else None))
    loops = [(t, a) for a, _, t in insts if t is not None and t <= a]
    inner = [(lo, hi) for lo, hi in loops if not any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi for l2, h2 in loops)]
    return [[mn for a, mn, _ in insts if lo <= a <= hi] for lo, hi in inner]


def test_headline_step_loop_has_no_selects_and_six_waves(pkg):
    obj = os.path.join(CSRC, "build", UNIT + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in (UNIT, "opair_kernel.inc", "pair_device.h")):
        pytest.skip("object older than its source")
    with tempfile.TemporaryDirectory() as tmp:
        co = _code_object(obj, tmp)
        symbol, md = _metadata(co, HEADLINE)
        loops = _innermost_loops(co, symbol)
    assert md["private_segment_fixed_size"] == 0 and md["agpr_count"] == 0, md          # no scratch, nothing parked in AccVGPRs
    assert md["vgpr_spill_count"] == 0 and md["vgpr_count"] <= 80, md                  # six waves per SIMD
    # the step loops (a tile whose steps are all inside the channel, and the last tile's): 14 window reads per step, two outputs per lane
    steps = [lp for lp in loops if sum(mn == "ds_read_b64" for mn in lp) >= 10]
    assert len(steps) == 2, [len(lp) for lp in loops]
    for lp in steps:
        count = lambda prefix: sum(mn.startswith(prefix) for mn in lp)
        assert count("ds_read_b64") == 14, lp
        assert count("v_cndmask") == 0, [mn for mn in lp if mn.startswith("v_cndmask")]
        # 24 taps of A and of B, and the three end slots of either that some lanes use: 51 products, two of them start a sum
        assert (count("v_mul_f32"), count("v_add_f32"), count("v_fma"), count("v_mac")) == (51, 49, 0, 0), lp
