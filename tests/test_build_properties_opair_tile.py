"""What the headline output-pair kernel does AROUND its arithmetic, read from the object the build made (CPU only).

rational_opair_kernel<24, false, 1, 1, float, float, 1> (147//160, 24 taps per phase, Float32, the PLAIN mode of big launches) spends 100
vector instructions per step on its slots (tests/test_build_properties_opair.py: 51 multiplies, 49 adds).  This file bounds the rest:

  * the compute waves' tile loop holds no flat instruction and no wait on vmcnt -- the tile descriptors come by LDS reads (csrc/pair_device.h:
    desc_get2), so a wave never waits for its own output stores at a tile hand-over;
  * at most 12 vector-ALU instructions per tile outside the two step loops (the lane's constants live in registers: no division per tile);
  * at most 101 per step: the slots and ONE address update (the window; the store's base advances in SGPRs, the lanes that store are an
    SGPR mask);
  * the loader's interior loop issues an LDS-DMA operation with at most 2 vector-ALU instructions;
  * at most 80 VGPRs, no scratch.

The counts of this build go to profiles/r14/tile_overhead_isa.txt beside the parent's (recorded there when this file was written)."""
import os
import re
import subprocess
import tempfile

import pytest

from test_build_properties_opair import CSRC, HEADLINE, LLVM, ROOT, UNIT, _code_object, _metadata

REPORT = os.path.join(ROOT, "profiles", "r14", "tile_overhead_isa.txt")
# the parent commit's counts, by the same functions (its object is not kept: the figures are).  Its loader had no interior loop without a
# multiply: 10.0 is the cheapest of its LDS-DMA loops (20 vector-ALU instructions around two operations).
PARENT = {"tile_flat": 2, "tile_vmcnt_waits": 2, "tile_valu_outside_steps": 40, "step_valu": [103, 109], "loader_valu_per_dma": 10.0, "vgpr_count": 77, "scratch": 0}


def _is_valu(mn):
    return mn.startswith("v_")


def _instructions(co, symbol):
    """[(address, mnemonic, operands, branch target or None)] of `symbol`"""
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + symbol, co], capture_output=True, text=True,
                         timeout=300, check=True).stdout
    start = int(re.search(r"^([0-9a-f]+) <" + re.escape(symbol) + ">:", dis, re.M).group(1), 16)
    insts = []
    for ln in dis.splitlines():
        m = re.match(r"\s+(\S+)(.*?)//\s*([0-9A-Fa-f]+):", ln)
        if not m:
            continue
        t = re.search(r"<" + re.escape(symbol) + r"\+0x([0-9a-f]+)>\s*$", ln) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
        insts.append((int(m.group(3), 16), m.group(1), m.group(2).strip(), start + int(t.group(1), 16) if t else None))
    return insts


def _loops(insts):
    """(lo, hi) address ranges: a loop is what lies between a backward branch and its target; ranges with one head are one loop"""
    heads = {}
    for a, _, _, t in insts:
        if t is not None and t <= a:
            heads[t] = max(heads.get(t, a), a)
    return sorted(heads.items())


def _body(insts, lo, hi):
    return [(a, mn, ops) for a, mn, ops, _ in insts if lo <= a <= hi]


def _innermost(loops):
    return [(lo, hi) for lo, hi in loops if not any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi for l2, h2 in loops)]


def measure(co, symbol):
    """the counts this file bounds, of one code object"""
    insts = _instructions(co, symbol)
    loops = _loops(insts)
    inner = _innermost(loops)
    n = lambda body, pred: sum(1 for _, mn, ops in body if pred(mn, ops))
    steps = [(lo, hi) for lo, hi in inner if n(_body(insts, lo, hi), lambda mn, ops: mn == "ds_read_b64") >= 10]
    assert len(steps) == 2, [(hex(lo), hex(hi)) for lo, hi in inner]
    # the compute waves' tile loop: the smallest loop that holds both step loops
    around = [(lo, hi) for lo, hi in loops if all(lo <= a and b <= hi for a, b in steps) and (lo, hi) not in steps]
    assert around, "no loop around the step loops"
    tlo, thi = min(around, key=lambda r: r[1] - r[0])
    tile = _body(insts, tlo, thi)
    in_steps = lambda a: any(lo <= a <= hi for lo, hi in steps)
    out = {
        "tile_flat": n(tile, lambda mn, ops: mn.startswith("flat_")),
        "tile_vmcnt_waits": n(tile, lambda mn, ops: mn == "s_waitcnt" and "vmcnt" in ops),
        "tile_valu_outside_steps": sum(1 for a, mn, _ in tile if _is_valu(mn) and not in_steps(a)),
        "step_valu": sorted(n(_body(insts, lo, hi), lambda mn, ops: _is_valu(mn)) for lo, hi in steps),
    }
    # the loader's interior loop: the innermost loops with an LDS-DMA operation and no multiply
    dma = []
    for lo, hi in inner:
        body = _body(insts, lo, hi)
        ops = n(body, lambda mn, o: mn == "global_load_lds_dwordx4")
        if ops and not n(body, lambda mn, o: "_mul_" in mn or "_mad_" in mn):
            dma.append(n(body, lambda mn, o: _is_valu(mn)) / ops)
    assert dma, "no LDS-DMA loop without a multiply"
    out["loader_valu_per_dma"] = max(dma)
    return out


def _built():
    obj = os.path.join(CSRC, "build", UNIT + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    if os.path.getmtime(obj) < max(os.path.getmtime(os.path.join(CSRC, f)) for f in (UNIT, "opair_kernel.inc", "pair_device.h", "pair_loader.h")):
        pytest.skip("object older than its source")
    return obj


def test_headline_tile_loop_overhead(pkg):
    obj = _built()
    with tempfile.TemporaryDirectory() as tmp:
        co = _code_object(obj, tmp)
        symbol, md = _metadata(co, HEADLINE)
        got = measure(co, symbol)
    got["vgpr_count"], got["scratch"] = md["vgpr_count"], md["private_segment_fixed_size"]
    text = "rational_opair_kernel<24, false, 1, 1, float, float, 1>, gfx950: instructions around the arithmetic (tests/test_build_properties_opair_tile.py)\n"
    text += f"{'count':<28}{'parent':>12}{'this build':>12}\n"
    text += "".join(f"{k:<28}{str(PARENT[k]):>12}{str(got[k]):>12}\n" for k in PARENT)
    print(text)
    try:                                                     # (the record; a read-only tree keeps the one it has)
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        if not os.path.exists(REPORT) or open(REPORT).read() != text:
            with open(REPORT, "w") as fh:
                fh.write(text)
    except OSError:
        pass
    assert got["tile_flat"] == 0, got
    assert got["tile_vmcnt_waits"] == 0, got
    assert got["tile_valu_outside_steps"] <= 12, got
    assert max(got["step_valu"]) <= 101, got
    assert got["loader_valu_per_dma"] <= 2, got
    assert md["vgpr_count"] <= 80 and md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
