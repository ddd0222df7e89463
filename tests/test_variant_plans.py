"""The plans of the LDS-tiled variant kernels (csrc/host_logic.cpp: plan_variant_poly_tiled, plan_variant_arb_tiled and the seven
families' eligibility functions with the switch value passed in) against tests/golden/variant_plan_cases.json: results recorded from
the seven plan_*_tiled functions those replaced (fn 0 plan_ctaps_tiled, 1 plan_bank_tiled, 2 plan_bank_ctaps_tiled, 3 plan_ctaps_arb_tiled,
4 plan_arb_bank_tiled, 5 plan_farrow_bank_tiled, 6 plan_ctaps_farrow_tiled), each with its switch unset (-1), 0 and 1, on 8 and 256 CUs,
over every type combination.  No GPU: tests/variant_plan_check.cpp is built by the host compiler with -fsanitize=address,undefined as
a program of its own and fed the rows."""
import json
import math
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN, XF64, RF64, CX, L, M, T, P, NOUT, NCH, RATE, CUS, MODE, MINSET, MINVAL, OK, CPL, PITCH, BANK, XOFF, SPAN = range(21)
TILE_OUT, TPC, TILES, LDS = 26, 27, 28, 31
KB = 1024


def _sb(r):
    return (8 if r[XF64] else 4) * (2 if r[CX] else 1)


def _tb(r):
    return (8 if r[RF64] else 4) * (2 if r[FN] in (0, 2, 3, 6) else 1)


def _twin(rows, r, mode):
    """the row with r's inputs and another switch value"""
    key = r[:MODE] + [mode] + r[MODE + 1:OK]
    return next((q for q in rows if q[:OK] == key), None)


def _check_rational_coverage(rows, fn):
    mine = [r for r in rows if r[FN] == fn]
    live = [r for r in mine if r[MODE] != 0 and r[NOUT] >= 1 and r[T] >= 1]          # past the first return
    assert any(r[MODE] == 0 for r in mine) and any(r[NOUT] < 1 for r in mine) and any(r[T] < 1 for r in mine)
    assert all(not r[OK] for r in mine if r not in live)
    bank = lambda r: (r[L] * (r[T] + 1) * _tb(r) + 15) // 16 * 16
    assert any(bank(r) > 96 * KB and not r[OK] for r in live)                         # a bank over 96 KB
    assert any(bank(r) <= 96 * KB and r[MODE] == 1 and not r[OK] for r in live)      # forced and refused: the 150 KB rejection
    assert {r[TILE_OUT] for r in live if r[OK]} == {256, 128, 64}                     # tile_out as planned, halved once and twice
    assert {r[CPL] for r in live if r[OK]} == ({4, 2, 1} if fn == 0 else {1})
    assert any(r[OK] and r[CPL] == 1 and r[NCH] >= 32 for r in live) or fn != 0       # channels per lane searched down from 4
    assert {(r[MODE], r[CUS]) for r in live if r[OK]} == {(-1, 8), (-1, 256), (1, 8), (1, 256)}
    # fewer tiles than CUs under the default rule: refused, and taken when forced
    few = [r for r in live if r[MODE] == -1 and not r[OK] and (_twin(rows, r, 1) or [0] * 32)[OK]]
    assert few and all(_twin(rows, r, 1)[TILES] < r[CUS] for r in few)
    assert any(r[MODE] == -1 and r[OK] and r[TILES] == r[CUS] for r in live)         # exactly a tile per CU: taken


def _check_arb_coverage(rows, fn):
    mine = [r for r in rows if r[FN] == fn]
    guard = lambda r: ((r[MODE] == 0 if fn != 5 else r[MODE] != 1) or r[NOUT] < 1 or r[T] < 1 or not r[RATE] > 0.0
                       or (fn == 4 and r[L] < 1) or (fn in (5, 6) and r[P] < 0))
    live = [r for r in mine if not guard(r)]
    assert {r[MODE] for r in mine} == {-1, 0, 1} and all(not r[OK] for r in mine if guard(r))
    assert any(r[NOUT] < 1 for r in mine) and any(r[T] < 1 for r in mine) and any(not r[RATE] > 0.0 for r in mine)
    assert fn != 4 or any(r[L] < 1 and r[MODE] == 1 and r[NOUT] >= 1 and r[T] >= 1 and r[RATE] > 0 for r in mine)
    assert fn not in (5, 6) or any(r[P] < 0 and r[MODE] == 1 and r[NOUT] >= 1 and r[T] >= 1 and r[RATE] > 0 for r in mine)
    fixed = {3: lambda r: (2 * r[L] * (r[T] + 1) * _tb(r) + 15) // 16 * 16, 4: lambda r: (2 * r[L] * (r[T] + 1) * _tb(r) + 15) // 16 * 16,
             5: lambda r: 0, 6: lambda r: r[T] * (r[P] + 1) * 16 + r[T] * 256 * _tb(r)}[fn]
    over = {3: lambda r: fixed(r) > 96 * KB, 4: lambda r: fixed(r) + (r[T] + 1) * _sb(r) > 78 * KB, 5: lambda r: False,
            6: lambda r: fixed(r) >= 159 * KB}[fn]
    if fn != 5:
        assert any(over(r) and not r[OK] for r in live) and all(not r[OK] for r in live if over(r))    # the byte budget
    fits = [r for r in live if not over(r)]
    assert any(r[MODE] == 1 and not r[OK] for r in fits)                              # forced and refused: not even one window
    per_tile = lambda r: math.ceil(255 / r[RATE]) + r[T] + 2.0
    assert any(r[OK] and r[SPAN] == int(per_tile(r)) for r in fits)                   # the span the rate asks for
    cut = [r for r in fits if r[MODE] == 1 and r[OK] and r[SPAN] < per_tile(r)]       # the cut span: only when forced
    assert cut and all(r[XOFF] == fixed(r) and r[LDS] == fixed(r) + r[SPAN] * _sb(r) * r[CPL] for r in fits if r[OK])
    if fn != 5:
        assert any((_twin(rows, r, -1) or [1] * 32)[OK] == 0 for r in cut)
    assert {r[CPL] for r in fits if r[OK]} == ({1, 2} if fn in (3, 6) else {1})
    assert {r[CUS] for r in fits if r[OK]} == {8, 256}
    tiles = lambda r: -(-r[NOUT] // 256) * (1 if fn == 6 else -(-r[NCH] // r[CPL]))
    assert all(r[TILES] == tiles(r) and r[TILE_OUT] == 256 for r in fits if r[OK])
    default = [r for r in fits if r[MODE] == -1]
    if fn == 3:       # never by default; with a threshold: outputs x channels, both sides, and a tile per CU
        assert all(not r[OK] for r in default if not r[MINSET] or r[MINVAL] < 0)
        assert any(r[OK] and r[NOUT] * r[NCH] == r[MINVAL] for r in default) and any(not r[OK] and r[NOUT] * r[NCH] == r[MINVAL] - 8 for r in default)
        assert any(r[OK] and r[TILES] == r[CUS] for r in default)
        assert any(not r[OK] and r[MINVAL] == 0 and r[MINSET] and -(-r[NOUT] // 256) * r[NCH] == r[CUS] - 1 for r in default)
    if fn == 4:       # 20 tiles a CU, both sides, on both chips
        for cus in (8, 256):
            assert any(r[OK] and r[CUS] == cus and r[TILES] == 20 * cus for r in default)
            assert any(not r[OK] and r[CUS] == cus and _twin(rows, r, 1)[TILES] == 20 * cus - 8 for r in default if _twin(rows, r, 1))
    if fn == 5:       # never by default
        assert default == [] and any(r[MODE] == -1 and r[NOUT] >= 1 for r in mine)
    if fn == 6:       # Float32 arithmetic, 32 taps per phase, 21 000 outputs a channel: each condition from both sides; another threshold
        plain = [r for r in default if not r[MINSET]]
        assert any(r[OK] and r[NOUT] == 21000 for r in plain) and any(not r[OK] and r[NOUT] == 20999 and not r[RF64] and r[T] == 32 for r in plain)
        assert all(not r[RF64] and r[T] == 32 and r[NOUT] >= 21000 for r in plain if r[OK])
        assert any(r[RF64] and r[T] == 32 and r[NOUT] >= 21000 for r in plain) and any(not r[RF64] and r[T] == 24 and r[NOUT] >= 21000 for r in plain)
        moved = [r for r in default if r[MINSET]]
        assert any(r[OK] and r[NOUT] == r[MINVAL] for r in moved) and any(not r[OK] and r[NOUT] == r[MINVAL] - 1 for r in moved)
        assert any(r[MINVAL] < 0 for r in moved) and all(not r[OK] for r in moved if r[MINVAL] < 0)


def test_plan_functions_reproduce_the_recorded_plans(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "multirate.jl_amd", "csrc")
    exe = str(tmp_path / "variant_plan_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tests", "variant_plan_check.cpp"), os.path.join(csrc, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "variant_plan_cases.json")) as f:
        table = json.load(f)
    rows = table["rows"]
    assert len(table["columns"]) == 32 and all(len(r) == 32 for r in rows) and len(rows) >= 300
    assert all(r[OK] or not any(r[OK + 1:]) for r in rows)                            # a refused plan is recorded as zeros
    assert all(not any(r[SPAN + 1:TILE_OUT]) and not r[29] and not r[30] for r in rows)   # the fields the pipe kernels alone use stay zero
    # the table reaches every return of the seven recorded functions
    for fn in (0, 1, 2):
        _check_rational_coverage(rows, fn)
    for fn in (3, 4, 5, 6):
        _check_arb_coverage(rows, fn)
    text = "".join(" ".join(repr(v) if i == RATE else str(v) for i, v in enumerate(r)) + "\n" for r in rows)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().endswith(f"rows {len(rows)} differing 0"), p.stdout[-500:]
