"""The launchers' grid arithmetic (csrc/host_logic.cpp: pair_grid, opair_six_wave_cap, persistent_grid_size) against
tests/golden/launch_grid_cases.json: results recorded from the three copies of the pair-grid block (rational_opair, fir_stream,
fir_stream_rt) and the persistent-grid blocks those functions replaced, over occupancy 0..8, 8 and 256 CUs, step counts round 1,
round the grid and round three tiles a workgroup, J 1..16, 0 / 1 / 3 / 64 independent streams, six- and four-wave workgroups, the
ring consumer with grid_cap 0 / 1 / 100 and the per-CU knobs.  No GPU: tests/launch_grid_check.cpp is built by the host compiler
with -fsanitize=address,undefined as a program of its own and fed the rows."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_functions_reproduce_the_recorded_launches(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "multirate.jl_amd", "csrc")
    exe = str(tmp_path / "launch_grid_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tests", "launch_grid_check.cpp"), os.path.join(csrc, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "launch_grid_cases.json")) as f:
        table = json.load(f)
    assert len(table["pair_columns"]) == 15 and len(table["persistent_columns"]) == 7
    pair, pers = table["pair"], table["persistent"]
    assert len(pair) >= 300 and len(pers) >= 100
    # the table crosses every branch: each kernel, ring with each cap, every stream count, both grab modes, the six-wave cap
    assert {r[0] for r in pair} == {0, 1, 2} and {(r[7], r[8]) for r in pair} == {(0, 0), (1, 0), (1, 1), (1, 100)}
    assert {r[5] for r in pair} == {0, 1, 3, 64} and {r[14] for r in pair} == {0, 1} and {r[6] for r in pair if r[0] == 0} == {256, 384}
    assert any(r[0] == 0 and r[9] == 0 and r[1] > 3 and r[10] == 3 for r in pair)
    assert {r[0] for r in pers} == {0, 1, 2}
    text = "".join("P " + " ".join(str(v) for v in r) + "\n" for r in pair) + "".join("G " + " ".join(str(v) for v in r) + "\n" for r in pers)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().endswith(f"rows {len(pair) + len(pers)} differing 0"), p.stdout[-500:]
