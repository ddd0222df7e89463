"""CPU-only checks of the constructors' one path (csrc/create.hip, csrc/create.h, the pure part in csrc/host_logic.cpp):

* the checks in front of the device query (create_check_args) and behind it (create_check_params), through the stand-alone program
  tests/create_check.cpp built with -fsanitize=address,undefined, on every case of tests/create_refusal_cases.py: every row of
  tests/golden/create_refusals.json -- recorded on the GPU from the library BEFORE the constructors were merged, see
  tests/test_gpu_create_refusals.py -- except the device rows must come out of the pure functions as recorded;
* the merged polynomial fit and the bank building, in the same program: a complex tap vector's coefficients are bit for bit the real
  fits of its real and of its imaginary parts, row r of a bank is bit for bit the fit (the filter banks) of row r alone;
* the library itself, without a device: every case the checks in front of the device query answer gives the recorded answer, every later
  one MRHIP_ERR_NO_DEVICE;
* the shape of the code: one descriptor per exported constructor, one fit, one tap-class refusal, the unit in the Makefile."""
import json
import os
import re
import shutil
import subprocess

import pytest

import create_refusal_cases as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multirate.jl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "create_refusals.json")


@pytest.fixture(scope="module")
def want():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def create_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("create_check") / "create_check")
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-w", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",   # (the runtime inside the program: it needs no place in the loader's library order)
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "create_check.cpp"), os.path.join(CSRC, "host_logic.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def test_the_case_list_covers_every_entry_point_and_the_table(want):
    cases = cr.cases()
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids) and sorted(ids) == sorted(want)
    assert len(cr.ENTRIES) == 16 and {c[1] for c in cases} == set(cr.ENTRIES)
    stages = {c[0]: c[2] for c in cases}
    # the recorded answers agree with the stage a case is filed under: a device row answers from the device checks, and nothing filed
    # under "args" or "params" does
    device_texts = {"device ordinal out of range", "no HIP device visible; libmultirate_hip has no CPU fallback",
                    "device is not gfx950 (MI355X); kernels are built for gfx950 only"}
    for case_id, (status, message) in want.items():
        assert (message in device_texts) == (stages[case_id] == "device"), case_id
    made = sorted(i for i, (status, _) in want.items() if status == 0)       # the one answer that is no refusal: a caller's bank of any order up to 32
    assert made == sorted(f"{n}:polyorder Nphi" for n in ("farrow_pnfb", "farrow_rates_pnfb", "farrow_pnfb_ctaps"))
    # the two groups of the ordering case: NULL h with the wrong tap class
    for name, (family, taps, bank, rates, pnfb, own) in cr.ENTRIES.items():
        short = name[len("mrhip_create_"):]
        for th in {"real": (cr.C64, cr.C128), "complex": (cr.F32, cr.F64), "either": ()}[taps]:
            status, message = want[f"{short}:wrong tap class {th}, h NULL"]
            if own:
                assert message.startswith(name + " takes ") and status == (5 if taps == "real" else 1), (name, th)
            else:
                assert (status, message) == (1, "h must hold at least one tap"), (name, th)
            assert want[f"{short}:wrong tap class {th}"][0] == (1 if taps == "complex" else 5), (name, th)
        assert want[f"{short}:tap dtype 4"] == [1, "bad tap dtype"] and want[f"{short}:tap dtype -1"] == [1, "bad tap dtype"]


def test_the_pure_checks_answer_every_case_as_recorded(create_check, want):
    cases = cr.cases()
    text = "".join(cr.text_row(case_id, name, changes) + "\n" for case_id, name, stage, changes in cases)
    p = subprocess.run([create_check], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == len(cases)
    differing, compared = [], 0
    for (case_id, name, stage, changes), line in zip(cases, lines):
        got_id, verdict, message = line.split(" | ", 2)
        got_stage, status, cleared = verdict.split()
        assert got_id == case_id
        if stage == "device":                                                # the pure functions pass such a call on (no refusal of theirs)
            assert (got_stage, int(status)) == ("params", 0), line
            continue
        compared += 1
        wstatus, wmessage = want[case_id]
        if (got_stage, int(status)) != (stage, wstatus) or (wstatus != 0 and message != wmessage) or (wstatus != 0 and cleared != "1"):
            differing.append((line, want[case_id]))
    assert not differing, differing[:8]
    assert compared == len(cases) - 2 * 16


def test_the_merged_fit_and_the_banks_row_by_row_and_component_by_component(create_check):
    p = subprocess.run([create_check, "fit"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "fit ok" and not p.stderr.strip(), (p.stdout[-2000:], p.stderr[-2000:])


def test_the_library_without_a_device(pkg, want):
    """what precedes the device query answers as recorded; everything later MRHIP_ERR_NO_DEVICE (there is no CPU path).  On a machine
    WITH a device every case answers as recorded, as in tests/test_gpu_create_refusals.py."""
    lib = pkg.load_library()
    ndev = lib.mrhip_device_count()
    buffers = cr.Buffers()
    differing = []
    for case_id, name, stage, changes in cr.cases():
        status, message, cleared = cr.run_case(lib, name, changes, buffers, max(ndev, 1))
        expected = want[case_id] if stage == "args" or ndev > 0 else [cr.NO_DEVICE, "no HIP device visible; libmultirate_hip has no CPU fallback"]
        if [status, message] != expected or (status != 0 and not cleared):
            differing.append((case_id, status, message, cleared, expected))
    assert not differing, differing[:8]


def test_one_descriptor_per_constructor_and_one_of_everything_else():
    create = open(os.path.join(CSRC, "create.hip")).read()
    header = open(os.path.join(CSRC, "create.h")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()
    logic = open(os.path.join(CSRC, "host_logic.cpp")).read()
    public = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    declared = set(re.findall(r"\bint (mrhip_create_\w+)\(", public))
    assert declared == set(cr.ENTRIES)
    rows = re.findall(r'^\s*\{kCreate(\w+),\s*kTaps(\w+),\s*(true|false),\s*(true|false),\s*(true|false),\s*"(mrhip_create_\w+)"', header, flags=re.M)
    assert len(rows) == 16 and {r[5] for r in rows} == declared
    for family, taps, bank, rates, pnfb, name in rows:                       # the table in C and the table of the cases say the same
        assert (family.lower(), taps.lower(), bank == "true", rates == "true", pnfb == "true") == cr.ENTRIES[name][:5], name
    for name in declared:                                                    # a constructor: its row of the table, then the one call
        body = re.search(r"\bint " + name + r"\([^)]*\)\s*\{(.*?)\n\}", create, flags=re.S).group(1)
        assert f'create_entry("{name}")' in body and body.count("create_filter(e, ") == 1 and len(body.strip().splitlines()) == 2, name
        assert not re.search(r"^int " + name + r"\(", api, flags=re.M)      # (mrhip_filt_once calls the public constructors)
    assert "hip" not in re.sub(r"mrhip|\.hip", "", logic.split("// ---- the constructors' host side")[1])          # no HIP call in the pure part
    assert logic.count("polyfit_rows(") == 2 and "farrow_fit" not in create + api + logic      # its definition and ONE caller
    assert (create + api + logic).count("takes Complex64 / Complex128 taps; real taps: ") == 1
    assert (create + api + logic).count("takes Float32 / Float64 taps (") == 1
    assert (create + api + logic).count('"polyorder must be in 0..min(32, Nphi-1)"') == 1 and (create + api + logic).count('"bad Nphi"') == 1
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bapi\.hip create\.hip\b", mk, flags=re.M)
    assert re.search(r"^.*create\.hip\.o.*:.*\bmrhip_filter\.h\b", mk, flags=re.M) and re.search(r"^.*create\.hip\.o.*:.*\brates_arb\.h\b.*\bcreate\.h\b", mk, flags=re.M)
