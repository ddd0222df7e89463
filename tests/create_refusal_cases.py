"""The refusals of the sixteen mrhip_create_* constructors, as data: one tiny valid call per entry point and, derived from it, one case
per answer the entry point can give -- what tests/test_gpu_create_refusals.py runs against the library on the GPU, tests/test_create_cpu.py
against the pure checks of csrc/host_logic.cpp and against the library without a device.  The expected (status, message) of every case
is tests/golden/create_refusals.json.

A case is (id, entry point, stage, changes): the valid call with `changes` applied.  `stage` says which part of the constructor
answers it: "args" the checks in front of the device query, "device" the device checks, "params" the checks behind them."""
import ctypes as C

import numpy as np

F32, F64, C64, C128 = 0, 1, 2, 3
HLEN, NPHI, POLYORDER, NCH, NUM, DEN, RATE = 8, 4, 2, 2, 3, 2, 1.5
RATES = (1.5, 0.75)
NO_DEVICE = 4

# name: (family, tap class accepted, bank, rates, pnfb, has a tap-class refusal of its own)
ENTRIES = {
    "mrhip_create_rational": ("rational", "either", False, False, False, False),
    "mrhip_create_rational_bank": ("rational", "real", True, False, False, True),
    "mrhip_create_rational_bank_ctaps": ("rational", "complex", True, False, False, True),
    "mrhip_create_arbitrary": ("arbitrary", "real", False, False, False, False),
    "mrhip_create_arbitrary_ctaps": ("arbitrary", "complex", False, False, False, True),
    "mrhip_create_arbitrary_bank": ("arbitrary", "real", True, False, False, True),
    "mrhip_create_arbitrary_bank_ctaps": ("arbitrary", "complex", True, False, False, True),
    "mrhip_create_arbitrary_rates": ("arbitrary", "real", False, True, False, True),
    "mrhip_create_farrow": ("farrow", "real", False, False, False, False),
    "mrhip_create_farrow_bank": ("farrow", "real", True, False, False, True),
    "mrhip_create_farrow_pnfb": ("farrow", "real", False, False, True, False),
    "mrhip_create_farrow_rates": ("farrow", "real", False, True, False, True),
    "mrhip_create_farrow_rates_pnfb": ("farrow", "real", False, True, True, True),
    "mrhip_create_farrow_ctaps": ("farrow", "complex", False, False, False, True),
    "mrhip_create_farrow_bank_ctaps": ("farrow", "complex", True, False, False, True),
    "mrhip_create_farrow_pnfb_ctaps": ("farrow", "complex", False, False, True, True),
}


def valid_call(name):
    """the arguments of the one valid call of an entry point, by name"""
    family, taps, bank, rates, pnfb, _ = ENTRIES[name]
    a = {"h": "taps", "hLen": HLEN, "th": C64 if taps == "complex" else F32, "tx": F32, "nch": NCH, "device": 0, "out": "out"}
    if family == "rational":
        a.update(num=NUM, den=DEN)
    else:
        a.update(Nphi=NPHI, **({"rates": RATES} if rates else {"rate": RATE}))
    if family == "farrow":
        a.update(polyorder=POLYORDER)
    return a


def cases():
    """[(id, entry point, stage, changes)]"""
    out = []
    for name, (family, taps, bank, rates, pnfb, own_refusal) in ENTRIES.items():
        def add(what, stage, **changes):
            out.append((f"{name[len('mrhip_create_'):]}:{what}", name, stage, changes))
        add("out NULL", "args", out=None)
        add("h NULL", "args", h=None)
        add("hLen 0", "args", hLen=0)
        add("tap dtype -1", "args", th=-1)
        add("tap dtype 4", "args", th=4)
        wrong = {"real": (C64, C128), "complex": (F32, F64), "either": ()}[taps]
        for th in wrong:
            add(f"wrong tap class {th}", "args", th=th)
            add(f"wrong tap class {th}, h NULL", "args", th=th, h=None)      # entry points with a refusal of their own give it first
        if wrong:
            add(f"wrong tap class {wrong[0]}, out NULL", "args", th=wrong[0], out=None)
        add("sample dtype -1", "args", tx=-1)
        add("sample dtype 4", "args", tx=4)
        add("nch 0", "args", nch=0)
        add("device -1", "device", device=-1)
        add("device count", "device", device="count")
        if family == "rational":
            add("ratio 0", "params", num=0)
            add("ratio 0 in the denominator", "params", den=0)
            add("ratio negative", "params", num=-NUM)
            add("num 2^31", "params", num=2 ** 31, den=1)
            add("num 2^31 + 1 over 2^31", "params", num=2 ** 31 + 1, den=2 ** 31)
            continue
        if rates:
            add("rates NULL", "params", rates=None)
            add("one rate 0", "params", rates=(RATE, 0.0))
            add("one rate negative", "params", rates=(-RATE, RATE))
            add("one rate inf", "params", rates=(RATE, float("inf")))
            add("one rate NaN", "params", rates=(float("nan"), RATE))
            add("one rate 2^-31", "params", rates=(RATE, 2.0 ** -31))
            add("one rate 2^-31 in front of a rate 0", "params", rates=(2.0 ** -31, 0.0))
        else:
            add("rate 0", "params", rate=0.0)
            add("rate negative", "params", rate=-RATE)
            add("rate NaN", "params", rate=float("nan"))
        add("Nphi 0", "params", Nphi=0)
        add("rate 0 and Nphi 0", "params", Nphi=0, **({"rates": (0.0, RATE)} if rates else {"rate": 0.0}))      # the rate is looked at first
        if family == "farrow":
            add("polyorder -1", "params", polyorder=-1)
            add("polyorder 33", "params", polyorder=33)
            # a fitted bank: refused (polyorder + 1 > Nphi); a caller's bank: nothing is fitted, the filter is made (status 0)
            add("polyorder Nphi", "params", polyorder=NPHI)
            add("Nphi 0 and polyorder -1", "params", Nphi=0, polyorder=-1)
    return out


class Buffers:
    """what the pointers of a call point to: 8 taps a channel (real or complex, 32 bits), and a polynomial bank large enough for every
    polyorder a case asks for (2 taps per phase, up to 34 coefficients, pairs)"""

    def __init__(self):
        rng = np.random.default_rng(5)
        self.real = rng.standard_normal((NCH, HLEN)).astype(np.float32)
        self.cplx = (rng.standard_normal((NCH, HLEN)) + 1j * rng.standard_normal((NCH, HLEN))).astype(np.complex64)
        self.pnfb = rng.standard_normal(2 * 34 * 2)

    def taps(self, name, th):
        if ENTRIES[name][4]:
            return self.pnfb
        return self.cplx if th in (C64, C128) else self.real


def call_args(name, changes, buffers, device_count=1):
    """(ctypes arguments, the out cell or None, the arrays to keep alive) of the valid call of `name` with `changes`"""
    a = valid_call(name)
    a.update(changes)
    if a["device"] == "count":
        a["device"] = device_count
    # (a wrong tap class: the valid buffer stays -- the refusal comes before anything reads it)
    taps = buffers.taps(name, valid_call(name)["th"])
    keep = [taps]
    h = None if a["h"] is None else taps.ctypes.data_as(C.c_void_p)
    out = None if a["out"] is None else C.c_void_p(0xdead0)          # not NULL: the constructor has to clear it
    if "num" in a:
        middle = [a["num"], a["den"]]
    else:
        if "rates" in a:
            r = None if a["rates"] is None else np.array(a["rates"], dtype=np.float64)
            keep.append(r)
            first = None if r is None else r.ctypes.data_as(C.c_void_p)
        else:
            first = a["rate"]
        middle = [first, a["Nphi"]] + ([a["polyorder"]] if "polyorder" in a else [])
    args = [h, a["hLen"], a["th"]] + middle + [a["tx"], a["nch"], a["device"], None if out is None else C.byref(out)]
    return args, out, keep


def run_case(lib, name, changes, buffers, device_count=1):
    """-> (status, message, *out is NULL afterwards or out was NULL).  A filter that was made is destroyed."""
    args, out, keep = call_args(name, changes, buffers, device_count)
    status = getattr(lib, name)(*args)
    message = "" if status == 0 else lib.mrhip_last_error().decode("utf-8", "replace")
    cleared = out is None or not out.value
    if status == 0 and out is not None and out.value:
        lib.mrhip_destroy(out)
    return status, message, cleared


def text_row(case_id, name, changes):
    """the case for tests/create_check.cpp: id | name h_null out_null hLen th tx nch num den rate nrates r0 r1 Nphi polyorder (nrates -1: not a
    constructor with rates, 0: rates NULL)"""
    a = valid_call(name)
    a.update(changes)
    rates = a.get("rates", ())
    nr = -1 if "rates" not in a else (0 if rates is None else len(rates))
    r = list(rates or ()) + [0.0, 0.0]
    f = [name, int(a["h"] is None), int(a["out"] is None), a["hLen"], a["th"], a["tx"], a["nch"], a.get("num", 1), a.get("den", 1),
         repr(float(a.get("rate", 0.0))), nr, repr(float(r[0])), repr(float(r[1])), a.get("Nphi", 1), a.get("polyorder", 0)]
    return case_id + " | " + " ".join(str(v) for v in f)
