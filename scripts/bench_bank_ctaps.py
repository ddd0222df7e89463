#!/usr/bin/env python3
"""Per-channel complex taps (FIRFilter.per_channel_complex_taps, csrc/kernels_bank_ctaps.hip) against what a user did before, on one MI355X.

Three workloads (and a fourth in Float64 arithmetic), each run six ways:
  (a) the new filter on poly_bank_ctaps_tiled_kernel (MRHIP_BANK_CTAPS_TILED=1)
  (b) the new filter on poly_bank_ctaps_generic_kernel (MRHIP_BANK_CTAPS_TILED=0)
  (c) filt_multi over nch one-channel complex_taps filters (one prepared MultiStream call per pass; the library serves complex taps
      as single calls inside it)
  (d) the loop of nch single calls on one-channel complex_taps filters
  (e) what a user did before with one filter object: two real bank filters, per_channel(real(H)) and per_channel(imag(H)), plus the
      torch combine (complex samples: yr + 1j * yi; real samples: torch.complex(yr, yi)) -- other roundings than the reference
  (f) the shared-taps complex_taps filter of the same shape: the floor
Taps: one Float32 low-pass prototype rotated to every channel's own centre frequency, h_c[n] = h[n] exp(j w_c n), Complex64 (w4: Float64, Complex128).
Wall time of one pass over the whole signal, host clock around work that ends in a device synchronise; the clocks are settled as
in scripts/bench_bank.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats per
row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).

    python scripts/bench_bank_ctaps.py [w1 w2 w3 w4] [--out FILE]
"""
import os
import statistics
import sys
import time
from fractions import Fraction

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels with MRHIP_BANK_CTAPS_TILED between calls)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda", 0)
SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "60"))
REPS = 5
WORKLOADS = {
    "w1": ("4096 ch x 1e4 ComplexF32 1//4, 33 Complex64 taps", 4096, 10_000, torch.complex64, Fraction(1, 4), 33, np.complex64),
    "w2": ("64 ch x 1e6 ComplexF32 1//4, 128 Complex64 taps", 64, 1_000_000, torch.complex64, Fraction(1, 4), 128, np.complex64),
    "w3": ("64 ch x 1e6 Float32 147//160, 3528 Complex64 taps", 64, 1_000_000, torch.float32, Fraction(147, 160), 3528, np.complex64),
    # (Float64 arithmetic, beyond the three shapes the feature was asked for: the default plan is not left unmeasured there)
    "w4": ("64 ch x 1e6 ComplexF64 1//4, 128 Complex128 taps", 64, 1_000_000, torch.complex128, Fraction(1, 4), 128, np.complex128),
}
TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128}


def timed(one_pass):
    """settle, then REPS timed passes: (times in ms, untimed passes)"""
    t0 = time.perf_counter()
    for i in range(20):
        one_pass()
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) * 1e3
        if i >= 1 and el >= SETTLE_MS:
            break
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        one_pass()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out, i + 1


def workload(key, emit):
    title, nch, n, dtype, ratio, ntaps, th = WORKLOADS[key]
    rng = np.random.default_rng(7)
    proto = (rng.standard_normal(ntaps) / ntaps).astype(np.float32 if th == np.complex64 else np.float64)
    w = 2 * np.pi * (np.arange(nch) / nch - 0.5)
    H = (proto[None, :] * np.exp(1j * w[:, None] * np.arange(ntaps)[None, :])).astype(th)
    np_tx = np.dtype(str(dtype).replace("torch.", ""))
    if dtype.is_complex:
        x = torch.view_as_complex(torch.rand((nch, n, 2), device=dev, dtype=torch.float64 if dtype == torch.complex128 else torch.float32))
    else:
        x = torch.rand((nch, n), device=dev, dtype=dtype)
    emit(f"## {title}")
    emit(f"{'way':<54}{'kernel':<32}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass)
        rows[name[1]] = ts
        emit(f"{name:<54}{kernel():<32}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (a), (b): the new filter
    f = pkg.FIRFilter.per_channel_complex_taps(H, ratio)
    f.bind(np_tx, nch)
    bound = f.outputlength_bound(n)
    ybuf = torch.empty((nch, bound), dtype=TORCH_OF[np.dtype(f.output_dtype)], device=dev)
    for name, mode in (("(a) bank-ctaps filter, tiled kernel", "1"), ("(b) bank-ctaps filter, universal kernel", "0")):
        os.environ["MRHIP_BANK_CTAPS_TILED"] = mode
        row(name, f.last_kernel_name, lambda: f.filt_into(ybuf, x))
    os.environ.pop("MRHIP_BANK_CTAPS_TILED")
    f.filt_into(ybuf, x)
    emit(f"    (default plan, MRHIP_BANK_CTAPS_TILED unset: {f.last_kernel_name()})")
    f.close()
    # (c), (d): one-channel complex_taps filters
    fs = [pkg.FIRFilter.complex_taps(H[c], ratio) for c in range(nch)]
    xs = [x[c] for c in range(nch)]
    for fc in fs:
        fc.bind(np_tx, 1)
    ys = [ybuf[c, :bound] for c in range(nch)]
    ms = pkg.MultiStream(fs, ys, xs)
    row("(c) filt_multi over one-channel complex_taps filters", fs[0].last_kernel_name, ms.run)

    def loop():
        for fc, yc, xc in zip(fs, ys, xs):
            fc.filt_into(yc, xc)
    row("(d) loop of single calls", fs[0].last_kernel_name, loop)
    for fc in fs:
        fc.close()
    # (e): two real bank filters and the combine
    fr = pkg.FIRFilter.per_channel(np.ascontiguousarray(H.real), ratio)
    fi = pkg.FIRFilter.per_channel(np.ascontiguousarray(H.imag), ratio)
    fr.bind(np_tx, nch), fi.bind(np_tx, nch)
    yr = torch.empty((nch, bound), dtype=TORCH_OF[np.dtype(fr.output_dtype)], device=dev)
    yi = torch.empty_like(yr)

    def two_real():
        fr.filt_into(yr, x)
        fi.filt_into(yi, x)
        return yr + 1j * yi if dtype.is_complex else torch.complex(yr, yi)
    row("(e) two real bank filters + torch combine", fr.last_kernel_name, two_real)
    fr.close(), fi.close()
    # (f): the shared-taps filter
    g = pkg.FIRFilter.complex_taps(H[0], ratio)
    row("(f) shared-taps complex_taps filter (the floor)", g.last_kernel_name, lambda: g.filt_into(ybuf, x))
    g.close()
    med = {k: statistics.median(v) for k, v in rows.items()}
    spread = max(rows["a"]) - min(rows["a"]), max(rows["b"]) - min(rows["b"])
    emit(f"    (a) vs (b): {med['b'] / med['a']:.2f}x (spread of the repeats: a {spread[0]:.3f} ms, b {spread[1]:.3f} ms); "
         f"(a) vs (c): {med['c'] / med['a']:.2f}x; (a) vs (d): {med['d'] / med['a']:.2f}x; (a) vs (e): {med['e'] / med['a']:.2f}x; "
         f"(a) vs (f): {med['f'] / med['a']:.2f}x")
    emit("")


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = open(args[i + 1], "a")
        del args[i:i + 2]

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for key in args or list(WORKLOADS):
        workload(key, emit)


if __name__ == "__main__":
    main()
