#!/usr/bin/env python3
"""Per-channel taps (FIRFilter.per_channel, csrc/kernels_bank.hip) against what a user did before, on one MI355X.

Three workloads, each run five ways:
  (a) the bank filter on poly_bank_tiled_kernel (MRHIP_BANK_TILED=1)
  (b) the bank filter on poly_bank_generic_kernel (MRHIP_BANK_TILED=0)
  (c) filt_multi over nch one-channel filters (one prepared MultiStream launch per pass)
  (d) the loop of nch single calls on one-channel filters
  (e) the ordinary shared-taps filter of the same shape: the floor the tuned kernels set
Wall time of one pass over the whole signal, host clock around work that ends in a device synchronise; the clocks are settled as
in scripts/bench_configs.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed
repeats per row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).

    python scripts/bench_bank.py [w1 w2 w3] [--out FILE]
"""
import os
import statistics
import sys
import time
from fractions import Fraction

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels with MRHIP_BANK_TILED between calls)
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
    "w1": ("64 ch x 1e6 Float32 147//160, 3528 taps", 64, 1_000_000, torch.float32, Fraction(147, 160), 3528),
    "w2": ("64 ch x 1e6 ComplexF32 1//4, 128 taps", 64, 1_000_000, torch.complex64, Fraction(1, 4), 128),
    "w3": ("4096 ch x 1e4 Float32 3//5, 33 taps", 4096, 10_000, torch.float32, Fraction(3, 5), 33),
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
    title, nch, n, dtype, ratio, ntaps = WORKLOADS[key]
    rng = np.random.default_rng(7)
    H = (rng.standard_normal((nch, ntaps)) / ntaps).astype(np.float32)
    if dtype.is_complex:
        x = torch.view_as_complex(torch.rand((nch, n, 2), device=dev, dtype=torch.float32))
    else:
        x = torch.rand((nch, n), device=dev, dtype=dtype)
    emit(f"## {title}")
    emit(f"{'way':<44}{'kernel':<28}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass)
        rows[name[1]] = ts
        emit(f"{name:<44}{kernel():<28}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (a), (b): the bank filter
    f = pkg.FIRFilter.per_channel(H, ratio)
    f.bind(np.dtype(str(dtype).replace("torch.", "")), nch)
    ybuf = torch.empty((nch, f.outputlength_bound(n)), dtype=TORCH_OF[np.dtype(f.output_dtype)], device=dev)
    for name, mode in (("(a) bank filter, tiled kernel", "1"), ("(b) bank filter, universal kernel", "0")):
        os.environ["MRHIP_BANK_TILED"] = mode
        row(name, f.last_kernel_name, lambda: f.filt_into(ybuf, x))
    os.environ.pop("MRHIP_BANK_TILED")
    f.filt_into(ybuf, x)
    emit(f"    (default plan, MRHIP_BANK_TILED unset: {f.last_kernel_name()})")
    f.close()
    # (c), (d): one-channel filters
    fs = [pkg.FIRFilter(H[c], ratio) for c in range(nch)]
    xs = [x[c] for c in range(nch)]
    for fc, xc in zip(fs, xs):
        fc.bind(np.dtype(str(dtype).replace("torch.", "")), 1)
    bound = fs[0].outputlength_bound(n)
    ys = [ybuf[c, :bound] for c in range(nch)]
    ms = pkg.MultiStream(fs, ys, xs)
    row("(c) filt_multi over one-channel filters", fs[0].last_kernel_name, ms.run)

    def loop():
        for fc, yc, xc in zip(fs, ys, xs):
            fc.filt_into(yc, xc)
    row("(d) loop of single calls", fs[0].last_kernel_name, loop)
    for fc in fs:
        fc.close()
    # (e): the shared-taps filter
    g = pkg.FIRFilter(H[0], ratio)
    row("(e) shared-taps filter (the floor)", g.last_kernel_name, lambda: g.filt_into(ybuf, x))
    g.close()
    med = {k: statistics.median(v) for k, v in rows.items()}
    spread = max(rows["a"]) - min(rows["a"]), max(rows["b"]) - min(rows["b"])
    emit(f"    (a) vs (b): {med['b'] / med['a']:.2f}x (spread of the repeats: a {spread[0]:.3f} ms, b {spread[1]:.3f} ms); "
         f"(a) vs (c): {med['c'] / med['a']:.2f}x; (a) vs (d): {med['d'] / med['a']:.2f}x; (a) vs (e): {med['e'] / med['a']:.2f}x")
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
