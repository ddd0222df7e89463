#!/usr/bin/env python3
"""Per-channel complex taps for FIRArbitrary (FIRFilter.per_channel_complex_taps_arbitrary, csrc/kernels_bank_arb_ctaps.hip) against what
a user did before, on one MI355X.

The six workloads of DESIGN.md 9 item 15 (w1 ... w6), each run six ways:
  (a) the new filter on arb_bank_ctaps_tiled_kernel (MRHIP_ARB_BANK_CTAPS_TILED=1)
  (b) the new filter on arb_bank_ctaps_generic_kernel (MRHIP_ARB_BANK_CTAPS_TILED=0)
  (c) filt_multi over nch one-channel FIRFilter.complex_taps_arbitrary filters (mrhip_filt_device_multi issues single calls for this kind)
  (d) the loop of nch single calls on one-channel filters
      ((c) and (d) over the first BENCH_SINGLES_MAX = 256 channels only when nch is larger, the row says so: every one-channel
      FIRArbitrary filter holds its own schedule buffers in host memory; the time for all nch channels is then the row's figure times
      nch / 256, these ways being one launch sequence per channel)
  (e) two real bank filters, per_channel_arbitrary(real(H)) and per_channel_arbitrary(imag(H)), plus the torch combine pass (for
      complex samples: y = (yr.re - yi.im) + i (yr.im + yi.re); its roundings are not the reference's)
  (f) the shared-taps FIRFilter.complex_taps_arbitrary filter of the same shape, on whatever kernel the dispatcher picks: the floor
Wall time of one pass over the whole signal, host clock around work that ends in a device synchronise; the clocks are settled as
in scripts/bench_arb_bank.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats
per row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).

    python scripts/bench_arb_bank_ctaps.py [w1 ... w6] [--out FILE]
"""
import os
import statistics
import sys
import time

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels with MRHIP_ARB_BANK_CTAPS_TILED between calls)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda", 0)
SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "60"))
REPS = 5
SINGLES_MAX = int(os.environ.get("BENCH_SINGLES_MAX", "256"))
WORKLOADS = {
    "w1": ("64 ch x 1e6 Float32, rate 2.123, Nphi 32, 1024 Complex64 taps", 64, 1_000_000, np.float32, 2.123, 32, 1024),
    "w2": ("64 ch x 1e6 Float32, rate 0.47, Nphi 32, 1024 Complex64 taps", 64, 1_000_000, np.float32, 0.47, 32, 1024),
    "w3": ("64 ch x 1e6 ComplexF32, rate 2.123, Nphi 32, 1024 Complex64 taps", 64, 1_000_000, np.complex64, 2.123, 32, 1024),
    "w4": ("4096 ch x 1e4 ComplexF32, rate 2.123, Nphi 32, 250 Complex64 taps", 4096, 10_000, np.complex64, 2.123, 32, 250),
    "w5": ("64 ch x 1e4 ComplexF32, rate 2.123, Nphi 32, 250 Complex64 taps (5312 tiles)", 64, 10_000, np.complex64, 2.123, 32, 250),
    "w6": ("4 ch x 2e4 ComplexF32, rate 2.123, Nphi 32, 250 Complex64 taps (664 tiles)", 4, 20_000, np.complex64, 2.123, 32, 250),
}
TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.complex64): torch.complex64}


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
    title, nch, n, dt, rate, Nphi, ntaps = WORKLOADS[key]
    rng = np.random.default_rng(7)
    H = ((rng.standard_normal((nch, ntaps)) + 1j * rng.standard_normal((nch, ntaps))) / ntaps).astype(np.complex64)
    x = torch.rand((nch, n), device=dev, dtype=torch.float32)
    if np.dtype(dt).kind == "c":
        x = torch.complex(x, torch.rand((nch, n), device=dev, dtype=torch.float32))
    emit(f"## {title}")
    emit(f"{'way':<52}{'kernel':<32}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass)
        rows[name[1]] = ts
        emit(f"{name:<52}{kernel():<32}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (a), (b): the new filter
    f = pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, rate, Nphi)
    f.bind(np.dtype(dt), nch)
    bound = f.outputlength_bound(n)
    ybuf = torch.empty((nch, bound), dtype=torch.complex64, device=dev)
    for name, mode in (("(a) new filter, tiled kernel", "1"), ("(b) new filter, universal kernel", "0")):
        os.environ["MRHIP_ARB_BANK_CTAPS_TILED"] = mode
        row(name, f.last_kernel_name, lambda: f.filt_into(ybuf, x))
    os.environ.pop("MRHIP_ARB_BANK_CTAPS_TILED")
    f.filt_into(ybuf, x)
    emit(f"    (default plan, MRHIP_ARB_BANK_CTAPS_TILED unset: {f.last_kernel_name()})")
    f.close()
    # (c), (d): one-channel complex-tap filters
    ns = min(nch, SINGLES_MAX)
    part = "" if ns == nch else f", first {ns} ch only"
    fs = [pkg.FIRFilter.complex_taps_arbitrary(H[c], rate, Nphi) for c in range(ns)]
    xs = [x[c] for c in range(ns)]
    for fc in fs:
        fc.bind(np.dtype(dt), 1)
    ys = [ybuf[c, :bound] for c in range(ns)]
    ms = pkg.MultiStream(fs, ys, xs)
    row("(c) filt_multi, one-channel filters" + part, fs[0].last_kernel_name, ms.run)

    def loop():
        for fc, yc, xc in zip(fs, ys, xs):
            fc.filt_into(yc, xc)
    row("(d) loop of single calls" + part, fs[0].last_kernel_name, loop)
    for fc in fs:
        fc.close()
    # (e): two real bank filters and the combine pass
    fr = pkg.FIRFilter.per_channel_arbitrary(np.ascontiguousarray(H.real), rate, Nphi)
    fi = pkg.FIRFilter.per_channel_arbitrary(np.ascontiguousarray(H.imag), rate, Nphi)
    fr.bind(np.dtype(dt), nch), fi.bind(np.dtype(dt), nch)
    part_dtype = TORCH_OF[np.dtype(dt)]
    yr = torch.empty((nch, bound), dtype=part_dtype, device=dev)
    yi = torch.empty((nch, bound), dtype=part_dtype, device=dev)

    def two_real_banks():
        fr.filt_into(yr, x)
        fi.filt_into(yi, x)
        if part_dtype == torch.float32:
            torch.complex(yr, yi, out=ybuf)
        else:
            torch.complex(yr.real - yi.imag, yr.imag + yi.real, out=ybuf)
    row("(e) two real bank filters + combine", fr.last_kernel_name, two_real_banks)
    fr.close(), fi.close()
    del yr, yi
    # (f): the shared-taps filter
    g = pkg.FIRFilter.complex_taps_arbitrary(H[0], rate, Nphi)
    row("(f) shared-taps filter (the floor)", g.last_kernel_name, lambda: g.filt_into(ybuf, x))
    g.close()
    med = {k: statistics.median(v) for k, v in rows.items()}
    for k in "cd":
        med[k] *= nch / ns                        # (one launch sequence per channel: scaled to all nch channels)
    spread = max(rows["a"]) - min(rows["a"]), max(rows["b"]) - min(rows["b"])
    best = min(med["a"], med["b"])
    emit(f"    (b) / (a): {med['b'] / med['a']:.2f}x (spread of the repeats: a {spread[0]:.3f} ms, b {spread[1]:.3f} ms); "
         f"(c) / best: {med['c'] / best:.2f}x; (d) / best: {med['d'] / best:.2f}x; (e) / best: {med['e'] / best:.2f}x; "
         f"best / (f): {best / med['f']:.2f}x (best: the faster of (a), (b))")
    if ns != nch:
        emit(f"    ((c) and (d) in the ratios: the measured rows times {nch}/{ns} = {med['c']:.1f} and {med['d']:.1f} ms for all {nch} channels)")
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
