#!/usr/bin/env python3
"""Per-channel taps with per-channel rates for FIRArbitrary (FIRFilter.per_channel_taps_and_rates, mrhip_set_channel_taps,
the BANK kernels of csrc/kernels_rates_arb.hip) against what a user did before, on one MI355X.

The three workloads of DESIGN.md 9 items 17, 18 and 21 (w1 ... w3: Float32, Nphi 32, the rates spread evenly over [2.0, 2.25], every
channel with taps of its own), each run five ways:
  (a) the new filter on the tiled kernel (MRHIP_ARB_RATES_BANK_TILED=1; reported as arb_rates_bank_tiled)
  (b) the new filter on the universal kernel (MRHIP_ARB_RATES_BANK_TILED=0; reported as arb_rates_bank_generic)
  (c) filt_multi over nch one-channel FIRFilter(H[c], rates[c], Nphi) filters: what a user does today (mrhip_filt_device_multi issues
      single calls for this kind).  Over the first BENCH_SINGLES_MAX = 256 channels only when nch is larger, the row says so: every
      one-channel FIRArbitrary filter holds its own schedule buffers in host memory; the time for all nch channels is then the row's
      figure times nch / 256, this way being one launch sequence per channel
  (d) the shared-taps FIRFilter.per_channel_rates(H[0], rates, Nphi) of the same shape on its default plan: the floor
  (e) the new filter on its default plan with set_channel_taps(H) before every pass: the cost of an adaptive update, the host's banks,
      the wait for the filter's stream and the upload included
Wall time of one pass over the whole signal, host clock around work that ends in a device synchronise; the clocks are settled as in
scripts/bench_arb_rates.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats per
row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).

    python scripts/bench_arb_rates_bank.py [w1 w2 w3] [--out FILE]
"""
import os
import statistics
import sys
import time

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels with MRHIP_ARB_RATES_BANK_TILED between calls)
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
    "w1": ("4096 ch x 1e4 Float32, rates 2.0 ... 2.25, Nphi 32, 250 taps a channel", 4096, 10_000, 32, 250),
    "w2": ("256 ch x 1e5 Float32, rates 2.0 ... 2.25, Nphi 32, 1024 taps a channel", 256, 100_000, 32, 1024),
    "w3": ("64 ch x 1e6 Float32, rates 2.0 ... 2.25, Nphi 32, 1024 taps a channel", 64, 1_000_000, 32, 1024),
}


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
    title, nch, n, Nphi, ntaps = WORKLOADS[key]
    rng = np.random.default_rng(7)
    H = (rng.standard_normal((nch, ntaps)) * Nphi / ntaps).astype(np.float32)
    rates = np.linspace(2.0, 2.25, nch)
    x = torch.rand((nch, n), device=dev, dtype=torch.float32)
    f = pkg.FIRFilter.per_channel_taps_and_rates(H, rates, Nphi)
    f.bind(np.float32, nch)
    bound = f.outputlength_bound(n)
    ybuf = torch.empty((nch, bound), dtype=torch.float32, device=dev)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    tiles_per_channel = -(-bound // 256)
    emit(f"## {title}")
    emit(f"    (bound {bound} outputs a channel: {tiles_per_channel} tiles a channel, {tiles_per_channel * nch} tiles; device banks {H.size * 2 * 4} bytes)")
    emit(f"{'way':<58}{'kernel':<28}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass)
        rows[name[1]] = ts
        emit(f"{name:<58}{kernel():<28}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (a), (b): the new filter (nothing waits inside the call: the counts stay on the device)
    for name, mode in (("(a) new filter, tiled kernel", "1"), ("(b) new filter, universal kernel", "0")):
        os.environ["MRHIP_ARB_RATES_BANK_TILED"] = mode
        row(name, f.last_kernel_name, lambda: f._filt_into_rates(ybuf, x, counts))
    os.environ.pop("MRHIP_ARB_RATES_BANK_TILED")
    f._filt_into_rates(ybuf, x, counts)
    default = "a" if f.last_kernel_name() == "arb_rates_bank_tiled" else "b"
    emit(f"    (default plan, MRHIP_ARB_RATES_BANK_TILED unset: {f.last_kernel_name()}; outputs of the last pass: {int(counts.sum())})")

    # (e): an adaptive update before every pass
    def adaptive():
        f.set_channel_taps(H)
        f._filt_into_rates(ybuf, x, counts)
    row("(e) new filter, default plan, set_channel_taps each pass", f.last_kernel_name, adaptive)
    f.close()
    # (c): one-channel filters, each with its own taps at its own rate
    ns = min(nch, SINGLES_MAX)
    part = "" if ns == nch else f", first {ns} ch only"
    fs = [pkg.FIRFilter(H[c], float(rates[c]), Nphi) for c in range(ns)]
    xs = [x[c] for c in range(ns)]
    for fc in fs:
        fc.bind(np.float32, 1)
    ys = [ybuf[c, :bound] for c in range(ns)]
    ms = pkg.MultiStream(fs, ys, xs)
    row("(c) filt_multi, one-channel filters" + part, fs[0].last_kernel_name, ms.run)
    for fc in fs:
        fc.close()
    # (d): the shared-taps filter with per-channel rates
    g = pkg.FIRFilter.per_channel_rates(H[0], rates, Nphi)
    g.bind(np.float32, nch)
    row("(d) shared-taps per_channel_rates, default plan (floor)", g.last_kernel_name, lambda: g._filt_into_rates(ybuf, x, counts))
    g.close()
    med = {k: statistics.median(v) for k, v in rows.items()}
    med["c"] *= nch / ns                          # (one launch sequence per channel: scaled to all nch channels)
    spread = max(rows["a"]) - min(rows["a"]), max(rows["b"]) - min(rows["b"])
    best = min(med["a"], med["b"])
    emit(f"    (b) / (a): {med['b'] / med['a']:.3f}x (spread of the repeats: a {spread[0]:.3f} ms, b {spread[1]:.3f} ms); "
         f"(c) / best: {med['c'] / best:.2f}x; best / (d): {best / med['d']:.2f}x; (e) - ({default}): {med['e'] - med[default]:.3f} ms (best: the faster of (a), (b))")
    if ns != nch:
        emit(f"    ((c) in the ratios: the measured row times {nch}/{ns} = {med['c']:.1f} ms for all {nch} channels)")
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
