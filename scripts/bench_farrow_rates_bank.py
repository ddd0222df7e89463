#!/usr/bin/env python3
"""Per-channel taps with per-channel rates for FIRFarrow (FIRFilter.per_channel_taps_and_rates_farrow, mrhip_set_channel_taps_farrow,
mrhip_set_channel_pnfb, the BANK kernels of csrc/kernels_rates_farrow.hip) against what a user did before, on one MI355X.

The three workloads of DESIGN.md 9 items 17, 18, 21 and 22 (w1 ... w3: Float32, Nphi 32, polyorder 4, the rates spread evenly over
[2.0, 2.25], every channel with taps of its own), each run these ways:
  (a) the new filter on the multi kernel (MRHIP_FARROW_RATES_BANK_MULTI=1; reported as farrow_rates_bank_multi)
  (b) the new filter on the universal kernel (MRHIP_FARROW_RATES_BANK_MULTI=0; reported as farrow_rates_bank_generic)
  (c) filt_multi over nch one-channel FIRFilter(H[c], rates[c], Nphi, polyorder) filters: what a user does today (mrhip_filt_device_multi
      issues single calls for this kind).  Over the first BENCH_SINGLES_MAX = 256 channels only when nch is larger, the row says so:
      every one-channel FIRFarrow filter holds its own schedule buffers in host memory; the time for all nch channels is then the row's
      figure times nch / 256, this way being one launch sequence per channel
  (d) the shared-taps FIRFilter.per_channel_rates_farrow(H[0], rates, Nphi, polyorder) of the same shape on its default plan: the floor
  (e) one set_channel_taps_farrow(H) of all channels, alone: the fit of every row, the wait for the filter's (idle) stream and the upload
  (f) one set_channel_pnfb(PN) of all channels, alone: the rounding, the wait and the upload -- no fit; (e) - (f) is the fit
Wall time of one pass over the whole signal (or of one call, (e) and (f)), host clock around work that ends in a device synchronise; the
clocks are settled as in scripts/bench_arb_rates.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then
five timed repeats per row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).

    python scripts/bench_farrow_rates_bank.py [w1 w2 w3] [--out FILE]
"""
import os
import statistics
import sys
import time

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels with MRHIP_FARROW_RATES_BANK_MULTI between calls)
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
POLYORDER = 4
WORKLOADS = {
    "w1": ("4096 ch x 1e4 Float32, rates 2.0 ... 2.25, Nphi 32, 250 taps a channel, polyorder 4", 4096, 10_000, 32, 250),
    "w2": ("256 ch x 1e5 Float32, rates 2.0 ... 2.25, Nphi 32, 1024 taps a channel, polyorder 4", 256, 100_000, 32, 1024),
    "w3": ("64 ch x 1e6 Float32, rates 2.0 ... 2.25, Nphi 32, 1024 taps a channel, polyorder 4", 64, 1_000_000, 32, 1024),
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
    f = pkg.FIRFilter.per_channel_taps_and_rates_farrow(H, rates, Nphi, POLYORDER)
    f.bind(np.float32, nch)
    PN = f.pnfb()
    bound = f.outputlength_bound(n)
    ybuf = torch.empty((nch, bound), dtype=torch.float32, device=dev)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    tiles_per_channel = -(-bound // 1024)
    emit(f"## {title}")
    emit(f"    (bound {bound} outputs a channel: {tiles_per_channel} tiles a channel, {tiles_per_channel * nch} tiles; device banks {PN.size * 8} bytes)")
    emit(f"{'way':<58}{'kernel':<28}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass)
        rows[name[1]] = ts
        emit(f"{name:<58}{kernel():<28}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (a), (b): the new filter (nothing waits inside the call: the counts stay on the device)
    for name, mode in (("(a) new filter, multi kernel", "1"), ("(b) new filter, universal kernel", "0")):
        os.environ["MRHIP_FARROW_RATES_BANK_MULTI"] = mode
        row(name, f.last_kernel_name, lambda: f._filt_into_rates(ybuf, x, counts))
    os.environ.pop("MRHIP_FARROW_RATES_BANK_MULTI")
    f._filt_into_rates(ybuf, x, counts)
    torch.cuda.synchronize()
    emit(f"    (default plan, MRHIP_FARROW_RATES_BANK_MULTI unset: {f.last_kernel_name()}; outputs of the last pass: {int(counts.sum())})")
    # (e), (f): the two calls alone, on an idle filter
    row("(e) set_channel_taps_farrow(H), all channels, alone", lambda: "-", lambda: f.set_channel_taps_farrow(H))
    row("(f) set_channel_pnfb(PN), all channels, alone", lambda: "-", lambda: f.set_channel_pnfb(PN))
    f.close()
    # (c): one-channel filters, each with its own taps at its own rate
    ns = min(nch, SINGLES_MAX)
    part = "" if ns == nch else f", first {ns} ch only"
    fs = [pkg.FIRFilter(H[c], float(rates[c]), Nphi, POLYORDER) for c in range(ns)]
    xs = [x[c] for c in range(ns)]
    for fc in fs:
        fc.bind(np.float32, 1)
    ys = [ybuf[c, :bound] for c in range(ns)]
    ms = pkg.MultiStream(fs, ys, xs)
    row("(c) filt_multi, one-channel filters" + part, fs[0].last_kernel_name, ms.run)
    for fc in fs:
        fc.close()
    # (d): the shared-taps filter with per-channel rates
    g = pkg.FIRFilter.per_channel_rates_farrow(H[0], rates, Nphi, POLYORDER)
    g.bind(np.float32, nch)
    row("(d) shared-taps per_channel_rates_farrow, default plan", g.last_kernel_name, lambda: g._filt_into_rates(ybuf, x, counts))
    g.close()
    med = {k: statistics.median(v) for k, v in rows.items()}
    med["c"] *= nch / ns                          # (one launch sequence per channel: scaled to all nch channels)
    spread = max(rows["a"]) - min(rows["a"]), max(rows["b"]) - min(rows["b"])
    best = min(med["a"], med["b"])
    emit(f"    (b) / (a): {med['b'] / med['a']:.3f}x, (b) - (a): {med['b'] - med['a']:.3f} ms (spread of the repeats: a {spread[0]:.3f} ms, b {spread[1]:.3f} ms); "
         f"(c) / best: {med['c'] / best:.2f}x; best / (d): {best / med['d']:.2f}x; the fit, (e) - (f): {med['e'] - med['f']:.3f} ms (best: the faster of (a), (b))")
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
