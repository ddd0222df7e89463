#!/usr/bin/env python3
"""Complex per-channel taps with per-channel rates for FIRArbitrary (FIRFilter.per_channel_complex_taps_and_rates,
mrhip_set_channel_ctaps / _device, csrc/kernels_rates_arb_ctaps.hip) against what a user did before, on one MI355X.

The three workloads of DESIGN.md 9 items 17, 18 and 21 with Complex64 taps (w1 ... w3: Float32 samples, Nphi 32, the rates spread
evenly over [2.0, 2.25], every channel with taps of its own) and the first one with ComplexF32 samples (w1c), each run these ways:
  (t) the new filter on the tiled kernel (MRHIP_ARB_RATES_CTAPS_TILED=1; reported as arb_rates_ctaps_tiled)
  (u) the new filter on the universal kernel (MRHIP_ARB_RATES_CTAPS_TILED=0; reported as arb_rates_ctaps_generic)
  (a) filt_multi over nch one-channel FIRFilter.complex_taps_arbitrary(H[c], rates[c], Nphi) filters: what a user does today
      (mrhip_filt_device_multi issues single calls for this kind).  Over the first BENCH_SINGLES_MAX = 256 channels only when nch is
      larger, the row says so; the time for all nch channels is then the row's figure times nch / 256, this way being one launch
      sequence per channel
  (b) real FIRFilter.per_channel_taps_and_rates filters over the real and the imaginary taps plus a combine pass: two filters for real
      samples, four for complex samples
  (c) the real-tap FIRFilter.per_channel_taps_and_rates filter of the same shape on its default plan: the floor
  (h) the new filter on its default plan with set_channel_ctaps(H) before every pass: an update through the host, its banks, the wait
      for the filter's stream and the upload included
  (d) the same with set_channel_ctaps_device(H_d): an update in stream order
Wall time of one pass over the whole signal, host clock around work that ends in a device synchronise; the clocks are settled as in
scripts/bench_arb_rates.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats per
row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).

    python scripts/bench_arb_rates_ctaps.py [w1 w1c w2 w3] [--out FILE]     the table
    python scripts/bench_arb_rates_ctaps.py --kernel-passes w1 [...]        the new filter only, on either kernel, settled + five
                                                                            passes each: the program to put behind
                                                                            `rocprofv3 --kernel-trace --stats --`
    python scripts/bench_arb_rates_ctaps.py --kernel-stats STATS.csv [--out FILE]     that run's kernel_stats.csv -> time per launch of
                                                                            the schedule kernel and of the two filter kernels
"""
import csv
import os
import statistics
import sys
import time

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels with MRHIP_ARB_RATES_CTAPS_TILED between calls)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "60"))
REPS = 5
SINGLES_MAX = int(os.environ.get("BENCH_SINGLES_MAX", "256"))
SWITCH = "MRHIP_ARB_RATES_CTAPS_TILED"
WORKLOADS = {
    "w1": ("4096 ch x 1e4 Float32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, 250 taps a channel", 4096, 10_000, 32, 250, np.float32),
    "w1c": ("4096 ch x 1e4 ComplexF32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, 250 taps a channel", 4096, 10_000, 32, 250, np.complex64),
    "w2": ("256 ch x 1e5 Float32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, 1024 taps a channel", 256, 100_000, 32, 1024, np.float32),
    "w3": ("64 ch x 1e6 Float32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, 1024 taps a channel", 64, 1_000_000, 32, 1024, np.float32),
}


def setup(key):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    title, nch, n, Nphi, ntaps, tx = WORKLOADS[key]
    rng = np.random.default_rng(7)
    H = ((rng.standard_normal((nch, ntaps)) + 1j * rng.standard_normal((nch, ntaps))) * Nphi / ntaps).astype(np.complex64)
    rates = np.linspace(2.0, 2.25, nch)
    x = torch.rand((nch, n), device=dev, dtype=torch.float32)
    if np.dtype(tx).kind == "c":
        x = torch.complex(x, torch.rand((nch, n), device=dev, dtype=torch.float32))
    return torch, pkg, dev, H, rates, x


def timed(one_pass, sync):
    """settle, then REPS timed passes: (times in ms, untimed passes)"""
    t0 = time.perf_counter()
    for i in range(20):
        one_pass()
        sync()
        el = (time.perf_counter() - t0) * 1e3
        if i >= 1 and el >= SETTLE_MS:
            break
    out = []
    for _ in range(REPS):
        sync()
        t = time.perf_counter()
        one_pass()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return out, i + 1


def workload(key, emit):
    torch, pkg, dev, H, rates, x = setup(key)
    title, nch, n, Nphi, ntaps, tx = WORKLOADS[key]
    cplx = np.dtype(tx).kind == "c"
    sync = torch.cuda.synchronize
    f = pkg.FIRFilter.per_channel_complex_taps_and_rates(H, rates, Nphi)
    f.bind(tx, nch)
    bound = f.outputlength_bound(n)
    ybuf = torch.empty((nch, bound), dtype=torch.complex64, device=dev)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    tiles_per_channel = -(-bound // 256)
    emit(f"## {key}: {title}")
    emit(f"    (bound {bound} outputs a channel: {tiles_per_channel} tiles a channel, {tiles_per_channel * nch} tiles; device banks {H.size * 2 * 8} bytes)")
    emit(f"{'way':<66}{'kernel':<28}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass, sync)
        rows[name[1]] = ts
        emit(f"{name:<66}{kernel():<28}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (t), (u): the new filter (nothing waits inside the call: the counts stay on the device)
    for name, mode in (("(t) new filter, tiled kernel", "1"), ("(u) new filter, universal kernel", "0")):
        os.environ[SWITCH] = mode
        row(name, f.last_kernel_name, lambda: f._filt_into_rates(ybuf, x, counts))
    os.environ.pop(SWITCH)
    f._filt_into_rates(ybuf, x, counts)
    default = "t" if f.last_kernel_name() == "arb_rates_ctaps_tiled" else "u"
    emit(f"    (default plan, {SWITCH} unset: {f.last_kernel_name()}; outputs of the last pass: {int(counts.sum())})")

    # (h), (d): an update before every pass, through the host and in stream order
    def host_update():
        f.set_channel_ctaps(H)
        f._filt_into_rates(ybuf, x, counts)
    row("(h) new filter, default plan, set_channel_ctaps each pass", f.last_kernel_name, host_update)
    H_d = torch.from_numpy(H).to(dev)

    def device_update():
        f.set_channel_ctaps_device(H_d)
        f._filt_into_rates(ybuf, x, counts)
    row("(d) new filter, default plan, set_channel_ctaps_device each pass", f.last_kernel_name, device_update)
    f.close()

    # (a): one-channel complex-tap filters, each with its own taps at its own rate
    ns = min(nch, SINGLES_MAX)
    part = "" if ns == nch else f", first {ns} ch only"
    fs = [pkg.FIRFilter.complex_taps_arbitrary(H[c], float(rates[c]), Nphi) for c in range(ns)]
    xs = [x[c] for c in range(ns)]
    for fc in fs:
        fc.bind(tx, 1)
    ys = [ybuf[c, :bound] for c in range(ns)]
    ms = pkg.MultiStream(fs, ys, xs)
    row("(a) filt_multi, one-channel complex-tap filters" + part, fs[0].last_kernel_name, ms.run)
    for fc in fs:
        fc.close()

    # (b): real bank filters over the real and the imaginary taps, and a combine pass
    Hr, Hi = np.ascontiguousarray(H.real), np.ascontiguousarray(H.imag)
    parts = [x.real.contiguous(), x.imag.contiguous()] if cplx else [x]
    reals = [(pkg.FIRFilter.per_channel_taps_and_rates(M, rates, Nphi), torch.empty((nch, bound), dtype=torch.float32, device=dev), p)
             for p in parts for M in (Hr, Hi)]                              # (Hr on xr, Hi on xr[, Hr on xi, Hi on xi])
    for g, _, _ in reals:
        g.bind(np.float32, nch)

    def real_filters():
        for g, y, p in reals:
            g._filt_into_rates(y, p, counts)
        if cplx:
            torch.complex(reals[0][1] - reals[3][1], reals[1][1] + reals[2][1], out=ybuf)
        else:
            torch.complex(reals[0][1], reals[1][1], out=ybuf)
    row(f"(b) {len(reals)} real per_channel_taps_and_rates filters + combine", reals[0][0].last_kernel_name, real_filters)
    for g, _, _ in reals[1:]:
        g.close()
    # (c): the real-tap bank filter of the same shape (real samples: the first of (b); complex samples: a filter of its own)
    g = reals[0][0]
    yfloor = reals[0][1]
    if cplx:
        g.close()
        g = pkg.FIRFilter.per_channel_taps_and_rates(Hr, rates, Nphi)
        g.bind(tx, nch)
        yfloor = ybuf
    row("(c) real-tap per_channel_taps_and_rates, default plan (floor)", g.last_kernel_name, lambda: g._filt_into_rates(yfloor, x, counts))
    g.close()

    med = {k: statistics.median(v) for k, v in rows.items()}
    med["a"] *= nch / ns                          # (one launch sequence per channel: scaled to all nch channels)
    spread = max(rows["t"]) - min(rows["t"]), max(rows["u"]) - min(rows["u"])
    best = min(med["t"], med["u"])
    emit(f"    (u) / (t): {med['u'] / med['t']:.3f}x (spread of the repeats: t {spread[0]:.3f} ms, u {spread[1]:.3f} ms); (a) / best: {med['a'] / best:.2f}x; "
         f"(b) / best: {med['b'] / best:.2f}x; best / (c): {best / med['c']:.2f}x; (h) - ({default}): {med['h'] - med[default]:.3f} ms; "
         f"(d) - ({default}): {med['d'] - med[default]:.3f} ms (best: the faster of (t), (u))")
    if ns != nch:
        emit(f"    ((a) in the ratios: the measured row times {nch}/{ns} = {med['a']:.1f} ms for all {nch} channels)")
    emit("")


def kernel_passes(key):
    """the new filter only, on either kernel: what a kernel trace of this row should see"""
    torch, pkg, dev, H, rates, x = setup(key)
    title, nch, n, Nphi, ntaps, tx = WORKLOADS[key]
    f = pkg.FIRFilter.per_channel_complex_taps_and_rates(H, rates, Nphi)
    f.bind(tx, nch)
    ybuf = torch.empty((nch, f.outputlength_bound(n)), dtype=torch.complex64, device=dev)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    for mode in ("1", "0"):
        os.environ[SWITCH] = mode
        ts, untimed = timed(lambda: f._filt_into_rates(ybuf, x, counts), torch.cuda.synchronize)
        print(f"{key}: {untimed} untimed + {REPS} timed passes on {f.last_kernel_name()}; wall median {statistics.median(ts):.3f} ms (under the profiler)", flush=True)
    f.close()


def kernel_stats(path, emit):
    """the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats -- ... --kernel-passes KEY` run (ONE key a run): the average time of
    a launch of the schedule kernel and of the two filter kernels, alone"""
    with open(path, newline="") as fh:
        stats = list(csv.DictReader(fh))
    for kernel in ("rates_schedule_kernel", "arb_rates_ctaps_tiled_kernel", "arb_rates_ctaps_generic_kernel"):
        mine = [r for r in stats if kernel in r["Name"]]
        if not mine:
            emit(f"    {kernel}: not in {os.path.basename(path)}")
            continue
        total_ns = sum(float(r["TotalDurationNs"]) for r in mine)
        calls = sum(int(r["Calls"]) for r in mine)
        emit(f"    {kernel}: {calls} launches, {total_ns / calls / 1e6:.3f} ms a launch (kernel trace)")


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
    if args and args[0] == "--kernel-passes":
        for key in args[1:]:
            kernel_passes(key)
    elif args and args[0] == "--kernel-stats":
        kernel_stats(args[1], emit)
    else:
        for key in args or list(WORKLOADS):
            workload(key, emit)


if __name__ == "__main__":
    main()
