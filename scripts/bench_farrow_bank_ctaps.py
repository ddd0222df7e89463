#!/usr/bin/env python3
"""Per-channel complex taps for FIRFarrow (FIRFilter.per_channel_complex_taps_farrow, csrc/kernels_bank_farrow_ctaps.hip) against what a
user did before, on one MI355X.

The seven workloads of DESIGN.md 9 item 16 (w1 ... w7; Nphi 32, polyorder 4), each run five ways:
  (b) the new filter (one kernel: farrow_bank_ctaps_generic_kernel)
  (c) filt_multi over nch one-channel FIRFilter.complex_taps_farrow filters (mrhip_filt_device_multi issues single calls for this kind)
  (d) the loop of nch single calls on one-channel filters
      ((c) and (d) over the first BENCH_SINGLES_MAX = 256 channels only when nch is larger, the row says so: every one-channel
      FIRFarrow filter holds its own schedule buffers; the time for all nch channels is then the row's figure times nch / 256, these
      ways being one launch sequence per channel)
  (e) two real bank filters, per_channel_farrow(real(H)) and per_channel_farrow(imag(H)), plus the torch combine pass (for complex
      samples: y = (yr.re - yi.im) + i (yr.im + yi.re); its roundings are not the reference's)
  (f) the shared-taps FIRFilter.complex_taps_farrow filter of the same shape, on whatever kernel the dispatcher picks: the floor
Wall time of one pass over the whole signal, host clock around work that ends in a device synchronise; the clocks are settled as in
scripts/bench_farrow_bank.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats
per row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).

The Float64 vector-ALU roof of a row is computed from its shape (f64_instructions): Float64 instructions per (channel, output, tap)
times their count, against the rate of separately rounded Float64 operations that scripts/bench_configs.py uses (39.3 T/s: half the
FMA peak -- nothing in this kernel may be fused).

    python scripts/bench_farrow_bank_ctaps.py [w1 ... w7] [--out FILE]       the table
    python scripts/bench_farrow_bank_ctaps.py --kernel-passes w1             the new filter only, settled + five passes: the program
                                                                             to put behind `rocprofv3 --kernel-trace --stats --`
    python scripts/bench_farrow_bank_ctaps.py --kernel-stats w1 STATS.csv    that run's kernel_stats.csv -> kernel time and roof share
"""
import csv
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "60"))
REPS = 5
SINGLES_MAX = int(os.environ.get("BENCH_SINGLES_MAX", "256"))
NPHI, POLYORDER = 32, 4
STRICT_F64_TOPS = 39.3                          # separately rounded Float64 operations, T/s (scripts/bench_configs.py)
KERNEL = "farrow_bank_ctaps_generic_kernel"
# title, channels, samples a channel, sample type, rate, taps, tap type
WORKLOADS = {
    "w1": ("64 ch x 1e6 Float32, rate 2.123, 1024 Complex64 taps", 64, 1_000_000, np.float32, 2.123, 1024, np.complex64),
    "w2": ("64 ch x 1e6 Float32, rate 0.47, 1024 Complex64 taps", 64, 1_000_000, np.float32, 0.47, 1024, np.complex64),
    "w3": ("64 ch x 1e6 ComplexF32, rate 2.123, 1024 Complex64 taps", 64, 1_000_000, np.complex64, 2.123, 1024, np.complex64),
    "w4": ("4096 ch x 1e4 ComplexF32, rate 2.123, 250 Complex64 taps", 4096, 10_000, np.complex64, 2.123, 250, np.complex64),
    "w5": ("64 ch x 1e4 ComplexF32, rate 2.123, 250 Complex64 taps", 64, 10_000, np.complex64, 2.123, 250, np.complex64),
    "w6": ("4 ch x 2e4 ComplexF32, rate 2.123, 250 Complex64 taps", 4, 20_000, np.complex64, 2.123, 250, np.complex64),
    "w7": ("config 4f's shape: 64 ch x 1e7 Float64, rate pi/3, 1024 Complex128 taps", 64, 10_000_000, np.float64, math.pi / 3, 1024, np.complex128),
}


def f64_instructions(nch, n_out, ntaps, tap, sample, polyorder=POLYORDER, Nphi=NPHI):
    """Float64 vector instructions (per lane) of one pass, from the shape: per (channel, output, tap)
         the two Horner chains: 2 components x polyorder x (one multiply + one add)
         the rounding to the tap's real scalar: 2 conversions Float64 -> Float32 for Complex64 taps (and 2 back when R is Float64)
         the dot, when R is Float64: real samples 2 multiplies + 2 adds, complex samples 4 multiplies + 2 add/sub + 2 adds
       (R = Float32: the dot is not Float64 work).  Returns (per tap, total)."""
    tap_f32 = np.dtype(tap) == np.complex64
    r_f64 = not tap_f32 or np.dtype(sample) in (np.dtype(np.float64), np.dtype(np.complex128))
    per = 2 * polyorder * 2 + (2 if tap_f32 else 0) + (2 if tap_f32 and r_f64 else 0)
    if r_f64:
        per += 8 if np.dtype(sample).kind == "c" else 4
    T = -(-ntaps // Nphi)
    return per, per * nch * n_out * T


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


def setup(key):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    title, nch, n, dt, rate, ntaps, th = WORKLOADS[key]
    rng = np.random.default_rng(7)
    H = ((rng.standard_normal((nch, ntaps)) + 1j * rng.standard_normal((nch, ntaps))) / ntaps).astype(th)
    real = torch.float64 if np.dtype(dt) in (np.dtype(np.float64), np.dtype(np.complex128)) else torch.float32
    x = torch.rand((nch, n), device=dev, dtype=real)
    if np.dtype(dt).kind == "c":
        x = torch.complex(x, torch.rand((nch, n), device=dev, dtype=real))
    return torch, pkg, dev, H, x


def workload(key, emit):
    torch, pkg, dev, H, x = setup(key)
    title, nch, n, dt, rate, ntaps, th = WORKLOADS[key]
    torch_of = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
                np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128}
    emit(f"## {key}: {title}")
    emit(f"{'way':<52}{'kernel':<34}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass, torch.cuda.synchronize)
        rows[name[1]] = ts
        emit(f"{name:<52}{kernel():<34}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (b): the new filter
    f = pkg.FIRFilter.per_channel_complex_taps_farrow(H, rate, NPHI, POLYORDER)
    f.bind(np.dtype(dt), nch)
    bound = f.outputlength_bound(n)
    n_out = f.outputlength(n)
    out_dtype = torch_of[np.dtype(f.output_dtype)]
    ybuf = torch.empty((nch, bound), dtype=out_dtype, device=dev)
    row("(b) new filter", f.last_kernel_name, lambda: f.filt_into(ybuf, x))
    f.close()
    # (c), (d): one-channel complex-tap filters
    ns = min(nch, SINGLES_MAX)
    part = "" if ns == nch else f", first {ns} ch only"
    fs = [pkg.FIRFilter.complex_taps_farrow(H[c], rate, NPHI, POLYORDER) for c in range(ns)]
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
    fr = pkg.FIRFilter.per_channel_farrow(np.ascontiguousarray(H.real), rate, NPHI, POLYORDER)
    fi = pkg.FIRFilter.per_channel_farrow(np.ascontiguousarray(H.imag), rate, NPHI, POLYORDER)
    fr.bind(np.dtype(dt), nch), fi.bind(np.dtype(dt), nch)
    part_dtype = torch_of[np.dtype(fr.output_dtype)]
    yr = torch.empty((nch, bound), dtype=part_dtype, device=dev)
    yi = torch.empty((nch, bound), dtype=part_dtype, device=dev)

    def two_real_banks():
        fr.filt_into(yr, x)
        fi.filt_into(yi, x)
        if not part_dtype.is_complex:
            torch.complex(yr, yi, out=ybuf)
        else:
            torch.complex(yr.real - yi.imag, yr.imag + yi.real, out=ybuf)
    row("(e) two real bank filters + combine", fr.last_kernel_name, two_real_banks)
    fr.close(), fi.close()
    del yr, yi
    # (f): the shared-taps filter
    g = pkg.FIRFilter.complex_taps_farrow(H[0], rate, NPHI, POLYORDER)
    row("(f) shared-taps filter (the floor)", g.last_kernel_name, lambda: g.filt_into(ybuf, x))
    g.close()
    med = {k: statistics.median(v) for k, v in rows.items()}
    for k in "cd":
        med[k] *= nch / ns                        # (one launch sequence per channel: scaled to all nch channels)
    spread = max(rows["b"]) - min(rows["b"])
    emit(f"    (c) / (b): {med['c'] / med['b']:.2f}x; (d) / (b): {med['d'] / med['b']:.2f}x; (e) / (b): {med['e'] / med['b']:.2f}x; "
         f"(b) / (f): {med['b'] / med['f']:.2f}x (spread of the repeats of (b): {spread:.3f} ms)")
    if ns != nch:
        emit(f"    ((c) and (d) in the ratios: the measured rows times {nch}/{ns} = {med['c']:.1f} and {med['d']:.1f} ms for all {nch} channels)")
    per, total = f64_instructions(nch, n_out, ntaps, th, dt)
    roof_ms = total / (STRICT_F64_TOPS * 1e12) * 1e3
    emit(f"    Float64 VALU roof: {per} Float64 instructions per (channel, output, tap) x {nch} x {n_out} x {-(-ntaps // NPHI)} = {total:.4g} "
         f"-> {roof_ms:.3f} ms at {STRICT_F64_TOPS} T/s; the wall time of (b) is {med['b'] / roof_ms:.2f}x that")
    emit("")


def kernel_passes(key):
    """the new filter only: what a kernel trace of this row should see"""
    torch, pkg, dev, H, x = setup(key)
    title, nch, n, dt, rate, ntaps, th = WORKLOADS[key]
    f = pkg.FIRFilter.per_channel_complex_taps_farrow(H, rate, NPHI, POLYORDER)
    f.bind(np.dtype(dt), nch)
    ybuf = torch.empty((nch, f.outputlength_bound(n)), dtype=torch.complex128 if np.dtype(f.output_dtype) == np.complex128 else torch.complex64, device=dev)
    ts, untimed = timed(lambda: f.filt_into(ybuf, x), torch.cuda.synchronize)
    print(f"{key}: {untimed} untimed + {REPS} timed passes on {f.last_kernel_name()}; wall median {statistics.median(ts):.3f} ms (under the profiler)", flush=True)
    f.close()


def kernel_stats(key, path, emit):
    """the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats -- ... --kernel-passes key` run -> time per pass and roof share
    (a pass of more than 2^24 outputs a channel is several launches: the total over the run divided by its passes)"""
    title, nch, n, dt, rate, ntaps, th = WORKLOADS[key]
    n_out = int(math.ceil(n * rate))                               # outputlength of a fresh stream (+- 1: immaterial here)
    with open(path, newline="") as fh:
        mine = [r for r in csv.DictReader(fh) if KERNEL in r["Name"]]
    assert mine, f"no {KERNEL} in {path}"
    total_ns = sum(float(r["TotalDurationNs"]) for r in mine)
    calls = sum(int(r["Calls"]) for r in mine)
    launches_per_pass = -(-n_out // (1 << 24))
    passes = calls / launches_per_pass
    ms = total_ns / passes / 1e6
    per, total = f64_instructions(nch, n_out, ntaps, th, dt)
    roof_ms = total / (STRICT_F64_TOPS * 1e12) * 1e3
    emit(f"{key}: {KERNEL}: {calls} launches = {passes:g} passes, {ms:.3f} ms a pass (kernel trace); Float64 VALU roof {roof_ms:.3f} ms "
         f"({per} instructions per (channel, output, tap)) -> {100 * roof_ms / ms:.1f} % of the separately rounded Float64 roof")


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
        kernel_stats(args[1], args[2], emit)
    else:
        for key in args or list(WORKLOADS):
            workload(key, emit)


if __name__ == "__main__":
    main()
