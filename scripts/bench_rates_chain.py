#!/usr/bin/env python3
"""Input lengths from device memory, and chaining, for the filters with per-channel rates (mrhip_filt_device_rates_lens_device,
mrhip_filt_device_rates_chained; FIRFilter.filt_rates_async) on one MI355X: the measurements of DESIGN.md 9 item 27.

    python scripts/bench_rates_chain.py old [--root DIR]     the EXISTING calls, both families, default plans: mrhip_filt_device_rates on
                                                             4096 ch x 1e4 and mrhip_filt_device_rates_ragged on 4096 ch with lengths
                                                             9000 ... 10000.  --root DIR: the package and library of another checkout
                                                             (the parent commit's, for the alternation parent, new, parent, new: a
                                                             fresh process each)
    python scripts/bench_rates_chain.py lengths              4096 ch, lengths drawn once (seed 7) uniformly from 9000 ... 10000, Float32,
                                                             250 taps, rates 2.0 ... 2.25, both families:
                                                               (a) the host ragged call (the lengths in a host array)
                                                               (b) the device-length call (the lengths already in a CUDA tensor)
                                                               (c) the loop "lengths computed on the GPU -> filter" through (b)
                                                               (d) the same loop as a user writes it without (b): the lengths copied to
                                                                   the host, waited for, then (a)
                                                               (e) the import alone: (b) over max_length 0 (the import kernel, an
                                                                   all-empty walk and no filter kernel) -- an upper bound of its cost
    python scripts/bench_rates_chain.py chain                4096 ch x 1e4 into stage 1 (rates 2.0 ... 2.25, ragged lengths as above), its
                                                             outputs into stage 2 (rates 0.4 ... 0.5, 100 taps), both with per-channel
                                                             rates, both families as stage 2 behind a FIRArbitrary stage 1:
                                                               (a) mrhip_filt_device_rates_chained: no host round trip
                                                               (b) stage 1's counts read on the host (a wait), then the host ragged call
    ... [--out FILE]

Wall time of one pass, host clock around work that ends in a device synchronise; the clocks are settled as in
scripts/bench_rates_ragged.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats
per row: median, minimum and maximum.  The streams continue from pass to pass (no reset)."""
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
if "--root" in args:
    i = args.index("--root")
    ROOT = os.path.abspath(args[i + 1])
    del args[i:i + 2]
import numpy as np
import torch

spec = importlib.util.spec_from_file_location("graft_entry_of_root", os.path.join(ROOT, "__graft_entry__.py"))
ge = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ge)
pkg = ge.load_package()
dev = torch.device("cuda", 0)
SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "60"))
REPS = 5
POLYORDER = 4
NCH, N, NTAPS = 4096, 10_000, 250
FAMILIES = ("arbitrary", "farrow")


def timed(one_pass):
    t0 = time.perf_counter()
    for i in range(20):
        one_pass()
        torch.cuda.synchronize()
        if i >= 1 and (time.perf_counter() - t0) * 1e3 >= SETTLE_MS:
            break
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        one_pass()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def make(family, h, rates):
    f = pkg.FIRFilter.per_channel_rates(h, rates, 32) if family == "arbitrary" else pkg.FIRFilter.per_channel_rates_farrow(h, rates, 32, POLYORDER)
    return f.bind(np.float32, len(rates))


def signal(ntaps=NTAPS, lo=2.0, hi=2.25):
    rng = np.random.default_rng(7)
    h = (rng.standard_normal(ntaps) * 32 / ntaps).astype(np.float32)
    return h, np.linspace(lo, hi, NCH)


def drawn_lengths():
    return np.random.default_rng(7).integers(9000, 10001, NCH).astype(np.int64)


def line(emit, name, kernel, ts):
    emit(f"{name:<72}{kernel:<24}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}")


def head(emit):
    emit(f"{'row':<72}{'kernel':<24}{'median ms':>10}{'min':>9}{'max':>9}")


def old(emit):
    h, rates = signal()
    x = torch.rand((NCH, N), device=dev, dtype=torch.float32)
    lens = drawn_lengths()
    head(emit)
    for family in FAMILIES:
        f = make(family, h, rates)
        ybuf = torch.empty((NCH, f.outputlength_bound(N)), dtype=torch.float32, device=dev)
        counts = torch.zeros(NCH, dtype=torch.int64, device=dev)
        ts = timed(lambda: f._filt_into_rates(ybuf, x, counts))
        line(emit, f"{family} mrhip_filt_device_rates, {NCH} ch x {N}", f.last_kernel_name(), ts)
        ts = timed(lambda: f._filt_into_rates(ybuf, x, counts, lengths=lens))
        line(emit, f"{family} mrhip_filt_device_rates_ragged, lengths 9000 ... 10000", f.last_kernel_name(), ts)
        f.close()
        del ybuf


def lengths(emit):
    h, rates = signal()
    x = torch.rand((NCH, N), device=dev, dtype=torch.float32)
    lens = drawn_lengths()
    emit(f"## lengths: {NCH} ch, uniform in 9000 ... 10000 (seed 7; min {lens.min()}, mean {lens.mean():.1f}, max {lens.max()}), Float32, {NTAPS} taps")
    head(emit)
    base = torch.from_numpy(lens + 5).to(dev)
    lens_dev = torch.from_numpy(lens).to(dev)
    made = torch.empty(NCH, dtype=torch.int64, device=dev)
    zeros = torch.zeros(NCH, dtype=torch.int64, device=dev)
    for family in FAMILIES:
        f = make(family, h, rates)
        ybuf = torch.empty((NCH, f.outputlength_bound(N)), dtype=torch.float32, device=dev)
        counts = torch.zeros(NCH, dtype=torch.int64, device=dev)
        ts = timed(lambda: f._filt_into_rates(ybuf, x, counts, lengths=lens))
        line(emit, f"{family} (a) host ragged call", f.last_kernel_name(), ts)
        a = statistics.median(ts)
        ts = timed(lambda: f.filt_rates_async(ybuf, x, lengths=lens_dev, max_length=N, counts=counts))
        line(emit, f"{family} (b) device-length call", f.last_kernel_name(), ts)
        b = statistics.median(ts)

        def loop_new():
            torch.sub(base, 5, out=made)                                     # the lengths: computed on the GPU
            f.filt_rates_async(ybuf, x, lengths=made, max_length=N, counts=counts)

        def loop_today():
            torch.sub(base, 5, out=made)
            on_host = made.cpu().numpy()                                     # a copy and a wait
            f._filt_into_rates(ybuf, x, counts, lengths=on_host)

        ts = timed(loop_new)
        line(emit, f"{family} (c) lengths computed on the GPU -> device-length call", f.last_kernel_name(), ts)
        c = statistics.median(ts)
        ts = timed(loop_today)
        line(emit, f"{family} (d) lengths computed on the GPU -> host, wait -> ragged call", f.last_kernel_name(), ts)
        d = statistics.median(ts)
        outputs = int(counts.sum())
        ts = timed(lambda: f.filt_rates_async(ybuf, x, lengths=zeros, max_length=0, counts=counts))
        line(emit, f"{family} (e) the import, an all-empty walk, no filter kernel", "-", ts)
        emit(f"    (b) - (a): {b - a:+.3f} ms; (c) - (d): {c - d:+.3f} ms; outputs of the last full pass: {outputs}")
        f.close()
        del ybuf


def chain(emit):
    h1, r1 = signal()
    h2, r2 = signal(100, 0.4, 0.5)
    x = torch.rand((NCH, N), device=dev, dtype=torch.float32)
    lens = drawn_lengths()
    emit(f"## chain: {NCH} ch x {N} (lengths 9000 ... 10000) -> FIRArbitrary rates 2.0 ... 2.25, {NTAPS} taps -> stage 2, rates 0.4 ... 0.5, 100 taps")
    head(emit)
    f1 = make("arbitrary", h1, r1)
    b1 = f1.outputlength_bound(N)
    y1 = torch.empty((NCH, b1), dtype=torch.float32, device=dev)
    c1 = torch.zeros(NCH, dtype=torch.int64, device=dev)
    ts = timed(lambda: f1._filt_into_rates(y1, x, c1, lengths=lens))
    line(emit, "stage 1 alone (host ragged call)", f1.last_kernel_name(), ts)
    for family in FAMILIES:
        f2 = make(family, h2, r2)
        y2 = torch.empty((NCH, f2.outputlength_bound(b1)), dtype=torch.float32, device=dev)
        c2 = torch.zeros(NCH, dtype=torch.int64, device=dev)

        def chained():
            f1._filt_into_rates(y1, x, c1, lengths=lens)
            f2.filt_rates_async(y2, y1, after=f1, max_length=b1, counts=c2)

        def through_the_host():
            f1._filt_into_rates(y1, x, c1, lengths=lens)
            on_host = c1.cpu().numpy()                                       # stage 1's counts: a copy and a wait
            f2._filt_into_rates(y2, y1, c2, lengths=on_host)

        ts = timed(chained)
        line(emit, f"stage 2 {family} (a) mrhip_filt_device_rates_chained", f2.last_kernel_name(), ts)
        a = statistics.median(ts)
        n_a = int(c2.sum())
        ts = timed(through_the_host)
        line(emit, f"stage 2 {family} (b) counts read on the host, then the ragged call", f2.last_kernel_name(), ts)
        emit(f"    (a) - (b): {a - statistics.median(ts):+.3f} ms; stage 2 outputs of the last pass: {n_a} (a), {int(c2.sum())} (b)")
        f2.close()
        del y2
    f1.close()


def main():
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = open(args[i + 1], "a")
        del args[i:i + 2]

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
    mode = args[0] if args else "lengths"
    if mode == "old":
        emit(f"## the existing calls, package of {os.path.basename(ROOT) or ROOT}")
        old(emit)
    elif mode == "lengths":
        lengths(emit)
    elif mode == "chain":
        chain(emit)
    else:
        sys.exit(f"unknown mode {mode}")


if __name__ == "__main__":
    main()
