#!/usr/bin/env python3
"""Per-channel input lengths for the filters with per-channel rates (mrhip_filt_device_rates_ragged; FIRFilter.filt_into with
``lengths``) on one MI355X: the measurements of DESIGN.md 9 item 20.

    python scripts/bench_rates_ragged.py old [--root DIR]     the workloads w1 ... w3 of items 17 and 18 through mrhip_filt_device_rates,
                                                              both families, (a) the tiled / multi kernel and (b) the universal one.
                                                              --root DIR: the package and library of another checkout (the parent
                                                              commit's, for the alternation parent, new, parent, new: a fresh process each)
    python scripts/bench_rates_ragged.py equal                the same rows through the new entry point with equal lengths, beside the
                                                              old one on the same library
    python scripts/bench_rates_ragged.py ragged               4096 ch, lengths drawn once (seed 7) uniformly from 9000 ... 10000, Float32,
                                                              250 taps, rates 2.0 ... 2.25, both families: the ragged call against
                                                              filt_multi over one-channel filters fed their own lengths (the first
                                                              256 channels, scaled by 16, as items 12 to 18 do)
    ... [--out FILE]

Wall time of one pass, host clock around work that ends in a device synchronise; the clocks are settled as in
scripts/bench_arb_rates.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats per
row: median, minimum and maximum.  The streams continue from pass to pass (no reset)."""
import importlib.util
import os
import statistics
import sys
import time

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels between calls)
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
SINGLES_MAX = 256
POLYORDER = 4
WORKLOADS = {
    "w1": ("4096 ch x 1e4, 250 taps", 4096, 10_000, 250),
    "w2": ("256 ch x 1e5, 1024 taps", 256, 100_000, 1024),
    "w3": ("64 ch x 1e6, 1024 taps", 64, 1_000_000, 1024),
}
FAMILIES = {"arbitrary": "MRHIP_ARB_RATES_TILED", "farrow": "MRHIP_FARROW_RATES_MULTI"}


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


def make(family, h, rates, one_channel=None):
    if one_channel is None:
        f = pkg.FIRFilter.per_channel_rates(h, rates, 32) if family == "arbitrary" else pkg.FIRFilter.per_channel_rates_farrow(h, rates, 32, POLYORDER)
        return f.bind(np.float32, len(rates))
    r = float(rates[one_channel])
    return (pkg.FIRFilter(h, r, 32) if family == "arbitrary" else pkg.FIRFilter(h, r, 32, POLYORDER)).bind(np.float32, 1)


def signal(nch, n, ntaps):
    rng = np.random.default_rng(7)
    h = (rng.standard_normal(ntaps) * 32 / ntaps).astype(np.float32)
    return h, np.linspace(2.0, 2.25, nch), torch.rand((nch, n), device=dev, dtype=torch.float32)


def line(emit, name, kernel, ts):
    emit(f"{name:<64}{kernel:<24}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}")


def rows(emit, entry_points):
    emit(f"{'row':<64}{'kernel':<24}{'median ms':>10}{'min':>9}{'max':>9}")
    for key, (title, nch, n, ntaps) in WORKLOADS.items():
        h, rates, x = signal(nch, n, ntaps)
        lens = np.full(nch, n, dtype=np.int64)
        for family, switch in FAMILIES.items():
            f = make(family, h, rates)
            ybuf = torch.empty((nch, f.outputlength_bound(n)), dtype=torch.float32, device=dev)
            counts = torch.zeros(nch, dtype=torch.int64, device=dev)
            for way, mode in (("(a)", "1"), ("(b)", "0")):
                os.environ[switch] = mode
                for ep in entry_points:
                    one = (lambda: f._filt_into_rates(ybuf, x, counts)) if ep == "old" else (lambda: f._filt_into_rates(ybuf, x, counts, lengths=lens))
                    ts = timed(one)
                    line(emit, f"{key} {family} {way} {title}, {ep} entry point", f.last_kernel_name(), ts)
            os.environ.pop(switch)
            f.close()
            del ybuf
        del x
        torch.cuda.empty_cache()


def ragged(emit):
    nch, ntaps = 4096, 250
    h, rates, x = signal(nch, 10_000, ntaps)
    lens = np.random.default_rng(7).integers(9000, 10001, nch).astype(np.int64)
    emit(f"## ragged: {nch} ch, lengths uniform in 9000 ... 10000 (seed 7; min {lens.min()}, mean {lens.mean():.1f}, max {lens.max()}), Float32, {ntaps} taps")
    emit(f"{'row':<64}{'kernel':<24}{'median ms':>10}{'min':>9}{'max':>9}")
    for family, switch in FAMILIES.items():
        f = make(family, h, rates)
        ybuf = torch.empty((nch, f.outputlength_bound(int(lens.max()))), dtype=torch.float32, device=dev)
        counts = torch.zeros(nch, dtype=torch.int64, device=dev)
        med = {}
        for way, mode in (("(a)", "1"), ("(b)", "0")):
            os.environ[switch] = mode
            ts = timed(lambda: f._filt_into_rates(ybuf, x, counts, lengths=lens))
            med[way] = statistics.median(ts)
            line(emit, f"{family} {way} ragged call", f.last_kernel_name(), ts)
        os.environ.pop(switch)
        f._filt_into_rates(ybuf, x, counts, lengths=lens)
        torch.cuda.synchronize()
        emit(f"    (default plan: {f.last_kernel_name()}; outputs of the last pass: {int(counts.sum())})")
        f.close()
        ns = SINGLES_MAX
        fs = [make(family, h, rates, c) for c in range(ns)]
        ms = pkg.MultiStream(fs, [ybuf[c] for c in range(ns)], [x[c, :int(lens[c])] for c in range(ns)])
        ts = timed(ms.run)
        line(emit, f"{family} (c) filt_multi, one-channel filters, first {ns} ch, own lengths", fs[0].last_kernel_name(), ts)
        scaled = statistics.median(ts) * nch / ns
        emit(f"    (c) scaled by {nch // ns} to all {nch} channels: {scaled:.1f} ms; (c) / best ragged: {scaled / min(med.values()):.1f}x")
        for fc in fs:
            fc.close()
        del ybuf


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
    mode = args[0] if args else "ragged"
    if mode == "old":
        emit(f"## old entry point, package of {os.path.basename(ROOT) or ROOT}")
        rows(emit, ["old"])
    elif mode == "equal":
        emit("## equal lengths through the new entry point beside the old one, the same library")
        rows(emit, ["old", "ragged"])
    elif mode == "ragged":
        ragged(emit)
    else:
        sys.exit(f"unknown mode {mode}")


if __name__ == "__main__":
    main()
