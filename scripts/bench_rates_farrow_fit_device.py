#!/usr/bin/env python3
"""The FIRFarrow fit on the device (mrhip_set_channel_taps_farrow_device, mrhip_set_channel_ctaps_farrow_device) against
the host calls it stands beside, on one MI355X.

Rows, the siblings' shapes (rates 2.0 ... 2.25, Nphi 32, polyorder 4, Float32 samples):
    4096 ch x 1e4, 250 taps a channel, Float32 taps        4096 ch x 1e4, 250 taps a channel, Complex64 taps
     256 ch x 1e5, 1024 taps a channel, Float32 taps         64 ch x 1e6, 1024 taps a channel, Float32 taps

Per row, ms per chunk (one tap update, then one mrhip_filt_device_rates of the shape, then a device synchronise; the taps live in a
device tensor, as a tracker leaves them):
    device fit   set_channel_taps_farrow_device (set_channel_ctaps_farrow_device)
    host fit     the taps brought to the host (.cpu()) and handed to set_channel_taps_farrow (set_channel_ctaps_farrow), as a user had to
    fitted banks set_channel_pnfb_device (set_channel_pnfb_ctaps_device) with banks fitted beforehand: the update without any fit
    no update    the chunk alone
and the new call alone, the stream idle: the wall of the host call (it returns without waiting) and the device time (an event pair).
Last, the filter whose bank is still shared, no update, at 4096 ch x 1e4: the row profiles/r17/rates_device_lengths.txt reports.

Method (as the siblings): sustained load first (passes of the filter until BENCH_SETTLE_MS of work), then REPS timed repeats per row,
each ending in a device synchronise; median, minimum and maximum are given, the spread is the last two.

    python scripts/bench_rates_farrow_fit_device.py [--out FILE]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda", 0)
SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "300"))
REPS = int(os.environ.get("BENCH_REPS", "9"))
NPHI, P = 32, 4
ROWS = [(4096, 10_000, 250, False), (4096, 10_000, 250, True), (256, 100_000, 1024, False), (64, 1_000_000, 1024, False)]


def settle(one_pass):
    t0 = time.perf_counter()
    for i in range(200):
        one_pass()
        torch.cuda.synchronize()
        if i >= 1 and (time.perf_counter() - t0) * 1e3 >= SETTLE_MS:
            break


def stats(ts):
    return f"{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}"


def timed(call, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def row(emit, nch, n, ntaps, cplx):
    rng = np.random.default_rng(7)
    H = (rng.standard_normal((nch, ntaps)) * NPHI / ntaps).astype(np.float32)
    if cplx:
        H = (H + 1j * (rng.standard_normal((nch, ntaps)) * NPHI / ntaps)).astype(np.complex64)
    rates = np.linspace(2.0, 2.25, nch)
    f = pkg.FIRFilter.per_channel_rates_farrow(np.ascontiguousarray(H[0].real), rates, NPHI, P).bind(np.float32, nch)
    host_fit = f.set_channel_ctaps_farrow if cplx else f.set_channel_taps_farrow
    device_fit = f.set_channel_ctaps_farrow_device if cplx else f.set_channel_taps_farrow_device
    banks = f.set_channel_pnfb_ctaps_device if cplx else f.set_channel_pnfb_device
    host_fit(H)
    PNd = torch.from_numpy(f.pnfb()).to(dev)                 # the banks, fitted beforehand
    Hd = torch.from_numpy(H).to(dev)
    x = torch.rand((nch, n), device=dev, dtype=torch.float32)
    y = torch.empty((nch, f.outputlength_bound(n)), dtype=torch.complex64 if cplx else torch.float32, device=dev)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    chunk = lambda: f._filt_into_rates(y, x, counts)
    name = f"{nch} ch x {n}, {ntaps} taps, {'Complex64' if cplx else 'Float32'} taps"
    emit(f"## {name}; ms")
    emit(f"{'way':<76}{'kernel':<28}{'median':>10}{'min':>9}{'max':>9}")
    settle(chunk)
    device_fit(Hd)                                           # (the first call: the table's upload, code object load)
    reps = REPS if n < 1_000_000 else max(REPS // 2, 3)
    ways = (("chunk, device fit (the new call)", lambda: (device_fit(Hd), chunk())),
            ("chunk, host fit (taps to the host, the host call)", lambda: (host_fit(Hd.cpu().numpy()), chunk())),
            ("chunk, fitted banks (set_channel_pnfb*_device, no fit)", lambda: (banks(PNd), chunk())),
            ("chunk, no update", chunk))
    med = {}
    for way, call in ways:
        settle(chunk)
        ts = timed(call, reps)
        med[way] = statistics.median(ts)
        emit(f"{way:<76}{f.last_kernel_name():<28}{stats(ts)}")
    walls, devs = [], []
    for _ in range(REPS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t = time.perf_counter()
        device_fit(Hd)
        walls.append((time.perf_counter() - t) * 1e3)
        e1.record()
        torch.cuda.synchronize()
        devs.append(e0.elapsed_time(e1))
    emit(f"{'the new call alone: host call, wall (no wait)':<76}{'-':<28}{stats(walls)}")
    emit(f"{'the new call alone: device, event pair':<76}{'-':<28}{stats(devs)}")
    a, b, d = med["chunk, device fit (the new call)"], med["chunk, host fit (taps to the host, the host call)"], med["chunk, no update"]
    emit(f"device fit against host fit: {a:.3f} against {b:.3f} ms ({b / a:.2f}x); surplus over the chunk without an update: {a - d:+.3f} ms")
    emit("")
    f.close()


def shared_bank(emit):
    nch, n, ntaps = 4096, 10_000, 250
    rng = np.random.default_rng(7)
    h = (rng.standard_normal(ntaps) * NPHI / ntaps).astype(np.float32)
    f = pkg.FIRFilter.per_channel_rates_farrow(h, np.linspace(2.0, 2.25, nch), NPHI, P).bind(np.float32, nch)
    x = torch.rand((nch, n), device=dev, dtype=torch.float32)
    y = torch.empty((nch, f.outputlength_bound(n)), dtype=torch.float32, device=dev)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    chunk = lambda: f._filt_into_rates(y, x, counts)
    emit(f"## the existing call, the bank still shared: mrhip_filt_device_rates, {nch} ch x {n}; ms")
    settle(chunk)
    emit(f"{'farrow mrhip_filt_device_rates, no update':<76}{f.last_kernel_name():<28}{stats(timed(chunk))}")
    emit("")
    f.close()


def main():
    args = sys.argv[1:]
    out = open(args[args.index("--out") + 1], "a") if "--out" in args else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    emit(f"# library: {os.path.basename(pkg.library_path())}; REPS {REPS}, settle {SETTLE_MS:.0f} ms")
    for r in ROWS:
        row(emit, *r)
    shared_bank(emit)


if __name__ == "__main__":
    main()
