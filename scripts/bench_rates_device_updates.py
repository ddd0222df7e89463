#!/usr/bin/env python3
"""Device-resident, stream-ordered updates of the filters with per-channel rates (mrhip_set_channel_rates_device,
mrhip_set_channel_taps_device, mrhip_set_channel_pnfb_device) against the host calls they stand beside, on one MI355X.

Shape: the row every sibling reports -- 4096 ch x 1e4 Float32, rates 2.0 ... 2.25, 250 taps a channel, Nphi 32 (FIRFarrow: polyorder 4).

  calls     per call: the device time of each of the three device calls (an event pair around the call on an idle stream) and the wall
            of the host call itself (it returns without waiting); next to them the wall of the host call it stands beside
            (set_channel_rates, set_channel_taps, set_channel_pnfb: complete on return), the stream idle
  loop      per chunk: 100 chunks of the shape, a rate AND a tap update before every chunk, the values computed by torch on the device
            (the tracker's stand-in).  Device way: the two device calls, nothing read back; host way: the values are brought to the host
            (.cpu()) and handed to the host calls, as a user had to; and the same loop without any update (the floor)
  existing  mrhip_filt_device_rates of the shape on the four filters (FIRArbitrary / FIRFarrow, shared / per-channel taps), default plans

--parent: the library is one built from the parent commit (MRHIP_LIB_PATH points at it): the rows of the device calls are left out and
the three new symbols are not bound.  Run the sections on both libraries in the same session, alternating, and compare.

Method (as the siblings): sustained load first (passes of the filter until BENCH_SETTLE_MS of work), then REPS timed repeats per row,
each ending in a device synchronise where it measures device work; median, minimum and maximum are given, the spread is the last two.

    python scripts/bench_rates_device_updates.py [calls loop existing] [--parent] [--out FILE]
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

PARENT = "--parent" in sys.argv
pkg = ge.load_package()
NEW = ("mrhip_set_channel_rates_device", "mrhip_set_channel_taps_device", "mrhip_set_channel_pnfb_device")
if PARENT:
    pkg.host.ABI[:] = [row for row in pkg.host.ABI if row[0] not in NEW]
dev = torch.device("cuda", 0)
SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "300"))
REPS = int(os.environ.get("BENCH_REPS", "9"))
NCH, N, NPHI, NTAPS, P = 4096, 10_000, 32, 250, 4
CHUNKS = 100
LO, HI = 1.9, 2.4


def settle(one_pass):
    t0 = time.perf_counter()
    for i in range(200):
        one_pass()
        torch.cuda.synchronize()
        if i >= 1 and (time.perf_counter() - t0) * 1e3 >= SETTLE_MS:
            break


def stats(ts):
    return f"{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}"


def filters(which):
    rng = np.random.default_rng(7)
    H = (rng.standard_normal((NCH, NTAPS)) * NPHI / NTAPS).astype(np.float32)
    rates = np.linspace(2.0, 2.25, NCH)
    F = pkg.FIRFilter
    T = -(-NTAPS // NPHI)
    PN = rng.standard_normal((NCH, T, P + 1)) / T
    made = {}
    if "arb" in which:
        made["arb"] = F.per_channel_rates(H[0], rates, NPHI).bind(np.float32, NCH)
    if "arb_bank" in which:
        made["arb_bank"] = F.per_channel_taps_and_rates(H, rates, NPHI).bind(np.float32, NCH)
    if "farrow" in which:
        made["farrow"] = F.per_channel_rates_farrow(H[0], rates, NPHI, P).bind(np.float32, NCH)
    if "farrow_bank" in which:
        g = F.per_channel_rates_farrow(H[0], rates, NPHI, P).bind(np.float32, NCH)
        g.set_channel_pnfb(PN)
        made["farrow_bank"] = g
    return H, rates, PN, made


def buffers(f, hi=None):
    x = torch.rand((NCH, N), device=dev, dtype=torch.float32)
    bound = f.outputlength_bound(N) if hi is None else int(np.ceil(N * hi)) + 2
    return x, torch.empty((NCH, bound), dtype=torch.float32, device=dev), torch.zeros(NCH, dtype=torch.int64, device=dev)


def section_calls(emit):
    H, rates, PN, made = filters(("arb_bank", "farrow_bank"))
    f, g = made["arb_bank"], made["farrow_bank"]
    x, ybuf, counts = buffers(f, HI)
    Hd, rd, PNd = torch.from_numpy(H).to(dev), torch.from_numpy(rates).to(dev), torch.from_numpy(PN).to(dev)
    emit(f"## per call, {NCH} ch, {NTAPS} taps a channel, Nphi {NPHI} (FIRFarrow: polyorder {P}); ms")
    emit(f"{'call':<44}{'what':<28}{'median':>10}{'min':>9}{'max':>9}")
    settle(lambda: f._filt_into_rates(ybuf, x, counts))

    def host_row(name, call):
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t) * 1e3)
        emit(f"{name:<44}{'host call, wall':<28}{stats(ts)}")

    def device_row(name, call):
        call()                                             # (the first call: code object load)
        walls, devs = [], []
        for _ in range(REPS):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t = time.perf_counter()
            call()
            walls.append((time.perf_counter() - t) * 1e3)
            e1.record()
            torch.cuda.synchronize()
            devs.append(e0.elapsed_time(e1))
        emit(f"{name:<44}{'host call, wall (no wait)':<28}{stats(walls)}")
        emit(f"{name:<44}{'device, event pair':<28}{stats(devs)}")

    host_row("set_channel_rates", lambda: f.set_channel_rates(rates))
    host_row("set_channel_taps", lambda: f.set_channel_taps(H))
    host_row("set_channel_pnfb", lambda: g.set_channel_pnfb(PN))
    if not PARENT:
        device_row("set_channel_rates_device", lambda: f.set_channel_rates_device(rd, LO, HI))
        device_row("set_channel_taps_device", lambda: f.set_channel_taps_device(Hd))
        device_row("set_channel_pnfb_device", lambda: g.set_channel_pnfb_device(PNd))
    emit("")
    f.close(), g.close()


def section_loop(emit):
    H, rates, PN, made = filters(("arb_bank",))
    f = made["arb_bank"]
    x, ybuf, counts = buffers(f, HI)
    baseH, baser = torch.from_numpy(H).to(dev), torch.from_numpy(rates).to(dev)
    Hd, rd = baseH.clone(), baser.clone()
    emit(f"## per chunk: {CHUNKS} chunks of {NCH} ch x {N} Float32, a rate and a tap update before every chunk; ms per chunk")
    emit(f"{'way':<72}{'median':>10}{'min':>9}{'max':>9}")

    def tracker(i):                                         # the values of chunk i, computed on the device
        torch.mul(baseH, 1.0 + 1e-6 * (i % 7), out=Hd)
        torch.mul(baser, 1.0 + 1e-6 * (i % 5), out=rd)

    def device_way():
        for i in range(CHUNKS):
            tracker(i)
            f.set_channel_rates_device(rd, LO, HI)
            f.set_channel_taps_device(Hd)
            f._filt_into_rates(ybuf, x, counts)

    def host_way():
        for i in range(CHUNKS):
            tracker(i)
            f.set_channel_rates(rd.cpu().numpy())
            f.set_channel_taps(Hd.cpu().numpy())
            f._filt_into_rates(ybuf, x, counts)

    def floor():
        for i in range(CHUNKS):
            tracker(i)
            f._filt_into_rates(ybuf, x, counts)

    def row(name, way):
        way()
        ts = []
        for _ in range(max(REPS // 3, 3)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            way()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3 / CHUNKS)
        emit(f"{name:<72}{stats(ts)}")

    settle(lambda: f._filt_into_rates(ybuf, x, counts))
    row("no update (the floor)", floor)
    row("host calls (values to the host, set_channel_rates, set_channel_taps)", host_way)
    if not PARENT:
        row("device calls (set_channel_rates_device, set_channel_taps_device)", device_way)
    emit("")
    f.close()


def section_existing(emit):
    H, rates, PN, made = filters(("arb", "arb_bank", "farrow", "farrow_bank"))
    x, ybuf, counts = buffers(made["arb"])
    emit(f"## mrhip_filt_device_rates, {NCH} ch x {N} Float32, default plans; ms per call")
    emit(f"{'filter':<44}{'kernel':<28}{'median':>10}{'min':>9}{'max':>9}")
    settle(lambda: made["arb"]._filt_into_rates(ybuf, x, counts))
    for name, f in made.items():
        settle(lambda: f._filt_into_rates(ybuf, x, counts))
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f._filt_into_rates(ybuf, x, counts)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        emit(f"{name:<44}{f.last_kernel_name():<28}{stats(ts)}")
        f.close()
    emit("")


def main():
    args = [a for a in sys.argv[1:] if a != "--parent"]
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
    emit(f"# library: {'PARENT commit' if PARENT else 'this commit'} ({os.path.basename(pkg.library_path())})")
    sections = {"calls": section_calls, "loop": section_loop, "existing": section_existing}
    for key in args or list(sections):
        sections[key](emit)


if __name__ == "__main__":
    main()
