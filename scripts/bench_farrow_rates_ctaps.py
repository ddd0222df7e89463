#!/usr/bin/env python3
"""Complex per-channel taps with per-channel rates for FIRFarrow (FIRFilter.per_channel_complex_taps_and_rates_farrow,
mrhip_set_channel_ctaps_farrow / mrhip_set_channel_pnfb_ctaps / _device, csrc/kernels_rates_farrow_ctaps.hip) against what a user did
before, on one MI355X.

The three workloads of DESIGN.md 9 items 18 and 22 with Complex64 taps (w1 ... w3: Nphi 32, polyorder 4, the rates spread evenly over
[2.0, 2.25], every channel with a bank of its own), each with Float32 samples and (w1c ... w3c) with ComplexF32 samples, run these ways:
  (m) the new filter on the multi kernel (MRHIP_FARROW_RATES_CTAPS_MULTI=1; reported as farrow_rates_ctaps_multi)
  (u) the new filter on the universal kernel (MRHIP_FARROW_RATES_CTAPS_MULTI=0; reported as farrow_rates_ctaps_generic)
  (a) filt_multi over nch one-channel FIRFilter.complex_taps_farrow(..., pnfb = PN[c]) filters: what a user does today
      (mrhip_filt_device_multi issues single calls for this kind).  Over the first BENCH_SINGLES_MAX = 256 channels only when nch is
      larger, the row says so; the time for all nch channels is then the row's figure times nch / 256, this way being one launch
      sequence per channel
  (b) real FIRFilter.per_channel_taps_and_rates_farrow filters over the real and the imaginary banks plus a combine pass: two filters
      for real samples, four for complex samples
  (c) the real-tap FIRFilter.per_channel_taps_and_rates_farrow filter of the same shape on its default plan: the floor
  (h) the new filter on its default plan with set_channel_ctaps_farrow(H) before every pass: the fit of every row on the host, the wait
      for the filter's stream and the upload included
  (p) the same with set_channel_pnfb_ctaps(PN): fitted banks through the host
  (d) the same with set_channel_pnfb_ctaps_device(PN_d): an update in stream order
Wall time of one pass over the whole signal, host clock around work that ends in a device synchronise; the clocks are settled as in
scripts/bench_arb_rates.py (at least 2 untimed passes, then on until BENCH_SETTLE_MS of work or 20 passes), then five timed repeats per
row: the table gives their median, minimum and maximum.  The streams continue from pass to pass (no reset).  The banks are random
coefficients (no fit: the kernels' time does not depend on the values); (h) fits random taps.

    python scripts/bench_farrow_rates_ctaps.py [w1 w1c w2 w2c w3 w3c] [--out FILE]     the table
    python scripts/bench_farrow_rates_ctaps.py --kernels w1 [...] [--out FILE]         rows (m) and (u) only (a library built with another
                                                                                       kFarrowRatesCtapsOPL: MRHIP_LIB_PATH)
    python scripts/bench_farrow_rates_ctaps.py --siblings [--out FILE]                 the five older per-channel-rate filters at 4096 ch x
                                                                                       1e4 on their default plans, five timed repeats: run
                                                                                       once per library (MRHIP_LIB_PATH) to compare two
                                                                                       builds; symbols a library lacks are left unbound
"""
import ctypes
import os
import statistics
import sys
import time

os.environ["MRHIP_ENV_DYNAMIC"] = "1"          # (the rows switch kernels with MRHIP_FARROW_RATES_CTAPS_MULTI between calls)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SETTLE_MS = float(os.environ.get("BENCH_SETTLE_MS", "60"))
REPS = 5
SINGLES_MAX = int(os.environ.get("BENCH_SINGLES_MAX", "256"))
SWITCH = "MRHIP_FARROW_RATES_CTAPS_MULTI"
P = 4
WORKLOADS = {
    "w1": ("4096 ch x 1e4 Float32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, polyorder 4, 250 taps a channel", 4096, 10_000, 32, 250, np.float32),
    "w1c": ("4096 ch x 1e4 ComplexF32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, polyorder 4, 250 taps a channel", 4096, 10_000, 32, 250, np.complex64),
    "w2": ("256 ch x 1e5 Float32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, polyorder 4, 1024 taps a channel", 256, 100_000, 32, 1024, np.float32),
    "w2c": ("256 ch x 1e5 ComplexF32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, polyorder 4, 1024 taps a channel", 256, 100_000, 32, 1024, np.complex64),
    "w3": ("64 ch x 1e6 Float32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, polyorder 4, 1024 taps a channel", 64, 1_000_000, 32, 1024, np.float32),
    "w3c": ("64 ch x 1e6 ComplexF32, Complex64 taps, rates 2.0 ... 2.25, Nphi 32, polyorder 4, 1024 taps a channel", 64, 1_000_000, 32, 1024, np.complex64),
}


def package():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    path = pkg.host.library_path()
    have = ctypes.CDLL(path)
    missing = [e[0] for e in pkg.host.ABI if not hasattr(have, e[0])]
    if missing:                                   # (an older build beside this one, --siblings: what it lacks is not called)
        pkg.host.ABI[:] = [e for e in pkg.host.ABI if e[0] not in missing]
    return pkg, path, missing


def setup(key):
    import torch
    pkg, path, _ = package()
    dev = torch.device("cuda", 0)
    title, nch, n, Nphi, ntaps, tx = WORKLOADS[key]
    rng = np.random.default_rng(7)
    T = -(-ntaps // Nphi)
    H = ((rng.standard_normal((nch, ntaps)) + 1j * rng.standard_normal((nch, ntaps))) * Nphi / ntaps).astype(np.complex64)
    PN = (rng.standard_normal((nch, T, P + 1)) + 1j * rng.standard_normal((nch, T, P + 1))) / (T * 32.0 ** np.arange(P + 1))
    rates = np.linspace(2.0, 2.25, nch)
    x = torch.rand((nch, n), device=dev, dtype=torch.float32)
    if np.dtype(tx).kind == "c":
        x = torch.complex(x, torch.rand((nch, n), device=dev, dtype=torch.float32))
    return torch, pkg, path, dev, H, PN, rates, x


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


def opl_of(pkg):
    import re
    src = open(os.path.join(ROOT, "multirate.jl_amd", "csrc", "rates_arb.h")).read()
    return int(re.search(r"^constexpr int kFarrowRatesCtapsOPL = (\d+);", src, flags=re.M).group(1))


def workload(key, emit, kernels_only=False):
    torch, pkg, path, dev, H, PN, rates, x = setup(key)
    title, nch, n, Nphi, ntaps, tx = WORKLOADS[key]
    cplx = np.dtype(tx).kind == "c"
    sync = torch.cuda.synchronize
    f = pkg.FIRFilter.per_channel_complex_taps_and_rates_farrow(H, rates, Nphi, P, pnfb=PN)
    f.bind(tx, nch)
    bound = f.outputlength_bound(n)
    ybuf = torch.empty((nch, bound), dtype=torch.complex64, device=dev)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    emit(f"## {key}: {title}")
    emit(f"    (library {os.path.basename(path)}; bound {bound} outputs a channel: {-(-bound // 512)} tiles of 512 a channel ({-(-bound // 512) * nch} tiles), "
         f"{-(-bound // 1024)} of 1024 ({-(-bound // 1024) * nch}); device banks {PN.size * 16} bytes)")
    emit(f"{'way':<70}{'kernel':<28}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    rows = {}

    def row(name, kernel, one_pass):
        ts, untimed = timed(one_pass, sync)
        rows[name[1]] = ts
        emit(f"{name:<70}{kernel():<28}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")

    # (m), (u): the new filter (nothing waits inside the call: the counts stay on the device)
    for name, mode in (("(m) new filter, multi kernel", "1"), ("(u) new filter, universal kernel", "0")):
        os.environ[SWITCH] = mode
        row(name, f.last_kernel_name, lambda: f._filt_into_rates(ybuf, x, counts))
    os.environ.pop(SWITCH)
    f._filt_into_rates(ybuf, x, counts)
    default = "m" if f.last_kernel_name() == "farrow_rates_ctaps_multi" else "u"
    emit(f"    (default plan, {SWITCH} unset: {f.last_kernel_name()}; outputs of the last pass: {int(counts.sum())})")
    spread = max(rows["m"]) - min(rows["m"]), max(rows["u"]) - min(rows["u"])
    med = {k: statistics.median(v) for k, v in rows.items()}
    if kernels_only:
        emit(f"    (u) / (m): {med['u'] / med['m']:.3f}x (spread of the repeats: m {spread[0]:.3f} ms, u {spread[1]:.3f} ms)")
        emit("")
        f.close()
        return

    # (h), (p), (d): an update before every pass, through the host (rows fitted, banks handed over) and in stream order
    def host_fit():
        f.set_channel_ctaps_farrow(H)
        f._filt_into_rates(ybuf, x, counts)
    row("(h) new filter, default plan, set_channel_ctaps_farrow each pass", f.last_kernel_name, host_fit)

    def host_banks():
        f.set_channel_pnfb_ctaps(PN)
        f._filt_into_rates(ybuf, x, counts)
    row("(p) new filter, default plan, set_channel_pnfb_ctaps each pass", f.last_kernel_name, host_banks)
    PN_d = torch.from_numpy(PN).to(dev)

    def device_update():
        f.set_channel_pnfb_ctaps_device(PN_d)
        f._filt_into_rates(ybuf, x, counts)
    row("(d) new filter, default plan, set_channel_pnfb_ctaps_device each pass", f.last_kernel_name, device_update)
    f.close()

    # (a): one-channel complex-tap filters, each with its own bank at its own rate
    ns = min(nch, SINGLES_MAX)
    part = "" if ns == nch else f", first {ns} ch only"
    fs = [pkg.FIRFilter.complex_taps_farrow(H[c], float(rates[c]), Nphi, P, pnfb=PN[c]) for c in range(ns)]
    xs = [x[c] for c in range(ns)]
    for fc in fs:
        fc.bind(tx, 1)
    ys = [ybuf[c, :bound] for c in range(ns)]
    ms = pkg.MultiStream(fs, ys, xs)
    row("(a) filt_multi, one-channel complex-tap filters" + part, fs[0].last_kernel_name, ms.run)
    for fc in fs:
        fc.close()

    # (b): real bank filters over the real and the imaginary banks, and a combine pass
    Hr = np.ascontiguousarray(H.real)
    PNr, PNi = np.ascontiguousarray(PN.real), np.ascontiguousarray(PN.imag)
    parts = [x.real.contiguous(), x.imag.contiguous()] if cplx else [x]
    reals = [(pkg.FIRFilter.per_channel_taps_and_rates_farrow(Hr, rates, Nphi, P, pnfb=M), torch.empty((nch, bound), dtype=torch.float32, device=dev), p)
             for p in parts for M in (PNr, PNi)]                            # (re on xr, im on xr[, re on xi, im on xi])
    for g, _, _ in reals:
        g.bind(np.float32, nch)

    def real_filters():
        for g, y, p in reals:
            g._filt_into_rates(y, p, counts)
        if cplx:
            torch.complex(reals[0][1] - reals[3][1], reals[1][1] + reals[2][1], out=ybuf)
        else:
            torch.complex(reals[0][1], reals[1][1], out=ybuf)
    row(f"(b) {len(reals)} real per_channel_taps_and_rates_farrow filters + combine", reals[0][0].last_kernel_name, real_filters)
    for g, _, _ in reals[1:]:
        g.close()
    # (c): the real-tap bank filter of the same shape (real samples: the first of (b); complex samples: a filter of its own)
    g = reals[0][0]
    yfloor = reals[0][1]
    if cplx:
        g.close()
        g = pkg.FIRFilter.per_channel_taps_and_rates_farrow(Hr, rates, Nphi, P, pnfb=PNr)
        g.bind(tx, nch)
        yfloor = ybuf
    row("(c) real-tap per_channel_taps_and_rates_farrow, default plan (floor)", g.last_kernel_name, lambda: g._filt_into_rates(yfloor, x, counts))
    g.close()

    med = {k: statistics.median(v) for k, v in rows.items()}
    med["a"] *= nch / ns                          # (one launch sequence per channel: scaled to all nch channels)
    best = min(med["m"], med["u"])
    emit(f"    (u) / (m): {med['u'] / med['m']:.3f}x (spread of the repeats: m {spread[0]:.3f} ms, u {spread[1]:.3f} ms); (a) / best: {med['a'] / best:.2f}x; "
         f"(b) / best: {med['b'] / best:.2f}x; best / (c): {best / med['c']:.2f}x; (h) - ({default}): {med['h'] - med[default]:.3f} ms; "
         f"(p) - ({default}): {med['p'] - med[default]:.3f} ms; (d) - ({default}): {med['d'] - med[default]:.3f} ms (best: the faster of (m), (u))")
    if ns != nch:
        emit(f"    ((a) in the ratios: the measured row times {nch}/{ns} = {med['a']:.1f} ms for all {nch} channels)")
    emit("")


def siblings(emit):
    """the five older per-channel-rate filters at 4096 ch x 1e4 Float32 on their default plans: rates_call gained one branch"""
    import torch
    pkg, path, missing = package()
    dev = torch.device("cuda", 0)
    nch, n, Nphi, ntaps = 4096, 10_000, 32, 250
    rng = np.random.default_rng(7)
    Hr = (rng.standard_normal((nch, ntaps)) * Nphi / ntaps).astype(np.float32)
    Hc = (Hr + 1j * Hr[::-1]).astype(np.complex64)
    rates = np.linspace(2.0, 2.25, nch)
    x = torch.rand((nch, n), device=dev, dtype=torch.float32)
    counts = torch.zeros(nch, dtype=torch.int64, device=dev)
    emit(f"## siblings at 4096 ch x 1e4 Float32, library {os.path.basename(path)}" + (f" (without {', '.join(missing)})" if missing else ""))
    emit(f"{'filter':<44}{'kernel':<28}{'median ms':>10}{'min':>9}{'max':>9}{'untimed':>9}")
    makers = (("per_channel_rates", lambda: pkg.FIRFilter.per_channel_rates(Hr[0], rates, Nphi)),
              ("per_channel_taps_and_rates", lambda: pkg.FIRFilter.per_channel_taps_and_rates(Hr, rates, Nphi)),
              ("per_channel_complex_taps_and_rates", lambda: pkg.FIRFilter.per_channel_complex_taps_and_rates(Hc, rates, Nphi)),
              ("per_channel_rates_farrow", lambda: pkg.FIRFilter.per_channel_rates_farrow(Hr[0], rates, Nphi, P)),
              ("per_channel_taps_and_rates_farrow", lambda: pkg.FIRFilter.per_channel_taps_and_rates_farrow(Hr, rates, Nphi, P)))
    for name, make in makers:
        f = make()
        f.bind(np.float32, nch)
        y = torch.empty((nch, f.outputlength_bound(n)), dtype=torch.complex64 if f.output_dtype.kind == "c" else torch.float32, device=dev)
        ts, untimed = timed(lambda: f._filt_into_rates(y, x, counts), torch.cuda.synchronize)
        emit(f"{name:<44}{f.last_kernel_name():<28}{statistics.median(ts):>10.3f}{min(ts):>9.3f}{max(ts):>9.3f}{untimed:>9d}")
        f.close()
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
    if args and args[0] == "--siblings":
        siblings(emit)
    elif args and args[0] == "--kernels":
        for key in args[1:]:
            workload(key, emit, kernels_only=True)
    else:
        for key in args or list(WORKLOADS):
            workload(key, emit)


if __name__ == "__main__":
    main()
