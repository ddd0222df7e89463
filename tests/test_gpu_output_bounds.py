"""GPU tests of PLACEMENT (need one MI355X): every kernel of the library, through every entry point, writes y[c][0 .. count) of every
channel row and nothing else -- whatever y's alignment and row stride (include/multirate_hip.h, "the hot path").

The other GPU modules take their outputs from f.filt(...) or from a fresh (nch, count) tensor: the base is 512-byte aligned, the row
stride is the count, an element past a row's end is the next row's first and the allocator's slack swallows the rest.  Here y is a
VIEW into a buffer whose every byte is 0xA5 (tests/output_bounds_cases.py: make_buffer) with a guard row above and below and guard
columns in front and behind; x is a view too.  The outputs of the calls of a stream lie end to end in that buffer, as a caller's
streaming loop puts them; after EVERY call the whole buffer comes back to the host and

    * last_kernel_name() is the case's kernel,
    * y[c][0 .. k + count), the outputs of every call so far, are bit for bit the reference's (the C oracle for real taps, the
      restatement classes for complex taps -- never the library),
    * every byte outside the outputs written so far is still 0xA5 (assert_only_written),

and after the last call the history and the stream state are the reference's.  Layouts (element offset of y, parity of the row stride,
element offset of x): tight (0, stride == capacity, 0), A (1, odd, 1), B (2, even, 3), C (3, odd, 2); 8- and 16-byte outputs: tight and A
(the other offsets repeat residues of the base address modulo 16), and B for the lane kernels (their 16-byte stores need an aligned base
AND an even stride); "1d": layout A with ONE channel and 1-D tensors.

Entry points per (case, layout): exact (filt_into, capacity == count), slack (capacity = count + 5; FIRArbitrary / FIRFarrow:
outputlength(n) + 2, the room filt() gives; calls this short are scheduled by the host), async (filt_into_async, capacity =
outputlength_bound(n), the count from the device), chunked (filt_into_chunked with MRHIP_CHUNKED_PER_CALL=1 and a chunk whose first
piece has an odd count: the later launches start at odd elements of y), launch_max (one filt_into call with MRHIP_LAUNCH_MAX below the
call length), and for FIRArbitrary / FIRFarrow estimate (two calls of about 7000 outputs, capacity outputlength(n) + 2, the schedule
evaluated on the device: the filter kernel is launched for the ESTIMATE and takes the count from the call record -- the columns from
count to the estimate must stay poison).  Further tests: the ring (open_ring().push, both completion protocols), FilterCascade,
MultiStream with caller-owned outputs, BUFFER_TOO_SMALL.  MRHIP_SCHED_PIECE is read once per process (api.hip: a function-local
static): the host's piecewise schedule, whose later launches start at y + k, is reached in a child process that runs the slack entry of
the FIRArbitrary / FIRFarrow cases again with a piece of 301 outputs.

STRICT everywhere; FUSED (against the oracle's fused switch), every entry point again, for the tight layout and layout A of the kernels
that have FUSED instantiations.  The module is run as a whole: the last test asserts that every kernel name of the table was reached.
"""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import output_bounds_cases as B
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

ENTRIES = ("exact", "slack", "async", "chunked", "launch_max")
REACHED = {}                                   # kernel name -> entry points that reached it
ONLY_ENTRIES = "OUTPUT_BOUNDS_ONLY_ENTRIES"    # set for the child process of the piecewise-schedule test: the entry points it runs
SWITCHES = sorted({k for c in B.ALL_CASES for k, _ in c.env} |
                  {"MRHIP_FORCE_GENERIC", "MRHIP_LAUNCH_MAX", "MRHIP_CHUNKED_PER_CALL", "MRHIP_ARB_LANE", "MRHIP_OPAIR", "MRHIP_STREAM",
                   "MRHIP_SCHED_PREFIX", "MRHIP_SCHED_PMAX", "MRHIP_SCHED_DEVICE_MIN"})


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _set_env(monkeypatch, case, extra=()):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    for k, v in tuple(case.env) + tuple(extra):
        monkeypatch.setenv(k, v)


_REFS = {}


def _reference(pkg, O, case, nch, fused, sizes):
    """taps, signal and, per call of `sizes`, the reference's outputs (nch, count); end state; histories.  Computed once and shared."""
    key = (case.id, nch, fused, tuple(sizes))
    if key not in _REFS:
        taps = B.make_taps(case, nch)
        x = B.make_signal(case, sum(sizes), nch)
        O.set_fused(fused)
        try:
            refs, pnfb = B.make_refs(pkg, O, case, taps, nch)
            outs, pos = [], 0
            for n in sizes:
                outs.append(np.stack([r.filt(x[c, pos:pos + n]) for c, r in enumerate(refs)]))
                pos += n
        finally:
            O.set_fused(False)
        assert len({r.state() for r in refs}) == 1
        for o in outs:
            assert o.dtype == case.out_dtype
            o.setflags(write=False)
        x.setflags(write=False)
        _REFS[key] = dict(taps=taps, x=x, pnfb=pnfb, outs=outs, state=refs[0].state(), hists=[np.array(r.history()) for r in refs])
    return _REFS[key]


def _x_view(torch, x, layout, one_d):
    """x on the device: the plain tensor (tight) or a view at element offset ox whose row stride is not the length"""
    ox = B.LAYOUTS[layout][2]
    n = x.shape[1]
    if layout == "tight":
        xd = torch.tensor(x, device="cuda")
    else:
        part = torch.tensor(x, device="cuda")
        big = torch.zeros((x.shape[0], ox + n + 5), dtype=part.dtype, device="cuda")
        big[:, ox:ox + n] = part
        xd = big[:, ox:ox + n]
    return xd[0] if one_d else xd


def _check_call(backing, geom, outs, what):
    """one copy of the whole buffer to the host: EVERY output written so far (`outs`: the reference's outputs of the calls up to this one,
    end to end -- a call that stores in front of its own place would spoil an earlier call's) against the reference, every other byte
    against the poison"""
    nch, cap, oy, pad = geom
    host = backing.cpu().numpy()
    want = np.concatenate(outs, axis=1)
    if want.shape[1]:
        assert_bit_equal(host[1:1 + nch, oy:oy + want.shape[1]], want, what + ": outputs")
    B.assert_only_written(host, nch, cap, oy, pad, want.shape[1], what)


def _end_state(case, f, ref, nch, what):
    assert B.library_state(f, case.kind) == ref["state"], (what, B.library_state(f, case.kind), ref["state"])
    hist = np.asarray(f.history).reshape(nch, -1)
    for c in range(nch):
        assert_bit_equal(hist[c], ref["hists"][c], f"{what}: history of channel {c}")


def _run(torch, pkg, O, monkeypatch, case, layout, entry, one_d=False, fused=False):
    nch = 1 if one_d else case.nch
    oy = B.LAYOUTS[layout][0]
    es = case.out_dtype.itemsize
    plan = B.plan_sizes(O, case)
    n_all = sum(plan)
    extra_env = ()
    if entry in ("chunked", "launch_max"):
        piece = B.odd_piece(O, case, n_all, n_all // 3 + 1)      # (three pieces, the last about as long as the others)
        if entry == "launch_max" and case.kind == "rational" and case.M == 1:
            piece *= case.L                     # (api.hip: a FIRInterpolator's MRHIP_LAUNCH_MAX counts outputs)
        extra_env = (("MRHIP_CHUNKED_PER_CALL", "1"),) if entry == "chunked" else (("MRHIP_LAUNCH_MAX", str(piece)),)
    if entry == "estimate":
        # two calls of about 7000 outputs with the schedule evaluated ON THE DEVICE (the switches of test_gpu_schedule.py: a host prefix of
        # 4096 outputs, device evaluation from 6000): api.hip then launches the filter kernel for the estimate before the count is known
        n1 = int(np.ceil(7000 / float(case.ratio)))
        plan = [n1, n1 + 37]
        assert sum(plan) <= B.MAX_SIGNAL
        extra_env = (("MRHIP_SCHED_PREFIX", "4096"), ("MRHIP_SCHED_PMAX", "8192"), ("MRHIP_SCHED_DEVICE_MIN", "6000"))
    sizes = plan if entry in ("exact", "slack", "async", "estimate") else B.pieces(n_all, piece) if entry == "chunked" else [n_all]
    ref = _reference(pkg, O, case, nch, fused, sizes)
    counts = [o.shape[1] for o in ref["outs"]]
    total = sum(counts)
    _set_env(monkeypatch, case, extra_env)
    f = B.make_filter(pkg, case, ref["taps"], nch, ref["pnfb"], fused)
    what0 = f"{case.id} layout={layout}{' 1-D' if one_d else ''} entry={entry}{' FUSED' if fused else ''}"
    assert np.dtype(f.output_dtype) == case.out_dtype, what0
    xd = _x_view(torch, ref["x"], layout, one_d)
    bounds = [f.outputlength_bound(n) if n else 0 for n in sizes] if entry == "async" else None
    room = 0 if entry in ("exact", "chunked", "launch_max") else 16 + (max(b - c for b, c in zip(bounds, counts)) if bounds else 0)
    cap = total + room
    pad = B.row_pad(layout, oy, cap, es)
    y, backing = B.make_buffer(torch, case.out_dtype, nch, cap, oy, pad)
    yv = y[0] if one_d else y
    geom = (nch, cap, oy, pad)
    cnt_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    kernel = case.async_name if entry == "async" else case.kernel      # (output_bounds_cases.py: ASYNC_KERNEL)
    if entry in ("chunked", "launch_max"):
        if entry == "chunked":
            got = f.filt_into_chunked(yv[..., :total], xd, piece)
        else:
            got = f.filt_into(yv[..., :total], xd)
        torch.cuda.current_stream().synchronize()
        assert got == total, (what0, got, total)
        assert f.last_kernel_name() == case.kernel, (what0, f.last_kernel_name())
        _check_call(backing, geom, ref["outs"], what0)
    else:
        k = pos = 0
        for i, (n, cnt) in enumerate(zip(sizes, counts)):
            what = f"{what0} call {i} ({n} samples, {cnt} outputs at element {k})"
            xi = xd[..., pos:pos + n]
            if entry == "exact":
                cap_i = cnt
            elif entry in ("slack", "estimate"):
                cap_i = cnt + 5 if case.kind == "rational" else max(f.outputlength(n), 0) + 2
            else:
                cap_i = bounds[i]
            assert cnt <= cap_i and k + cap_i <= cap, (what, cap_i, cap)
            yi = yv[..., k:k + cap_i]
            if entry == "async":
                f.filt_into_async(yi, xi, count=cnt_dev)
                f.sync_state()
                got = int(cnt_dev.item())
            else:
                got = f.filt_into(yi, xi)
            torch.cuda.current_stream().synchronize()
            assert got == cnt, (what, got, cnt)
            if cnt and (i in (0, 3) or not case.short_calls_elsewhere or entry == "estimate"):
                assert f.last_kernel_name() == kernel, (what, f.last_kernel_name())
            _check_call(backing, geom, ref["outs"][:i + 1], what)
            k += cnt
            pos += n
    _end_state(case, f, ref, nch, what0)
    if entry == "estimate":
        info = f.schedule_info()
        assert info["device_pieces"] > 0 or info["periodic_steps"] > 0, (what0, info)     # (the schedule really ran on the device)
    REACHED.setdefault(kernel, set()).add(entry)
    f.close()


def _params():
    out = []
    for case in B.ALL_CASES:
        for layout in B.layouts_of(case):
            out.append(pytest.param(case, layout, False, id=f"{case.id}-{layout}"))
        if case.one_channel:
            out.append(pytest.param(case, "A", True, id=f"{case.id}-1d"))
    return out


@pytest.mark.parametrize("case,layout,one_d", _params())
def test_every_entry_point_writes_only_its_outputs(pkg, O, torch_cuda, monkeypatch, case, layout, one_d):
    entries = ENTRIES + (("estimate",) if case.kind != "rational" else ())
    if os.environ.get(ONLY_ENTRIES):                       # (the child process of the piecewise-schedule test below)
        entries = tuple(os.environ[ONLY_ENTRIES].split(","))
    for entry in entries:
        _run(torch_cuda, pkg, O, monkeypatch, case, layout, entry, one_d=one_d)
    if case.fused and not one_d and layout in ("tight", "A"):
        for entry in entries:
            _run(torch_cuda, pkg, O, monkeypatch, case, layout, entry, fused=True)


# ---- the ring -------------------------------------------------------------------------------------------------------------------------
def _ring_params():
    return [pytest.param(c, layout, protocol, id=f"{c.id}-{layout}-{protocol}")
            for c in B.ALL_CASES if c.ring for layout in B.layouts_of(c) for protocol in ("write_through", "write_back")]


@pytest.mark.parametrize("case,layout,protocol", _ring_params())
def test_ring_pushes_write_only_their_outputs(pkg, O, torch_cuda, monkeypatch, case, layout, protocol):
    """open_ring().push: three unequal chunks, the middle one shorter than the history, under both completion protocols that
    test_gpu_ring.py exercises: the default (chunks of less than 32 MB of outputs: the resident kernel's write-through stores) and
    MRHIP_RING_FLUSH_MIN_MB=0 (plain stores, completed by L2 write-backs; ring_api.inc falls back to write-through stores on a device
    that does not show eight XCDs, which ring.info() tells)"""
    torch = torch_cuda
    _set_env(monkeypatch, case)
    monkeypatch.setenv("MRHIP_RING_IDLE_MS", "500")
    if protocol == "write_back":
        monkeypatch.setenv("MRHIP_RING_FLUSH_MIN_MB", "0")
    else:
        monkeypatch.delenv("MRHIP_RING_FLUSH_MIN_MB", raising=False)
    plan = B.plan_sizes(O, case)
    T = -(-case.hlen // case.L)
    sizes = [plan[0], max(1, (T - 1) // 2), plan[3]]
    nch, oy, es = case.nch, B.LAYOUTS[layout][0], case.out_dtype.itemsize
    ref = _reference(pkg, O, case, nch, False, sizes)
    counts = [o.shape[1] for o in ref["outs"]]
    f = B.make_filter(pkg, case, ref["taps"], nch)
    xd = _x_view(torch, ref["x"], layout, False)
    cap = sum(counts)
    pad = B.row_pad(layout, oy, cap, es)
    y, backing = B.make_buffer(torch, case.out_dtype, nch, cap, oy, pad)
    torch.cuda.current_stream().synchronize()               # x and the poison are complete before the first push
    with f.open_ring() as ring:
        info = ring.info()
        assert info["resident"], "this shape is served by the resident kernel"
        k = pos = 0
        for i, (n, cnt) in enumerate(zip(sizes, counts)):
            what = f"{case.id} layout={layout} ring chunk {i} ({n} samples, {cnt} outputs at element {k})"
            got, seq = ring.push(y[:, k:k + cnt], xd[:, pos:pos + n])
            assert got == cnt, (what, got, cnt)
            ring.wait(seq)
            _check_call(backing, (nch, cap, oy, pad), ref["outs"][:i + 1], what)
            k += cnt
            pos += n
        ring.drain()
    assert f.last_kernel_name() == case.kernel
    _end_state(case, f, ref, nch, f"{case.id} ring")
    REACHED.setdefault(case.kernel, set()).add("ring" if protocol == "write_through" else "ring_write_back" if info["xcds"] == 8 else "ring")
    f.close()


# ---- BUFFER_TOO_SMALL ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["opair-147_160-f32", "arb_pipe-f64", "farrow_pipe-f64"])
def test_a_buffer_one_element_short_is_refused_and_left_alone(pkg, O, torch_cuda, monkeypatch, case_id):
    """capacity = count - 1: MRHIP_ERR_BUFFER_TOO_SMALL, every byte of the buffer still poison, state and history untouched (the same
    call into a buffer that has the room then gives the reference's outputs)"""
    torch = torch_cuda
    case = next(c for c in B.ALL_CASES if c.id == case_id)
    _set_env(monkeypatch, case)
    n = B.plan_sizes(O, case)[0]
    nch, layout = case.nch, "A"
    oy, es = B.LAYOUTS[layout][0], case.out_dtype.itemsize
    ref = _reference(pkg, O, case, nch, False, [n])
    cnt = ref["outs"][0].shape[1]
    f = B.make_filter(pkg, case, ref["taps"], nch, ref["pnfb"])
    before = B.library_state(f, case.kind)
    xd = _x_view(torch, ref["x"], layout, False)
    pad = B.row_pad(layout, oy, cnt, es)
    y, backing = B.make_buffer(torch, case.out_dtype, nch, cnt, oy, pad)
    with pytest.raises(pkg.MultirateHIPError) as ei:
        f.filt_into(y[:, :cnt - 1], xd)
    assert ei.value.code == 2, ei.value                      # MRHIP_ERR_BUFFER_TOO_SMALL
    torch.cuda.synchronize()
    B.assert_only_written(backing, nch, cnt, oy, pad, 0, f"{case.id}: refused call")
    assert B.library_state(f, case.kind) == before
    assert not np.asarray(f.history).any()
    assert f.filt_into(y, xd) == cnt
    torch.cuda.synchronize()
    _check_call(backing, (nch, cnt, oy, pad), ref["outs"], f"{case.id}: the call after the refused one")
    _end_state(case, f, ref, nch, case.id)
    f.close()


# ---- FilterCascade ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "A", "C"])
@pytest.mark.parametrize("second", ["rational", "arbitrary"])
def test_cascade_writes_only_the_last_stage_s_outputs(pkg, O, torch_cuda, monkeypatch, second, layout):
    """FIRDecimator 1//2, then FIRRational 3//2 or FIRArbitrary 1.37: filt_into (exact capacity) and filt_into_async (the bound);
    only the last stage writes y, the stages between write buffers of the cascade"""
    torch = torch_cuda
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(11)
    nch, sizes = 3, [3001, 1, 2, 3100]
    h1 = (rng.standard_normal(31) / 8).astype(np.float32)
    h2 = (rng.standard_normal(3 * 24 if second == "rational" else 32 * 8) / 4).astype(np.float32)
    r2 = Fraction(3, 2) if second == "rational" else 1.37
    x = rng.standard_normal((nch, sum(sizes))).astype(np.float32)
    o1 = [O.FIRFilter(h1, Fraction(1, 2), tx=np.float32) for _ in range(nch)]
    o2 = [O.FIRFilter(h2, r2, 32, tx=np.float32) for _ in range(nch)]
    outs, pos = [], 0
    for n in sizes:
        outs.append(np.stack([o2[c].filt(o1[c].filt(x[c, pos:pos + n])) for c in range(nch)]))
        pos += n
    counts = [o.shape[1] for o in outs]
    assert counts[0] > 768 and counts[3] > 768
    oy = B.LAYOUTS[layout][0]
    xd = _x_view(torch, x, layout, False)
    for mode in ("into", "async"):
        cas = pkg.FilterCascade(pkg.FIRFilter(h1, Fraction(1, 2)).bind(np.float32, nch), pkg.FIRFilter(h2, r2, 32).bind(np.float32, nch))
        bounds = [cas.outputlength_bound(n) for n in sizes]
        cap = sum(counts) + (16 + max(b - c for b, c in zip(bounds, counts)) if mode == "async" else 0)
        pad = B.row_pad(layout, oy, cap, 4)
        y, backing = B.make_buffer(torch, np.float32, nch, cap, oy, pad)
        cnt_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = pos = 0
        for i, (n, cnt) in enumerate(zip(sizes, counts)):
            what = f"cascade 1//2 -> {r2} layout={layout} {mode} call {i} ({n} samples, {cnt} outputs at element {k})"
            if mode == "into" or i == 0:                    # (the first call is a plain one: it allocates the buffers between the stages)
                got = cas.filt_into(y[:, k:k + cnt], xd[:, pos:pos + n])
            else:
                cas.filt_into_async(y[:, k:k + bounds[i]], xd[:, pos:pos + n], cnt_dev)
                torch.cuda.synchronize()
                got = int(cnt_dev.item())
            torch.cuda.synchronize()
            assert got == cnt, (what, got, cnt)
            _check_call(backing, (nch, cap, oy, pad), outs[:i + 1], what)
            k += cnt
            pos += n
        for st in cas.stages:
            st.sync_state()
        last, so = cas.stages[1], o2[0].state
        assert last.state.inputDeficit == so.inputDeficit and (second == "rational" and last.state.phiIdx == so.phiIdx or
                                                               second == "arbitrary" and last.state.phiAccumulator == so.phiAccumulator)
        assert_bit_equal(np.asarray(last.history).reshape(nch, -1)[nch - 1], o2[nch - 1].history, "history of the last stage")
        REACHED.setdefault(last.last_kernel_name(), set()).add("cascade")
        cas.close()


# ---- several streams, one call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("oy", [0, 1, 3])
def test_multistream_writes_only_its_outputs_into_caller_owned_buffers(pkg, O, torch_cuda, monkeypatch, oy):
    """MultiStream / mrhip_filt_device_multi with caller-owned ys: FIRRational 147//160, FIRDecimator 1//4 and FIRArbitrary side by side,
    two rounds; ys[i] is a contiguous (nch_i, capacity_i) block at element offset oy of a poisoned buffer (the entry point takes the
    capacity as the row stride), capacity_i = outputlength_bound: the columns count .. capacity of every row and the guards stay poison"""
    torch = torch_cuda
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(12)
    specs = [(Fraction(147, 160), 147 * 24, 2, 2001), (Fraction(1, 4), 128, 3, 4003), (1.37, 32 * 8, 1, 1500)]
    filters, refs, xs_h, xs, ys, backs, caps = [], [], [], [], [], [], []
    for ratio, hlen, nch, n in specs:
        h = (rng.standard_normal(hlen) / 8).astype(np.float32)
        f = pkg.FIRFilter(h, ratio, 32).bind(np.float32, nch)
        cap = f.outputlength_bound(n)
        x = rng.standard_normal((2, nch, n)).astype(np.float32)
        # one "row" of nch * cap elements: rows of the stream back to back, guards in front, behind, above and below
        y, backing = B.make_buffer(torch, np.float32, 1, nch * cap, oy, 2)
        filters.append(f); refs.append([O.FIRFilter(h, ratio, 32, tx=np.float32) for _ in range(nch)])
        xs_h.append(x); xs.append(torch.from_numpy(x[0]).cuda()); ys.append(y[0].view(nch, cap)); backs.append(backing); caps.append(cap)
    ms = pkg.MultiStream(filters, ys, xs)
    for rnd in range(2):
        for xd, x in zip(xs, xs_h):
            xd.copy_(torch.from_numpy(x[rnd]).cuda())
        for b in backs:
            b.view(-1).view(torch.uint8).fill_(B.POISON)
        got = list(ms.run())
        torch.cuda.synchronize()
        for i, (ratio, hlen, nch, n) in enumerate(specs):
            want = np.stack([r.filt(xs_h[i][rnd, c]) for c, r in enumerate(refs[i])])
            cnt, cap = want.shape[1], caps[i]
            what = f"MultiStream oy={oy} round {rnd} stream {i} ({ratio})"
            assert got[i] == cnt and 0 < cnt <= cap, (what, got[i], cnt, cap)
            by, es = B.backing_bytes(backs[i])
            assert_bit_equal(ys[i].cpu().numpy()[:, :cnt], want, what)
            allowed = np.zeros(by.shape, dtype=bool)
            for c in range(nch):
                allowed[1, (oy + c * cap) * es:(oy + c * cap + cnt) * es] = True
            hit = B.first_stray(by, allowed)
            assert hit is None, f"{what}: stray byte at row {hit[0] - 1}, element {hit[1] // es - oy} of the block ({nch} rows of {cap}, count {cnt})"
            REACHED.setdefault(filters[i].last_kernel_name(), set()).add("multi")
    for f in filters:
        f.close()


# ---- the host's piecewise schedule: a process of its own ---------------------------------------------------------------------------------
def test_host_piecewise_schedule_writes_later_pieces_at_odd_offsets(pkg, torch_cuda):
    """A FIRArbitrary / FIRFarrow call whose estimate exceeds two pieces of MRHIP_SCHED_PIECE outputs and fits the buffer is scheduled by the
    host piece by piece (api.hip: arb_call_host_pieces), every piece a launch at y + k.  The switch is read ONCE per process, so the
    FIRArbitrary / FIRFarrow cases run their slack-capacity entry again, tight layout (an even row stride where the capacity is even:
    the lane kernel's 16-byte stores) and layout A, in a child process with a piece of 301 outputs: these
    calls (about 1000 outputs, capacity = the estimate) then take that path -- MRHIP_DEBUG=2 makes it say so -- and their launches start at
    elements 301, 602, ... of the call's place in y."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ids = [f"tests/test_gpu_output_bounds.py::test_every_entry_point_writes_only_its_outputs[{c.id}-{layout}]"
           for c in B.ALL_CASES if c.kind != "rational" for layout in ("tight", "A")]
    env = dict(os.environ, MRHIP_SCHED_PIECE="301", MRHIP_DEBUG="2", **{ONLY_ENTRIES: "slack"})
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", *ids], cwd=root, env=env, capture_output=True,
                       text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and f"{len(ids)} passed" in r.stdout, out[-3000:]
    assert out.count("[mrhip] arbitrary schedule: recurrence") >= len(ids), out[-3000:]      # (printed by arb_call_host_pieces only)


# ---- coverage (the module is run as a whole) ------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_table_was_reached_through_every_entry_point_it_is_eligible_for():
    assert set(REACHED) >= set(B.CASES), sorted(set(B.CASES) - set(REACHED))
    assert set(B.CASES) == B.kernel_names_in_csrc()
    for kernel in B.CASES:
        # (a kernel of ASYNC_KERNEL takes no device-planned call: its shapes' asynchronous calls were checked on the kernel named there)
        want = set(ENTRIES) - ({"async"} if kernel in B.ASYNC_KERNEL else set()) | ({"estimate"} if B.CASES[kernel][0].kind != "rational" else set())
        assert want <= REACHED[kernel], (kernel, REACHED[kernel])
    assert "ring" in REACHED["rational_opair_kernel"]
    assert "ring_write_back" in REACHED["rational_opair_kernel"], "no ring test ran the write-back protocol (a device without eight XCDs?)"
    assert any("cascade" in v for v in REACHED.values()) and any("multi" in v for v in REACHED.values())
