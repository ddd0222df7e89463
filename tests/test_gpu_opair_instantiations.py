"""Every rational_opair_kernel instantiation the dispatcher can reach, against the oracle (needs one MI355X).

rational_opair_kernel<T, FUSED, NC, SMIN, TXS, R, MODE> (csrc/opair_kernel.inc) is unrolled per tapsPerPhi T: each T has its own
register ring, its own counted waits, its own shifted tap columns and its own exact no-op end slots.  The table of what
plan_rational_opair / launch_rational_opair can reach is written out in opair_cases.py (STRICT_COUNT: 832 STRICT instantiations,
FUSED_COUNT: 144 FUSED ones, 24 (type, SMIN, T) with T in {24, 32} that have the PLAIN modes 1 and 3 and the resident ring's mode 2
next to mode 0) and every entry is run here with the dispatch that ships: no MRHIP_* switch is set (the guard's child process
alone sets MRHIP_DEBUG=1 to read the launch geometry).

Per instantiation one ratio of opair_cases.RATIOS[SMIN], rotated by T + index(type), hLen = T*L - r with r rotating over
0, 1, L//2, L-1, standard-normal taps with up to three exact zeros (min(3, hLen // 4): never a zero filter), and two shapes:

* many tiles: 64 channels built from 4 distinct rows, chunks [p, 1, 13, rest] with p prime; runs of -0.0 longer than a lane's run of
  samples (one of them across the short chunks' boundaries), +Inf / -Inf in row 0, a 3-sample NaN run in row 3; the signal is
  uploaded afresh for every case, so the first call reads cold lines.  `rest` gives opair_cases.many_outputs() outputs per
  channel, sized per instantiation: workgroups take tiles by dynamic grabs only when tiles > 3 x grid (pair_grid:
  static_grabs false), the grid is as many workgroups as the 256 CUs hold at once -- the 1 to 4 per CU the plan sizes its LDS stages
  for, up to 6 where a tile stops short of its stage (opair_cases.plan: wg_bound, an upper bound by LDS and wave slots) -- and a
  tile is as many steps as fit a stage (the plan shortens tiles only until a call has 1 024 of them, which is below 3 x grid
  wherever more than one workgroup shares a CU) -- so every instantiation needs about 3 x 256 x 150 KiB / stages of input
  whatever its ratio: 30 to 90 MB over the 64 channels.  Outputs per channel of the large chunk, per SMIN (fewest .. most over the
  types and T): SMIN 0: 58 945 .. 527 773, 1: 30 250 .. 223 830, 2: 40 262 .. 94 928, 3: 30 250 .. 64 839, 4: 25 000 .. 53 587,
  5: 25 000 .. 40 262.  Calls of that size are past n_out * nch = 2^22 in most cases, so T = 24 and 32 run MODE 1 in the large
  chunk there; their MODE 3 has a many-tiles call of its own in test_modes_of_24_and_32_taps.
  test_many_tiles_shape_takes_dynamic_grabs checks the premise against the geometry the library reports.
* one short call: 3 channels, a little over two tiles (a partial last step in a partial last tile), then a chunk of T - 1 samples.

Checked against O.FIRFilter run over the same chunks: the outputs of all channels bit for bit (NaNs in the same places -- their
payload is the host FPU's on the oracle side -- everything else bit-equal), the history of all channels, (phiIdx, inputDeficit), and
last_kernel_name() == "rational_opair_kernel" after every call that has outputs.  Each parameter counts the instantiations it
reached and asserts its row of the table; the totals are asserted by the last tests of the module (run the module as a whole).

Instantiations excluded: none."""
import math
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import opair_cases as oc
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

OPAIR = "rational_opair_kernel"
_REACHED = {"strict": {}, "fused": {}, "mode0": set(), "mode1": set(), "mode2": set(), "mode3": set()}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _tdtype(torch, d):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128}[np.dtype(d)]


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def _cuts(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def _oracle(O, h, ratio, tx, rows, sizes):
    """the oracle's chunk loop over the distinct rows: per row the outputs chunk by chunk, and the filters (end state, history)"""
    cuts = _cuts(sizes)
    fos = [O.FIRFilter(h, ratio, tx=tx) for _ in rows]
    outs = [[fo.filt(r[a:b]) for a, b in zip(cuts[:-1], cuts[1:])] for fo, r in zip(fos, rows)]
    return outs, fos


def _assert_equal_but_nan_payload(got, want, what):
    ft = np.float64 if want.dtype in (np.float64, np.complex128) else np.float32
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    g, w = np.ascontiguousarray(got).view(ft), np.ascontiguousarray(want).view(ft)
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"NaN positions: {what}"
    ok = ~np.isnan(w)
    assert_bit_equal(g[ok], w[ok], what)


def _check_outputs(torch, ys, ref, reps, what):
    """ys: per chunk the (channels, n) device tensor; ref: per distinct row its outputs chunk by chunk; channel i carries row
    i % len(ref).  Compared on the device (words equal, or NaN on both sides); a difference is reported by the host comparison."""
    for i, y in enumerate(ys):
        want = np.stack([r[i] for r in ref])
        assert tuple(y.shape) == (len(ref) * reps, want.shape[1]), f"{what}: chunk {i}: {tuple(y.shape)} vs {reps} x {want.shape}"
        if want.shape[1] == 0:
            continue
        w = torch.from_numpy(want).cuda()
        assert y.dtype == w.dtype, f"{what}: {y.dtype} vs {w.dtype}"
        yf, wf = (torch.view_as_real(y.contiguous()), torch.view_as_real(w)) if y.is_complex() else (y.contiguous(), w)
        it = torch.int32 if yf.dtype == torch.float32 else torch.int64
        yf = yf.view(reps, *wf.shape)
        same = (yf.view(it) == wf.view(it)) | (torch.isnan(yf) & torch.isnan(wf))
        if not bool(same.all().item()):
            _assert_equal_but_nan_payload(y.cpu().numpy(), np.tile(want, (reps, 1)), f"{what}: chunk {i}")
            raise AssertionError(f"{what}: chunk {i}: the device comparison found a difference the host comparison did not")


def _check_end_state(f, fos, reps, what):
    hist = np.asarray(f.history).reshape(len(fos) * reps, -1)
    want = np.tile(np.stack([np.asarray(fo.history) for fo in fos]), (reps, 1)).reshape(len(fos) * reps, -1)
    assert_bit_equal(hist, want, f"history: {what}")
    st, so = f.state, fos[0].state
    assert (st.phiIdx, st.inputDeficit) == (so.phiIdx, so.inputDeficit), what


def _upload(torch, x):
    return torch.from_numpy(x).pin_memory().cuda()          # a fresh allocation: the first call reads cold lines


def _run_case(pkg, O, torch, ratio, h, tx, rows, reps, sizes, numerics, what):
    """filt over the chunks against the oracle; returns the per-call output counts"""
    ref, fos = _oracle(O, h, ratio, tx, rows, sizes)
    xd = _upload(torch, np.tile(rows, (reps, 1)))
    f = pkg.FIRFilter(h, ratio, numerics=numerics)
    try:
        cuts, ys, counts = _cuts(sizes), [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            y = f.filt(xd[:, a:b])
            ys.append(y)
            counts.append(int(y.shape[-1]))
            if b > a and y.shape[-1] > 0:
                assert f.last_kernel_name() == OPAIR, (what, f.last_kernel_name())
        _check_outputs(torch, ys, ref, reps, what)
        _check_end_state(f, fos, reps, what)
    finally:
        f.close()
    return counts


def _sweep(pkg, O, torch, tname, smin, taps, numerics, short):
    _, th, tx, _, _ = oc.TYPES[oc.TYPE_INDEX[tname]]
    rng = _rng(tname, smin, numerics)
    reached, failed = [], []
    for T in taps:
        what = f"{tname} SMIN={smin} T={T} numerics={numerics}"
        try:                                                 # (a mismatch does not end the sweep: every failing T is reported)
            ratio, h, rows, sizes = oc.many_case(rng, tname, smin, T)
            assert -(-len(h) // ratio.numerator) == T and ratio.denominator // ratio.numerator == smin
            assert np.count_nonzero(h) >= max(1, len(h) - 3), what
            what += f" {ratio} hLen={len(h)}"
            _run_case(pkg, O, torch, ratio, h, tx, rows, oc.MANY_CHANNELS // oc.MANY_ROWS, sizes, numerics, "many tiles: " + what)
            if short:
                ratio, h, rows, sizes = oc.short_case(rng, tname, smin, T)
                assert np.count_nonzero(h) >= max(1, len(h) - 3), what
                _run_case(pkg, O, torch, ratio, h, tx, rows, 1, sizes, numerics, "short: " + what)
        except AssertionError as e:
            failed.append(f"{what}: {e}")
            continue
        reached.append(T)
    assert not failed, "\n".join(failed)
    return reached


@pytest.mark.parametrize("tname,smin", oc.strict_params(), ids=lambda v: str(v))
def test_every_strict_instantiation(pkg, O, torch_cuda, tname, smin):
    """item 1: <T, false, NC, SMIN, TXS, R> for every T the plan accepts, both shapes"""
    reached = _sweep(pkg, O, torch_cuda, tname, smin, oc.strict_taps(tname, smin), pkg.NUMERICS_STRICT, short=True)
    _REACHED["strict"][(tname, smin)] = len(reached)
    assert len(reached) == oc.STRICT_COUNT[(tname, smin)], (tname, smin, reached)


@pytest.mark.parametrize("tname,smin", oc.fused_params(), ids=lambda v: str(v))
def test_every_fused_instantiation(pkg, O, torch_cuda, tname, smin):
    """item 2: <T, true, ...> for T = 4, 8, ... (SMIN <= 1) against the oracle's fused mode, the many-tiles shape"""
    O.set_fused(True)
    try:
        reached = _sweep(pkg, O, torch_cuda, tname, smin, oc.fused_taps(tname, smin), pkg.NUMERICS_FUSED, short=False)
    finally:
        O.set_fused(False)
    _REACHED["fused"][(tname, smin)] = len(reached)
    assert len(reached) == oc.FUSED_COUNT[(tname, smin)], (tname, smin, reached)


@pytest.mark.parametrize("tname,smin,T", oc.mode_params(), ids=lambda v: str(v))
def test_modes_of_24_and_32_taps(pkg, O, torch_cuda, tname, smin, T):
    """item 3: T in {24, 32}, SMIN <= 1 exist in four MODEs.  64 channels from 4 distinct rows, about 70 000 outputs per channel:
    MODE 3 (host-planned, n_out * nch just under 2^22: a first call of 65 400 outputs per channel, the rest behind it), MODE 1 (a
    host-planned call of n_out * nch >= 2^22), MODE 0 (MODE 1's calls planned on the device: filt_into_async) and MODE 2 (the
    resident ring: three unequal chunks, one shorter than the history), each bit-equal to the oracle's chunk loop."""
    torch = torch_cuda
    _, th, tx, _, _ = oc.TYPES[oc.TYPE_INDEX[tname]]
    rng = _rng("modes", tname, smin, T)
    ratio, h, rows, _ = oc.many_case(rng, tname, smin, T, n_out=70_000)
    L, M = ratio.numerator, ratio.denominator
    n = rows.shape[1]
    nch, reps = oc.MANY_CHANNELS, oc.MANY_CHANNELS // oc.MANY_ROWS
    what = f"{tname} SMIN={smin} T={T} {ratio} hLen={len(h)}"
    assert np.count_nonzero(h) >= len(h) - 3, what
    xd = _upload(torch, np.tile(rows, (reps, 1)))

    # MODE 3
    sizes = [65_400 * M // L, n - 65_400 * M // L]
    ref, fos = _oracle(O, h, ratio, tx, rows, sizes)
    cuts = _cuts(sizes)
    f = pkg.FIRFilter(h, ratio)
    try:
        ys = [f.filt(xd[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert 65_000 * nch <= ys[0].shape[-1] * nch < (1 << 22) and f.last_kernel_name() == OPAIR, (what, ys[0].shape)
        _check_outputs(torch, ys, ref, reps, "MODE 3: " + what)
        _check_end_state(f, fos, reps, "MODE 3: " + what)
    finally:
        f.close()
    _REACHED["mode3"].add((tname, smin, T))
    del ys

    # MODE 1 and MODE 0: the same two chunks, one reference
    sizes = [n - 1_500, 1_500]
    ref, fos = _oracle(O, h, ratio, tx, rows, sizes)
    cuts = _cuts(sizes)
    f = pkg.FIRFilter(h, ratio)
    try:
        ys = [f.filt(xd[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert ys[0].shape[-1] * nch >= (1 << 22) and f.last_kernel_name() == OPAIR, what
        _check_outputs(torch, ys, ref, reps, "MODE 1: " + what)
        _check_end_state(f, fos, reps, "MODE 1: " + what)
    finally:
        f.close()
    _REACHED["mode1"].add((tname, smin, T))
    del ys

    f = pkg.FIRFilter(h, ratio).bind(tx, nch)
    try:
        cnt = torch.zeros(len(sizes), dtype=torch.int64, device="cuda")
        ys = []
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            y = torch.empty((nch, f.outputlength_bound(b - a)), dtype=_tdtype(torch, f.output_dtype), device="cuda")
            f.filt_into_async(y, xd[:, a:b], cnt[i:i + 1])
            ys.append(y)
        last = f.sync_state()
        c = cnt.cpu().tolist()
        assert c == [len(r) for r in ref[0]] and last == c[-1] and f.last_kernel_name() == OPAIR, (what, c)
        _check_outputs(torch, [y[:, :k] for y, k in zip(ys, c)], ref, reps, "MODE 0: " + what)
        _check_end_state(f, fos, reps, "MODE 0: " + what)
    finally:
        f.close()
    _REACHED["mode0"].add((tname, smin, T))
    del ys

    # MODE 2: the ring
    sizes = [n // 3 + 7, T - 2, n - (n // 3 + 7) - (T - 2)]
    ref, fos = _oracle(O, h, ratio, tx, rows, sizes)
    cuts = _cuts(sizes)
    f = pkg.FIRFilter(h, ratio).bind(tx, nch)
    try:
        ys = [torch.zeros((nch, max(f.outputlength_bound(s), 1)), dtype=_tdtype(torch, f.output_dtype), device="cuda") for s in sizes]
        torch.cuda.synchronize()                            # x and the buffers are complete: the resident kernel is behind no stream
        with f.open_ring() as ring:
            assert ring.info()["resident"], what
            counts = [ring.push(y, xd[:, a:b])[0] for y, a, b in zip(ys, cuts[:-1], cuts[1:])]
            ring.drain()
        assert counts == [len(r) for r in ref[0]], (what, counts)
        _check_outputs(torch, [y[:, :k] for y, k in zip(ys, counts)], ref, reps, "MODE 2: " + what)
        _check_end_state(f, fos, reps, "MODE 2: " + what)
    finally:
        f.close()
    _REACHED["mode2"].add((tname, smin, T))


_LINE = re.compile(r"\[mrhip\] rational_opair T=(\d+) smin=(\d+) .* grid=(\d+) block=(\d+) .* c=(\d+) P=(\d+) cM=(\d+) J=(\d+) ns=(\d+)")


def test_many_tiles_shape_takes_dynamic_grabs():
    """item 4, the sweep's own premise: in the many-tiles shape workgroups take several tiles each, by dynamic grabs (pair_grid, host_logic.cpp:
    static_grabs is false when tiles > 3 x grid), and the short shape has at least two tiles per channel.  The geometry cannot be
    seen from Python, so a child process (a fresh interpreter with MRHIP_DEBUG=1: the library then prints one line per instantiation,
    at its first launch) issues, for every (type, SMIN) and one T per ratio of the table, the many-tiles shape's large chunk and
    the short shape's first call; the parent checks the bound on what the library printed, and that opair_cases.plan -- which sizes
    the short shape -- tiles the calls as the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MRHIP_DEBUG="1")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "opair_cases.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-800:], p.stderr[-800:])
    lines = p.stderr.splitlines()
    seen = 0
    for i, ln in enumerate(lines):
        if not ln.startswith("CASE "):
            continue
        kind, tname, smin, T, n_out, nch, mP, mJ = ln.split()[1:9]
        smin, T, n_out, nch, mP, mJ = (int(v) for v in (smin, T, n_out, nch, mP, mJ))
        m = _LINE.match(lines[i + 1]) if i + 1 < len(lines) else None
        assert m, f"no launch line behind {ln!r}: {lines[i + 1:i + 2]}"
        gT, gs, grid, _, _, P, _, J, _ = (int(v) for v in m.groups())
        assert (gT, gs) == (T, smin), (ln, lines[i + 1])
        print(f"{kind} {tname} SMIN={smin} T={T}: n_out={n_out} nch={nch} grid={grid} P={P} J={J} tiles={math.ceil(n_out / (J * P)) * nch}")
        assert (P, J) == (mP, mJ), f"opair_cases.plan and the library disagree: {ln} / {lines[i + 1]}"
        if kind == "many":
            assert math.ceil(n_out / (J * P)) * nch > 3 * grid, (ln, lines[i + 1])
        else:
            assert math.ceil(n_out / (J * P)) >= 2, (ln, lines[i + 1])
        seen += 1
    # per (type, SMIN): one T per ratio of the table, in both shapes
    assert seen == 2 * sum(len(oc.RATIOS[s]) for _, s in oc.strict_params()), seen


def test_strict_total_is_832():
    """2 x 6 + 4 x 2 = 20 parameters (type x SMIN); their rows of the table sum to 832"""
    assert len(_REACHED["strict"]) == 20 and sum(_REACHED["strict"].values()) == oc.STRICT_TOTAL == 832, _REACHED["strict"]


def test_fused_total_is_144():
    assert len(_REACHED["fused"]) == 12 and sum(_REACHED["fused"].values()) == oc.FUSED_TOTAL == 144, _REACHED["fused"]


def test_each_mode_of_24_and_32_taps_covers_24():
    assert [len(_REACHED[m]) for m in ("mode0", "mode1", "mode2", "mode3")] == [oc.MODE_TOTAL] * 4 == [24] * 4, {m: len(_REACHED[m]) for m in _REACHED if m.startswith("mode")}
