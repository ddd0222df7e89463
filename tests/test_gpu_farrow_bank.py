"""GPU tests of per-channel taps for FIRFarrow (csrc/kernels_bank_farrow.hip): FIRFilter.per_channel_farrow(H, rate, Nphi, polyorder),
one FIRFilter(H[c], rate, Nphi, polyorder) per channel behind one filter object (mrhip_create_farrow_bank).

Bar (include/multirate_hip.h, "Per-channel taps for FIRFarrow"): for every channel c the outputs, the per-call counts, the end state
and the history are BIT FOR BIT those of the oracle's FIRFilter(H[c], rate, Nphi, polyorder = P) fed x[c] -- on
farrow_bank_generic_kernel (MRHIP_FORCE_GENERIC=1) and on farrow_bank_tiled_kernel (MRHIP_FARROW_BANK_TILED=1), whole and chunked (a
one-sample chunk, an empty one, chunks shorter than the history), STRICT and FUSED, host-scheduled, split, device-planned, captured and
chained.  No tolerance anywhere.

The polynomial fit.  The reference pins no bits of polyfit (Julia: A \\ y, LAPACK), and the oracle says so (oracle.polyfit: "the fit is
done ONCE on the caller's side and the same coefficients are handed to oracle and GPU"): its numpy QR and the library's Householder QR
(polyfit_rows, the per-row fit mrhip_create_farrow and mrhip_create_farrow_bank both make) agree to rounding, not bit for bit -- of the
342 rows of this file's banks, 132 differ in some coefficient's last bits (7 of 171 with Float32 taps, 125 of 171 with Float64 taps).
The bank constructor takes no caller-fitted pnfb, so the oracle is handed the library's fit of row c (`_fit`: mrhip_polyfit per row of
taps2pfb(H[c], Nphi), rounded to the tap type -- what every other FIRFarrow test of this suite does), and the fit itself is checked on
its own: the bank's pnfb is bit for bit that per-row fit and the one-channel filter's pnfb, and agrees with the oracle's pfb2pnfb
within the bound tests/test_oracle.py already holds the two fits to.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NCH = 3
RATES = [0.47, 1.0, 2.123, 32.0 / 3]
# (Nphi, hLen, polyorder): T = 1 (no history), 8 (zero-padded rows), 8, 32, and a constant polynomial
BANKS = [(4, 4, 2), (4, 30, 3), (32, 250, 4), (32, 1024, 4), (32, 250, 0)]
X_LENS = [1, 5, 257, 1500]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
ALL_TYPES = [(th, tx) for th in (np.float32, np.float64) for tx in (np.float32, np.float64, np.complex64, np.complex128)]
FEW_TYPES = [(np.float32, np.float32), (np.float64, np.complex64)]
CASES = [((32, 250, 4), t) for t in ALL_TYPES] + [(b, t) for b in BANKS if b != (32, 250, 4) for t in FEW_TYPES]
GENERIC, TILED = "farrow_bank_generic_kernel", "farrow_bank_tiled_kernel"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _chunks(n, how):
    if how is None:
        return [(0, n)]
    if isinstance(how, int):
        return [(a, min(a + how, n)) for a in range(0, n, how)]
    out, pos = [], 0
    for c in how:
        if pos + c > n:
            break
        out.append((pos, pos + c))
        pos += c
    out.append((pos, n))
    return out


_SIGNALS = {}


def _signal(seed, hLen, x_len, th, tx, nch=NCH):
    """rows that tell channels apart: row 0 random, row 1 a single 1 at tap 0, row 2 = row 0 reversed and negated; further rows
    random.  A swapped or a shared bank fails every case."""
    key = (seed, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, nch)
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        H = (rng.standard_normal((nch, hLen)) / hLen).astype(th)
        if nch > 1:
            H[1] = 0
            H[1, 0] = 1
        if nch > 2:
            H[2] = -H[0][::-1]
        x = rng.random((nch, x_len)) - 0.5
        if np.dtype(tx).kind == "c":
            x = x + 1j * (rng.random((nch, x_len)) - 0.5)
        x = x.astype(tx)
        H.setflags(write=False), x.setflags(write=False)
        _SIGNALS[key] = (H, x)
    return _SIGNALS[key]


_FITS = {}


def _fit(pkg, O, h, Nphi, P):
    """pfb2pnfb (src/Filters.jl:311-321) with the library's per-row fit: one polynomial per row of taps2pfb(h, Nphi), ascending powers,
    stored in the tap type (values representable in it, held as Float64).  Computed once per tap vector."""
    key = (h.tobytes(), h.dtype.name, Nphi, P)
    if key not in _FITS:
        pfb = O.taps2pfb(h, Nphi)
        _FITS[key] = np.stack([pkg.polyfit(pfb[i].astype(np.float64), P).astype(h.dtype).astype(np.float64) for i in range(pfb.shape[0])])
    return _FITS[key]


def _oracle(pkg, O, h, rate, Nphi, P, tx):
    """the reference of one channel: the oracle's FIRFilter(h, rate, Nphi, polyorder = P) on the library's fit of h"""
    return O.FIRFilter(h, rate, Nphi, tx=tx, polyorder=P, pnfb=_fit(pkg, O, h, Nphi, P))


def _state3(st):
    return (st.inputDeficit, st.phiAccumulator, st.phiIdx)


_REFS = {}


def _reference(pkg, O, seed, rate, Nphi, hLen, P, x_len, th, tx, how, nch=NCH, fused=False, mod_form=False):
    """the oracle per channel, one O.FIRFilter(H[c], rate, Nphi, polyorder = P) fed x[c] in the pieces of `how`: (outputs [c][piece],
    (inputDeficit, phiAccumulator, phiIdx), histories [c]); computed once per case and shared"""
    key = (seed, rate, Nphi, hLen, P, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), nch, fused, mod_form)
    if key not in _REFS:
        H, x = _signal(seed, hLen, x_len, th, tx, nch)
        O.set_fused(fused)
        O.set_mod_form(mod_form)
        try:
            refs = [_oracle(pkg, O, H[c], rate, Nphi, P, tx) for c in range(nch)]
            outs = [[r.filt(x[c, a:b]) for a, b in _chunks(x_len, how)] for c, r in enumerate(refs)]
        finally:
            O.set_fused(False)
            O.set_mod_form(False)
        for i in range(len(outs[0])):
            assert len({len(o[i]) for o in outs}) == 1            # (the per-call counts do not depend on the taps)
        states = {_state3(r.state) for r in refs}
        assert len(states) == 1                                   # (nor does the state)
        _REFS[key] = (outs, states.pop(), [r.history for r in refs])
    return _REFS[key]


def _filter(pkg, monkeypatch, H, rate, Nphi, P, tx, tiled, fused=False, grid=None):
    """a bound bank filter on the universal kernel (MRHIP_FORCE_GENERIC is read when the device object is created) or on the tiled
    kernel wherever its plan fits (MRHIP_FARROW_BANK_TILED=1)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if tiled else "1")
    monkeypatch.setenv("MRHIP_FARROW_BANK_TILED", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_FARROW_BANK_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_FARROW_BANK_GRID", str(grid))
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    return pkg.FIRFilter.per_channel_farrow(H, rate, Nphi, P, numerics=numerics).bind(tx, H.shape[0])


def _run_case(pkg, O, monkeypatch, rate, Nphi, hLen, P, x_len, th, tx, fused=False, nch=NCH, grid=None, chunkings=CHUNKINGS, mod_form=False):
    seed = 1000 * Nphi + hLen + x_len
    H, x = _signal(seed, hLen, x_len, th, tx, nch)
    want_dtype = np.result_type(th, tx)
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        want, state, hists = _reference(pkg, O, seed, rate, Nphi, hLen, P, x_len, th, tx, how, nch, fused, mod_form)
        assert want[0][0].dtype == want_dtype
        for tiled in (False, True):
            what = f"rate {rate} Nphi {Nphi} hLen {hLen} P {P} x_len {x_len} {name} tiled={tiled}"
            f = _filter(pkg, monkeypatch, H, rate, Nphi, P, tx, tiled, fused, grid)
            if mod_form:
                f.set_mod_form(True)
            assert f.output_dtype == want_dtype
            for i, (a, b) in enumerate(pieces):
                y = f.filt(np.ascontiguousarray(x[:, a:b])).reshape(nch, -1)
                assert y.dtype == want_dtype and y.shape == (nch, len(want[0][i])), (what, a, b, y.shape)   # the per-call count
                for c in range(nch):
                    assert_bit_equal(y[c], want[c][i], f"{what} chunk [{a}, {b}) channel {c}")
                if y.shape[1] > 0:
                    assert f.last_kernel_name() == (TILED if tiled else GENERIC), what
            st = f.state
            assert st.kind == 5 and st.nchannels == nch
            assert _state3(st) == state, what
            hist = f.history.reshape(nch, -1)
            assert hist.dtype == np.dtype(tx)
            for c in range(nch):
                assert_bit_equal(hist[c], hists[c], f"{what} history {c}")
            f.close()


# ---- 1. shape sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("bank,types", CASES, ids=lambda v: "-".join(np.dtype(t).name for t in v) if isinstance(v[0], type) else "x".join(map(str, v)))
def test_shape_sweep_both_kernels_equal_the_oracle_per_channel(pkg, O, monkeypatch, bank, types, rate):
    for x_len in X_LENS:
        _run_case(pkg, O, monkeypatch, rate, *bank, x_len, *types)


# ---- 2. FUSED ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.47, 2.123])
@pytest.mark.parametrize("th,tx", [(np.float32, np.float32), (np.float64, np.complex128)], ids=lambda t: np.dtype(t).name)
def test_fused_equals_the_fused_oracle(pkg, O, monkeypatch, th, tx, rate):
    for x_len in (257, 1500):
        _run_case(pkg, O, monkeypatch, rate, 32, 250, 4, x_len, th, tx, fused=True)


# ---- 3. the seam -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,plus", [(0.47, 2), (2.123, 7)])
def test_seam_outputs_start_from_plus_zero(pkg, O, monkeypatch, rate, plus):
    """negative constant rows, x = 0: every product is -0.0, and so is every sum of them -- except on the seam (the outputs whose
    window still reaches into the history of a call: n < tapsPerPhi), which start from +0.0 (support.jl:46): 0 + (-0) = +0.  The first
    `plus` outputs of EACH call are +0.0, the rest -0.0; both kernels must match the sign."""
    Nphi, T, P, x_len = 32, 4, 4, 40
    H = -np.outer(np.arange(1, NCH + 1), np.ones(Nphi * T)).astype(np.float32)
    x = np.zeros((NCH, x_len), dtype=np.float32)
    refs = [_oracle(pkg, O, H[c], rate, Nphi, P, np.float32) for c in range(NCH)]
    want = [np.stack([r.filt(x[c]) for c, r in enumerate(refs)]) for _ in range(2)]
    for w in want:
        sign = np.signbit(w)
        assert not w.any() and not sign[:, :plus].any() and sign[:, plus:].all() and w.shape[1] > plus     # (the case is not vacuous)
    for tiled in (False, True):
        f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32, tiled)
        for i in range(2):
            y = f.filt(x)
            assert f.last_kernel_name() == (TILED if tiled else GENERIC)
            assert np.array_equal(y.view(np.uint32), want[i].view(np.uint32)), f"signs of zero, call {i}, tiled={tiled}"
        f.close()


# ---- 4. known answer without the oracle --------------------------------------------------------------------------------------
def test_known_answer_running_sums_scaled_per_channel(pkg, monkeypatch):
    """H[c] = (c + 1) * ones(Nphi * T), x = ones: every row of pfb_c is constant, its fitted polynomial is c + 1 plus higher
    coefficients of about 1e-16 that vanish when the tap is rounded to Float32, so every tap is c + 1 and an output is (c + 1) times
    the number of ones in its window: y_c[k] = (c + 1) * min(n_k, T).  Rate 1.0: every sample gives an output, n_k = k.  Rate 0.5:
    every second sample (1, 3, 5, ...) gives one, n_k = 2k - 1."""
    Nphi, T, P = 32, 4, 4
    H = np.outer(np.arange(1, NCH + 1), np.ones(Nphi * T)).astype(np.float32)
    x = np.ones((NCH, 10), dtype=np.float32)
    k = np.arange(1, 11)
    scale = np.arange(1, NCH + 1, dtype=np.float32)[:, None]
    for tiled in (False, True):
        for rate, arrived in ((1.0, k), (0.5, 2 * k[:5] - 1)):
            f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32, tiled)
            y = f.filt(x)
            assert y.dtype == np.float32
            assert np.array_equal(y, scale * np.minimum(arrived, T).astype(np.float32)), (tiled, rate, y)
            assert np.array_equal(y[:, -1], 4 * scale[:, 0])
            f.close()


# ---- 5. tiles and workgroups -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 3, 7, 64])
def test_workgroups_whose_runs_cross_channel_boundaries(pkg, O, monkeypatch, grid):
    """3 channels x 1500 outputs = 3 x 6 tiles: one workgroup walks every channel (1), runs that cross a channel in mid-run (2, 7;
    3: none does), more workgroups than the 18 tiles (64: idle ones)"""
    x_len = 707                                                        # ceil-ish 707 * 2.123 = 1500 outputs
    _run_case(pkg, O, monkeypatch, 2.123, 32, 250, 4, x_len, np.float32, np.float32, grid=grid, chunkings={"whole": None})
    want, _, _ = _reference(pkg, O, 1000 * 32 + 250 + x_len, 2.123, 32, 250, 4, x_len, np.float32, np.float32, None)
    assert 1500 <= len(want[0][0]) <= 1502


@pytest.mark.parametrize("nch", [1, 2, 33])
def test_channel_counts_at_the_default_grid(pkg, O, monkeypatch, nch):
    _run_case(pkg, O, monkeypatch, 2.123, 32, 250, 4, 707, np.float32, np.float32, nch=nch, chunkings={"whole": None})


def test_over_span_tiles_read_global_memory_and_equal_the_universal_kernel_and_the_oracle(pkg, O, monkeypatch):
    """rate 1/50: a full tile of 256 outputs runs over 12 750 samples, more than the 40 KiB of samples the plan gives a tile
    (10 240 Float32 samples): the three full tiles read their windows from global memory, the last (32 outputs) is staged"""
    rate, Nphi, hLen, P, x_len, nch = 1.0 / 50, 32, 250, 4, 40_000, 2
    H, x = _signal(7, hLen, x_len, np.float32, np.float32, nch)
    want, state, hists = _reference(pkg, O, 7, rate, Nphi, hLen, P, x_len, np.float32, np.float32, None, nch)
    ys = {}
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32, tiled)
        ys[tiled] = f.filt(x)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert _state3(f.state) == state
        assert_bit_equal(f.history, np.stack(hists), f"history, tiled={tiled}")
        f.close()
    assert ys[True].shape == (nch, 800)
    assert_bit_equal(ys[True], ys[False], "tiled == universal")
    assert_bit_equal(ys[True], np.stack([w[0] for w in want]), "tiled == oracle")


def test_the_default_rule_and_the_switch(pkg, O, monkeypatch):
    """MRHIP_FARROW_BANK_TILED unset: the measured rule -- the tiled kernel won nowhere and stays behind its
    switch, so the call takes the universal kernel; MRHIP_FARROW_BANK_TILED=0: the same, even with MRHIP_FORCE_GENERIC=0.  The outputs
    are the oracle's either way."""
    rate, Nphi, hLen, P, x_len = 2.123, 32, 250, 4, 707
    seed = 1000 * Nphi + hLen + x_len
    H, x = _signal(seed, hLen, x_len, np.float32, np.float32)
    want, state, _ = _reference(pkg, O, seed, rate, Nphi, hLen, P, x_len, np.float32, np.float32, None)
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.delenv("MRHIP_FARROW_BANK_GRID", raising=False)
    for mode in (None, "0"):
        if mode is None:
            monkeypatch.delenv("MRHIP_FARROW_BANK_TILED", raising=False)
        else:
            monkeypatch.setenv("MRHIP_FARROW_BANK_TILED", mode)
        f = pkg.FIRFilter.per_channel_farrow(H, rate, Nphi, P).bind(np.float32, NCH)
        y = f.filt(x)
        assert f.last_kernel_name() == GENERIC, mode
        assert_bit_equal(y, np.stack([w[0] for w in want]), f"MRHIP_FARROW_BANK_TILED={mode}")
        assert _state3(f.state) == state
        f.close()


# ---- 6. call paths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=lambda t: np.dtype(t).name)
def test_split_call_places_every_piece_and_leaves_the_right_history(pkg, O, monkeypatch, torch_cuda, tx):
    """MRHIP_LAUNCH_MAX=4099: a piece per 4099 outputs, each written at its own offset of y; the continuation pieces have no seam"""
    torch = torch_cuda
    rate, Nphi, hLen, P, x_len, nch = 1.37, 32, 250, 4, 30_011, 2
    H, x = _signal(9, hLen, x_len, np.float32, tx, nch)
    want, state, hists = _reference(pkg, O, 9, rate, Nphi, hLen, P, x_len, np.float32, tx, None, nch)
    xd = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setenv("MRHIP_LAUNCH_MAX", "4099")
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, H, rate, Nphi, P, tx, tiled)
        y = f.filt(xd).cpu().numpy()
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert_bit_equal(y, np.stack([w[0] for w in want]), f"split call, tiled={tiled}")
        assert _state3(f.state) == state
        assert_bit_equal(f.history, np.stack(hists), "history")
        assert_bit_equal(f.history[1], x[1, -f.historyLen:], "history == the last samples")
        f.close()


def test_host_scheduled_calls_under_the_older_mod_form(pkg, O, monkeypatch):
    """set_mod_form(True) with an Nphi that is no power of two: the schedule is evaluated on the host"""
    _run_case(pkg, O, monkeypatch, 0.47, 6, 30, 3, 1500, np.float32, np.float32, chunkings={"whole": None, "prime": 97}, mod_form=True)
    _run_case(pkg, O, monkeypatch, 0.47, 6, 30, 3, 257, np.float32, np.complex64, chunkings={"ragged": [1, 0, 7, 2]}, mod_form=True)


def _oracle_stream(pkg, O, H, rate, Nphi, P, x, chunk, n):
    refs = [_oracle(pkg, O, H[c], rate, Nphi, P, x.dtype) for c in range(H.shape[0])]
    out = [np.stack([r.filt(x[c, i * chunk:(i + 1) * chunk]) for c, r in enumerate(refs)]) for i in range(n)]
    return out, _state3(refs[0].state), np.stack([r.history for r in refs])


@pytest.mark.parametrize("tiled", [False, True])
def test_async_calls_equal_the_synchronous_stream(pkg, O, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, P, chunk, n = 2.123, 32, 250, 4, 96, 5
    H, x = _signal(21, hLen, chunk * n, np.float32, np.complex64)
    want, state, hist = _oracle_stream(pkg, O, H, rate, Nphi, P, x, chunk, n)
    sync = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.complex64, tiled)
    for i in range(n):
        assert_bit_equal(sync.filt(np.ascontiguousarray(x[:, i * chunk:(i + 1) * chunk])), want[i], f"synchronous call {i}")
    sync.close()
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.complex64, tiled)
    xd = torch.from_numpy(np.array(x)).cuda()
    bound = f.outputlength_bound(chunk)
    ys = torch.zeros((n, NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i in range(n):
        f.filt_into_async(ys[i], xd[:, i * chunk:(i + 1) * chunk], cnt[i:i + 1])
    last = f.sync_state()
    assert f.last_kernel_name() == (TILED if tiled else GENERIC)      # both kernels take the count from the call record
    counts = cnt.cpu().tolist()
    assert counts == [w.shape[1] for w in want] and last == counts[-1]
    for i in range(n):
        assert_bit_equal(ys[i, :, :counts[i]].cpu().numpy(), want[i], f"asynchronous call {i}")
    assert _state3(f.state) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


@pytest.mark.parametrize("tiled", [False, True])
def test_captured_call_replayed_three_times_equals_the_synchronous_stream(pkg, O, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, P, chunk, n = 2.123, 32, 250, 4, 96, 5            # chunk >= historyLen (7)
    H, x = _signal(22, hLen, chunk * n, np.float32, np.float32)
    want, state, hist = _oracle_stream(pkg, O, H, rate, Nphi, P, x, chunk, n)
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32, tiled)
    xd = torch.from_numpy(np.array(x)).cuda()
    # The stream starts with a plain call and an asynchronous one of the captured size: the schedule's work buffers are allocated
    # by the first device-planned call of a size (allocations cannot be captured).  The graph takes the stream over from there.
    assert_bit_equal(f.filt(xd[:, :chunk].contiguous()).cpu().numpy(), want[0], "plain call")
    bound = f.outputlength_bound(chunk)
    y1 = torch.zeros((NCH, bound), dtype=torch.float32, device="cuda")
    f.filt_into_async(y1, xd[:, chunk:2 * chunk])
    c1 = f.sync_state()
    assert_bit_equal(y1[:, :c1].cpu().numpy(), want[1], "asynchronous call of the captured size")
    xs = torch.zeros((NCH, chunk), dtype=torch.float32, device="cuda")
    ys = torch.zeros((NCH, bound), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        f.filt_into_async(ys, xs, cnt)
    for i in range(2, n):
        xs.copy_(xd[:, i * chunk:(i + 1) * chunk])
        g.replay()
        torch.cuda.synchronize()
        c = int(cnt.cpu()[0])
        assert c == want[i].shape[1]
        assert_bit_equal(ys[:, :c].cpu().numpy(), want[i], f"replay {i}")
    f.sync_state()
    assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    assert _state3(f.state) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


@pytest.mark.parametrize("tiled", [False, True])
def test_chained_call_behind_a_decimator(pkg, O, monkeypatch, torch_cuda, tiled):
    """filt_into_async(..., after=prev): the input length of the bank filter's call is the decimator's count, on the device"""
    torch = torch_cuda
    rate, Nphi, hLen, P = 2.123, 32, 250, 4
    sizes = [1001, 17, 2000]
    H, x = _signal(23, hLen, sum(sizes), np.float32, np.float32)
    h1 = np.random.default_rng(24).standard_normal(16).astype(np.float32)
    f1 = pkg.FIRFilter(h1, Fraction(1, 4)).bind(np.float32, NCH)
    f2 = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32, tiled)
    o1 = [O.FIRFilter(h1, Fraction(1, 4), tx=np.float32) for _ in range(NCH)]
    o2 = [_oracle(pkg, O, H[c], rate, Nphi, P, np.float32) for c in range(NCH)]
    xd = torch.from_numpy(np.array(x)).cuda()
    mid = torch.zeros((NCH, f1.outputlength_bound(max(sizes))), dtype=torch.float32, device="cuda")
    outs = [torch.zeros((NCH, f2.outputlength_bound(f1.outputlength_bound(s))), dtype=torch.float32, device="cuda") for s in sizes]
    cnt = torch.zeros(len(sizes), dtype=torch.int64, device="cuda")
    pos = 0
    for i, s in enumerate(sizes):
        b1 = f1.outputlength_bound(s)
        f1.filt_into_async(mid[:, :b1], xd[:, pos:pos + s])
        f2.filt_into_async(outs[i], mid[:, :b1], cnt[i:i + 1], after=f1)
        pos += s
    torch.cuda.synchronize()
    assert f2.last_kernel_name() == (TILED if tiled else GENERIC)
    counts = cnt.cpu().tolist()
    pos = 0
    for i, s in enumerate(sizes):
        for c in range(NCH):
            ref = o2[c].filt(o1[c].filt(x[c, pos:pos + s]))
            assert counts[i] == len(ref), (i, c, counts[i], len(ref))
            assert_bit_equal(outs[i][c, :counts[i]].cpu().numpy(), ref, f"chained call {i} channel {c}")
        pos += s
    f2.sync_state()
    assert _state3(f2.state) == _state3(o2[0].state)
    assert_bit_equal(f2.history, np.stack([r.history for r in o2]), "history after the chained calls")
    f1.close(), f2.close()


# ---- 7. accessors and errors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
def test_pnfb_tapsforphase_and_reset(pkg, O, monkeypatch, th):
    rate, Nphi, hLen, P, x_len = 0.47, 4, 30, 3, 300
    H, x = _signal(31, hLen, x_len, th, np.float32)
    refs = [_oracle(pkg, O, H[c], rate, Nphi, P, np.float32) for c in range(NCH)]
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32, tiled=True)
    pn = f.pnfb()
    assert pn.shape == (NCH, f.tapsPerPhi, P + 1) and pn.dtype == np.float64
    ones = [pkg.FIRFilter(H[c], rate, Nphi, P).bind(np.float32, 1) for c in range(NCH)]
    A = np.vander(np.arange(1.0, Nphi + 1.0), P + 1, increasing=True)
    eps = float(np.finfo(th).eps)
    for c in range(NCH):
        assert_bit_equal(pn[c], _fit(pkg, O, np.array(H[c]), Nphi, P), f"pnfb of channel {c} == the per-row fit of row {c}")
        assert_bit_equal(pn[c], ones[c].pnfb(), f"pnfb of channel {c} == the one-channel filter's")
        # the oracle's pfb2pnfb, row by row: two backward-stable Float64 QR fits of one row agree in their FITTED VALUES to
        # 1e-6 max|row| (the bound of tests/test_oracle.py), and each coefficient c_j was then rounded to the tap type once on either
        # side: at most eps |c_j| x^j more per term, x <= Nphi
        theirs, pfb = O.pfb2pnfb(O.taps2pfb(np.array(H[c]), Nphi), P), O.taps2pfb(np.array(H[c]), Nphi)
        for i in range(f.tapsPerPhi):
            bound = 1e-6 * np.abs(pfb[i]).max() + eps * (np.abs(A) @ (np.abs(pn[c, i]) + np.abs(theirs[i]))).max()
            assert np.abs(A @ pn[c, i] - A @ theirs[i]).max() <= bound, (c, i)
    for phase in (0.0, 1.0, 1.25, Nphi + 0.5, Nphi + 1.0):
        t = f.tapsforphase(phase)
        assert t.shape == (NCH, f.tapsPerPhi) and t.dtype == np.dtype(th)
        for c in range(NCH):
            assert_bit_equal(t[c], ones[c].tapsforphase(phase), f"tapsforphase({phase}) of channel {c}")
    for bad in (-0.5, Nphi + 1.5):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.tapsforphase(bad)
        assert e.value.code == 1
    want = np.stack([r.filt(x[c]) for c, r in enumerate(refs)])
    assert_bit_equal(f.filt(x), want, "first run")
    f.reset()
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == (1, 1.0) and not f.history.any()
    assert_bit_equal(f.filt(x), want, "reset, then the same again")
    f.close()
    for o in ones:
        o.close()


def test_buffer_too_small_wrong_channel_count_and_the_c_abi_errors(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    lib = pkg.load_library()
    F32, F64, C64, C128 = 0, 1, 2, 3
    H, x = _signal(33, 8, 100, np.float32, np.float32)
    f = _filter(pkg, monkeypatch, H, 1.5, 4, 2, np.float32, tiled=True)
    xd = torch.from_numpy(np.array(x)).cuda()
    small = torch.zeros((NCH, 10), dtype=torch.float32, device="cuda")
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.filt_into(small, xd)                                          # buffer too small: the state stays
    assert e.value.code == 2
    assert (f.state.inputDeficit, f.state.phiAccumulator) == (1, 1.0) and not f.history.any()
    want = np.stack([_oracle(pkg, O, H[c], 1.5, 4, 2, np.float32).filt(x[c]) for c in range(NCH)])
    assert_bit_equal(f.filt(xd).cpu().numpy(), want, "the same call with room")
    f.close()
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_farrow(H, 1.5, 4, 2).bind(np.float32, NCH + 1)
    assert e.value.code == 1
    out = C.c_void_p()
    for th, hh in ((C64, np.array(H).astype(np.complex64)), (C128, np.array(H).astype(np.complex128))):
        rc = lib.mrhip_create_farrow_bank(hh.ctypes.data_as(C.c_void_p), H.shape[1], th, 1.5, 4, 2, F32, NCH, 0, C.byref(out))
        assert rc == 5 and not out.value
        assert "left out" in lib.mrhip_last_error().decode()
    hh = np.array(H)
    for P in (4, 5, 33, -1):                                            # polyorder >= Nphi, > 32, < 0
        assert lib.mrhip_create_farrow_bank(hh.ctypes.data_as(C.c_void_p), H.shape[1], F32, 1.5, 4, P, F32, NCH, 0, C.byref(out)) == 1
        assert not out.value
    for rate in (0.0, -1.0):
        assert lib.mrhip_create_farrow_bank(hh.ctypes.data_as(C.c_void_p), H.shape[1], F32, rate, 4, 2, F32, NCH, 0, C.byref(out)) == 1
        assert not out.value
    assert lib.mrhip_create_farrow_bank(hh.ctypes.data_as(C.c_void_p), H.shape[1], F32, 1.5, 0, 0, F32, NCH, 0, C.byref(out)) == 1   # bad Nphi
    assert lib.mrhip_create_farrow_bank(None, H.shape[1], F32, 1.5, 4, 2, F32, NCH, 0, C.byref(out)) == 1 and not out.value


def test_equal_rows_equal_the_shared_taps_filter(pkg, monkeypatch):
    rate, Nphi, hLen, P, x_len = 2.123, 32, 250, 4, 1500
    H, x = _signal(51, hLen, x_len, np.float32, np.float32)
    same = np.ascontiguousarray(np.broadcast_to(H[0], (NCH, hLen)))
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    shared = pkg.FIRFilter(H[0], rate, Nphi, P)                    # mrhip_create_farrow: one h for every channel, as before
    want = shared.filt(np.array(x))
    assert "bank" not in shared.last_kernel_name()
    ss = shared.state
    for tiled in (False, True):
        b = _filter(pkg, monkeypatch, same, rate, Nphi, P, np.float32, tiled)
        assert_bit_equal(b.filt(np.array(x)), want, f"equal rows == the shared-taps filter, tiled={tiled}")
        assert_bit_equal(b.history, shared.history, "history")
        st = b.state
        assert _state3(st) + (st.xIdx,) == _state3(ss) + (ss.xIdx,)
        b.close()
    shared.close()


# ---- 8. unchanged predicates -------------------------------------------------------------------------------------------------
def test_cascade_takes_such_a_stage_through_the_per_stage_calls(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    H, x = _signal(41, 250, 3000, np.float32, np.float32)
    h2 = np.random.default_rng(42).standard_normal(16).astype(np.float32)
    xd = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.setenv("MRHIP_FARROW_BANK_TILED", "1")
    a, b = pkg.FIRFilter.per_channel_farrow(H, 2.123, 32, 4), pkg.FIRFilter(h2, Fraction(1, 2))
    by_hand = b.filt(a.filt(xd))
    cas = pkg.FilterCascade(pkg.FIRFilter.per_channel_farrow(H, 2.123, 32, 4), pkg.FIRFilter(h2, Fraction(1, 2)))
    y = cas.filt(xd)
    assert cas.stages[0].last_kernel_name() == TILED
    assert_bit_equal(y.cpu().numpy(), by_hand.cpu().numpy(), "cascade == by hand")
    cas.close(), a.close(), b.close()


def test_filt_multi_with_such_a_filter_equals_the_single_calls(pkg, O, monkeypatch, torch_cuda):
    torch = torch_cuda
    rate, Nphi, hLen, P, x_len = 2.123, 32, 250, 4, 400
    H, x = _signal(43, hLen, x_len, np.float32, np.float32)
    want = np.stack([_oracle(pkg, O, H[c], rate, Nphi, P, np.float32).filt(x[c]) for c in range(NCH)])
    bank = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32, tiled=True)
    plain = pkg.FIRFilter(H[0], rate, Nphi, P)
    xd = torch.from_numpy(np.array(x)).cuda()
    ys = pkg.filt_multi([bank, plain], [xd, xd[0].contiguous()])
    assert_bit_equal(ys[0].cpu().numpy(), want, "the bank filter's stream")
    assert_bit_equal(ys[1].cpu().numpy(), want[0], "the other stream")
    assert bank.last_kernel_name() == TILED
    bank.close(), plain.close()


def test_ring_is_not_resident(pkg, monkeypatch):
    H, _ = _signal(44, 250, 8, np.float32, np.float32)
    f = _filter(pkg, monkeypatch, H, 2.123, 32, 4, np.float32, tiled=True)
    with f.open_ring() as ring:
        assert ring.info()["resident"] is False
    f.close()
