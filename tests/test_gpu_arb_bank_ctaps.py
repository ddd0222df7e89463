"""GPU tests of per-channel complex taps for FIRArbitrary (csrc/kernels_bank_arb_ctaps.hip):
FIRFilter.per_channel_complex_taps_arbitrary(H, rate, Nphi), one FIRFilter(H[c]::Vector{Complex}, rate, Nphi) per channel behind one
filter object (mrhip_create_arbitrary_bank_ctaps).

Bar (include/multirate_hip.h, "Per-channel complex taps for FIRArbitrary"): for every channel c the outputs, the per-call counts, the
end state and the history are BIT FOR BIT those of the one-channel complex-tap FIRArbitrary filter of H[c] fed x[c] -- on
arb_bank_ctaps_generic_kernel (MRHIP_FORCE_GENERIC=1) and on arb_bank_ctaps_tiled_kernel (MRHIP_ARB_BANK_CTAPS_TILED=1).  That
one-channel filter is given three ways: tests/complex_taps_arb_restatement.py (pinned to the oracle by
tests/test_complex_taps_arb_cpu.py), the existing FIRFilter.complex_taps_arbitrary(H[c], rate, Nphi).bind(tx, 1) on the GPU, and, for
real samples, the untouched oracle by components.  No tolerance anywhere.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_arb_restatement import ComplexTapsArbitraryRestated
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NCH = 3
RATES = [0.47, 1.0, 2.123, 32.0 / 3]
BANKS = [(4, 4), (4, 30), (32, 250), (32, 1024)]              # (Nphi, hLen): T = 1 (no history), 8 (zero-padded), 8, 32
X_LENS = [1, 5, 257, 1500]                                    # 257: the first size to cross a tile boundary
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
ALL_TYPES = [(np.complex64, np.float32), (np.complex128, np.float64), (np.complex64, np.complex64), (np.complex64, np.complex128),
             (np.complex128, np.complex64)]
FEW_TYPES = [(np.complex64, np.float32), (np.complex64, np.complex64)]
CASES = [((32, 250), t) for t in ALL_TYPES] + [(b, t) for b in BANKS if b != (32, 250) for t in FEW_TYPES]
GENERIC, TILED = "arb_bank_ctaps_generic_kernel", "arb_bank_ctaps_tiled_kernel"


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
    """rows that tell channels and components apart: row 0 random complex, row 1 a single 1j at tap 0 (at rate 1.0 the channel's
    output is 1j times its own input), row 2 = -conj(row 0) reversed; further rows random.  A swapped bank, a shared bank or an
    exchanged re / im fails every case."""
    key = (seed, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, nch)
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        H = ((rng.standard_normal((nch, hLen)) + 1j * rng.standard_normal((nch, hLen))) / hLen).astype(th)
        if nch > 1:
            H[1] = 0
            H[1, 0] = 1j
        if nch > 2:
            H[2] = -np.conj(H[0][::-1])
        x = rng.random((nch, x_len)) - 0.5
        if np.dtype(tx).kind == "c":
            x = x + 1j * (rng.random((nch, x_len)) - 0.5)
        x = x.astype(tx)
        H.setflags(write=False), x.setflags(write=False)
        _SIGNALS[key] = (H, x)
    return _SIGNALS[key]


def _state4(st):
    return (st.inputDeficit, st.phiAccumulator, st.phiIdx, st.alpha)


_REFS = {}


def _reference(seed, rate, Nphi, hLen, x_len, th, tx, how, nch=NCH, mod_form=False):
    """the restatement per channel, one ComplexTapsArbitraryRestated(H[c], rate, Nphi) fed x[c] in the pieces of `how`: (outputs
    [c][piece], (inputDeficit, phiAccumulator, phiIdx, alpha), histories [c]); computed once per case and shared"""
    key = (seed, rate, Nphi, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), nch, mod_form)
    if key not in _REFS:
        H, x = _signal(seed, hLen, x_len, th, tx, nch)
        refs = [ComplexTapsArbitraryRestated(H[c], rate, Nphi, tx=tx, mod_form=1 if mod_form else 0) for c in range(nch)]
        outs = [[r.filt(x[c, a:b], scalar=False) for a, b in _chunks(x_len, how)] for c, r in enumerate(refs)]
        for i in range(len(outs[0])):
            assert len({len(o[i]) for o in outs}) == 1            # (the per-call counts do not depend on the taps)
        states = {_state4(r) for r in refs}
        assert len(states) == 1                                   # (nor does the state)
        _REFS[key] = (outs, states.pop(), [r.history_array() for r in refs])
    return _REFS[key]


def _oracle_by_components(O, H, rate, Nphi, x):
    """real samples: per channel, the oracle's outputs with the taps real(H[c]) and imag(H[c]), put together"""
    rt = np.float32 if H.dtype == np.complex64 else np.float64
    out = []
    for c in range(x.shape[0]):
        yr = O.FIRFilter(np.ascontiguousarray(H[c].real).astype(rt), rate, Nphi, tx=x.dtype).filt(x[c])
        yi = O.FIRFilter(np.ascontiguousarray(H[c].imag).astype(rt), rate, Nphi, tx=x.dtype).filt(x[c])
        y = np.empty(len(yr), dtype=np.complex64 if yr.dtype == np.float32 else np.complex128)
        y.real, y.imag = yr, yi
        out.append(y)
    return np.stack(out)


def _filter(pkg, monkeypatch, H, rate, Nphi, tx, tiled, grid=None):
    """a bound bank filter on the universal kernel (MRHIP_FORCE_GENERIC is read when the device object is created) or on the tiled
    kernel wherever its LDS plan fits (MRHIP_ARB_BANK_CTAPS_TILED=1)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0" if tiled else "1")
    monkeypatch.setenv("MRHIP_ARB_BANK_CTAPS_TILED", "1")
    if grid is None:
        monkeypatch.delenv("MRHIP_ARB_BANK_CTAPS_GRID", raising=False)
    else:
        monkeypatch.setenv("MRHIP_ARB_BANK_CTAPS_GRID", str(grid))
    return pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, rate, Nphi).bind(tx, H.shape[0])


def _want_dtype(th, tx):
    return np.dtype(np.complex128 if (np.dtype(th) == np.complex128 or np.dtype(tx) in (np.float64, np.complex128)) else np.complex64)


def _run_case(pkg, monkeypatch, rate, Nphi, hLen, x_len, th, tx, nch=NCH, grid=None, chunkings=CHUNKINGS, mod_form=False):
    seed = 1000 * Nphi + hLen + x_len
    H, x = _signal(seed, hLen, x_len, th, tx, nch)
    want_dtype = _want_dtype(th, tx)
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        want, state, hists = _reference(seed, rate, Nphi, hLen, x_len, th, tx, how, nch, mod_form)
        for tiled in (False, True):
            what = f"rate {rate} Nphi {Nphi} hLen {hLen} x_len {x_len} {name} tiled={tiled}"
            f = _filter(pkg, monkeypatch, H, rate, Nphi, tx, tiled, grid)
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
            assert st.kind == 4 and st.nchannels == nch and st.tap_dtype == (3 if np.dtype(th) == np.complex128 else 2)
            assert _state4(st) == state, what
            hist = f.history.reshape(nch, -1)
            assert hist.dtype == np.dtype(tx)
            for c in range(nch):
                assert_bit_equal(hist[c], hists[c], f"{what} history {c}")
            f.close()


# ---- 1. shape sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("bank,types", CASES, ids=lambda v: "-".join(np.dtype(t).name for t in v) if isinstance(v[0], type) else "x".join(map(str, v)))
def test_shape_sweep_both_kernels_equal_the_restatement_per_channel(pkg, monkeypatch, bank, types, rate):
    for x_len in X_LENS:
        _run_case(pkg, monkeypatch, rate, *bank, x_len, *types)


# ---- 2. each channel equals the existing one-channel GPU filter ------------------------------------------------------------------
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.float64), (np.complex64, np.complex64)],
                         ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("rate", [0.47, 2.123])
def test_each_channel_equals_the_one_channel_complex_taps_filter(pkg, O, monkeypatch, rate, th, tx):
    Nphi, hLen, x_len = 32, 250, 1500
    H, x = _signal(61, hLen, x_len, th, tx)
    pieces = _chunks(x_len, [1, 0, 7, 2])
    ones, want = [], []
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    for c in range(NCH):
        o = pkg.FIRFilter.complex_taps_arbitrary(H[c], rate, Nphi).bind(tx, 1)
        want.append([o.filt(np.ascontiguousarray(x[c, a:b])) for a, b in pieces])
        assert "bank" not in o.last_kernel_name()
        ones.append(o)
    for tiled in (False, True):
        f = _filter(pkg, monkeypatch, H, rate, Nphi, tx, tiled)
        ys = [f.filt(np.ascontiguousarray(x[:, a:b])).reshape(NCH, -1) for a, b in pieces]
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        st, hist = f.state, f.history.reshape(NCH, -1)
        for c in range(NCH):
            for i in range(len(pieces)):
                assert_bit_equal(ys[i][c], want[c][i], f"channel {c} piece {i} tiled={tiled}")
            so = ones[c].state
            assert _state4(st) + (st.xIdx,) == _state4(so) + (so.xIdx,)
            assert_bit_equal(hist[c], ones[c].history.reshape(-1), f"history {c}")
        if np.dtype(tx).kind != "c":
            assert_bit_equal(np.concatenate(ys, axis=1), _oracle_by_components(O, H, rate, Nphi, x), f"oracle by components, tiled={tiled}")
        f.close()
    for o in ones:
        o.close()


# ---- 3. known answers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=lambda t: np.dtype(t).name)
def test_row_one_multiplies_its_channel_by_i_at_rate_one(pkg, monkeypatch, tx):
    """H[1] = [1j, 0, 0, ...]: at rate 1.0 channel 1 of the output is 1j * x[1] -- whatever the other rows hold (np.array_equal: the
    sign of a zero is not claimed)"""
    H, x = _signal(5, 250, 1500, np.complex64, tx)
    for tiled in (False, True):
        f = _filter(pkg, monkeypatch, H, 1.0, 32, tx, tiled)
        y = f.filt(x)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert np.array_equal(y[1], (1j * x[1].astype(np.complex64)).astype(np.complex64)), f"tiled={tiled}"
        f.close()


def test_known_answer_running_sums_scaled_per_channel(pkg, monkeypatch):
    """H[c] = (c + 1) * (1 - 1j) * ones(Nphi * T), x = ones: every column of pfb_c is (c + 1)(1 - 1j) * ones(T); dh = [diff(h), 0] is
    zero, so dpfb is zero.  Rate 1.0: Δ = Nphi, the accumulator stays 1.0 and every sample gives an output,
    y_c[k] = (c + 1)(1 - 1j) * min(k, T), the running sum of the ones that have arrived.  Rate 0.5: Δ = 2 Nphi, every second sample
    (1, 3, 5, ...) gives one: y_c[k] = (c + 1)(1 - 1j) * min(2k - 1, T)."""
    Nphi, T = 4, 3
    scale = (np.arange(1, NCH + 1) * (1 - 1j)).astype(np.complex64)[:, None]
    H = (scale * np.ones(Nphi * T)).astype(np.complex64)
    x = np.ones((NCH, 10), dtype=np.float32)
    k = np.arange(1, 11)
    for tiled in (False, True):
        for rate, arrived in ((1.0, k), (0.5, 2 * k[:5] - 1)):
            f = _filter(pkg, monkeypatch, H, rate, Nphi, np.float32, tiled)
            assert np.array_equal(f.taps(0), scale[:, :, None] * np.ones((NCH, T, Nphi), dtype=np.complex64)) and not f.taps(1).any()
            y = f.filt(x)
            assert f.last_kernel_name() == (TILED if tiled else GENERIC)
            assert y.dtype == np.complex64 and f.state.alpha == 0.0
            assert np.array_equal(y, (scale * np.minimum(arrived, T)).astype(np.complex64)), (tiled, rate, y)
            f.close()


# ---- 4. a tile whose run exceeds the planned span ----------------------------------------------------------------------------
def test_over_span_tiles_read_global_memory_and_equal_the_universal_kernel_and_the_oracle(pkg, O, monkeypatch):
    """rate 1/50: a full tile of 256 outputs runs over 12 750 samples, more than the 40 KiB of samples the plan gives a tile
    (10 240 Float32 samples): the three full tiles read their windows from global memory, the last (32 outputs) is staged"""
    rate, Nphi, hLen, x_len, nch = 1.0 / 50, 32, 250, 40_000, 2
    H, x = _signal(7, hLen, x_len, np.complex64, np.float32, nch)
    ys = {}
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, H, rate, Nphi, np.float32, tiled)
        ys[tiled] = f.filt(x)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        ys[tiled, "hist"], ys[tiled, "state"] = f.history, _state4(f.state)
        f.close()
    assert ys[True].shape == (nch, 800)
    assert_bit_equal(ys[True], ys[False], "tiled == universal")
    assert_bit_equal(ys[True, "hist"], ys[False, "hist"], "history")
    assert_bit_equal(ys[True, "hist"], np.array(x[:, -7:]), "history == the last samples")
    assert ys[True, "state"] == ys[False, "state"]
    assert_bit_equal(ys[True], _oracle_by_components(O, H, rate, Nphi, x), "tiled == oracle by components")


# ---- 5. ownership of tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 3, 7, 64])
def test_workgroups_that_cross_channel_boundaries_reload_both_banks(pkg, monkeypatch, grid):
    """5 channels x 9 tiles: one workgroup walks every channel (1), runs that cross a channel in mid-run (2, 3, 7), more workgroups
    than the 45 tiles (64: idle ones)"""
    _run_case(pkg, monkeypatch, math.pi / 3, 32, 250, 2000, np.complex64, np.float32, nch=5, grid=grid, chunkings={"whole": None})


@pytest.mark.parametrize("nch", [1, 2, 33])
def test_channel_counts_at_the_default_grid(pkg, monkeypatch, nch):
    _run_case(pkg, monkeypatch, math.pi / 3, 32, 250, 2000, np.complex64, np.float32, nch=nch, chunkings={"whole": None})


# ---- 6. the default rule -----------------------------------------------------------------------------------------------------
def test_the_default_rule_takes_the_tiled_kernel_from_twenty_tiles_per_cu(pkg, monkeypatch):
    """MRHIP_ARB_BANK_CTAPS_TILED unset (the measured rule): 33 channels x 164 tiles are more than 20 tiles per CU
    of a 256-CU chip -- the tiled kernel; 33 x 9 and 3 x 9 tiles are fewer -- the universal kernel; =0: never the tiled kernel; =1: the
    tiled kernel at 3 x 9 tiles too.  The outputs are the restatement's in every case."""
    rate, Nphi, hLen = math.pi / 3, 32, 250
    for nch, x_len, mode, kernel in ((33, 40_000, None, TILED), (33, 2000, None, GENERIC), (3, 2000, None, GENERIC), (33, 40_000, "0", GENERIC),
                                     (3, 2000, "1", TILED)):
        seed = 1000 * Nphi + hLen + x_len
        H, x = _signal(seed, hLen, x_len, np.complex64, np.float32, nch)
        want, state, _ = _reference(seed, rate, Nphi, hLen, x_len, np.complex64, np.float32, None, nch)
        monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
        monkeypatch.delenv("MRHIP_ARB_BANK_CTAPS_GRID", raising=False)
        if mode is None:
            monkeypatch.delenv("MRHIP_ARB_BANK_CTAPS_TILED", raising=False)
        else:
            monkeypatch.setenv("MRHIP_ARB_BANK_CTAPS_TILED", mode)
        f = pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, rate, Nphi).bind(np.float32, nch)
        y = f.filt(x)
        assert f.last_kernel_name() == kernel, (nch, x_len, mode)
        assert_bit_equal(y, np.stack([w[0] for w in want]), f"default rule, {nch} channels x {x_len}, MRHIP_ARB_BANK_CTAPS_TILED={mode}")
        assert _state4(f.state) == state
        f.close()


# ---- 7. a call that mrhip_filt_device splits into pieces ---------------------------------------------------------------------
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=lambda t: np.dtype(t).name)
def test_split_call_places_every_piece_and_leaves_the_right_history(pkg, monkeypatch, torch_cuda, tx):
    """MRHIP_LAUNCH_MAX=4099: a piece per 4099 outputs, each written at its own offset of y (in OUTPUT elements: a complex output
    of real samples is twice the sample size)"""
    torch = torch_cuda
    rate, Nphi, hLen, x_len, nch = 1.37, 32, 250, 30_011, 2
    H, x = _signal(9, hLen, x_len, np.complex64, tx, nch)
    want, state, hists = _reference(9, rate, Nphi, hLen, x_len, np.complex64, tx, None, nch)
    xd = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setenv("MRHIP_LAUNCH_MAX", "4099")
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, H, rate, Nphi, tx, tiled)
        y = f.filt(xd).cpu().numpy()
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert_bit_equal(y, np.stack([w[0] for w in want]), f"split call, tiled={tiled}")
        assert _state4(f.state) == state
        assert_bit_equal(f.history, np.stack(hists), "history")
        assert_bit_equal(f.history[1], x[1, -f.historyLen:], "history == the last samples")
        f.close()


# ---- 8. the host-scheduled path ----------------------------------------------------------------------------------------------
def test_host_scheduled_calls_under_the_older_mod_form(pkg, monkeypatch):
    """set_mod_form(True) with an Nphi that is no power of two: the schedule is evaluated on the host"""
    _run_case(pkg, monkeypatch, 0.47, 6, 30, 1500, np.complex64, np.float32, chunkings={"whole": None, "prime": 97}, mod_form=True)
    _run_case(pkg, monkeypatch, 0.47, 6, 30, 257, np.complex64, np.complex64, chunkings={"ragged": [1, 0, 7, 2]}, mod_form=True)


# ---- 9. device-planned calls -------------------------------------------------------------------------------------------------
def _restated_stream(H, rate, Nphi, x, chunk, n):
    refs = [ComplexTapsArbitraryRestated(H[c], rate, Nphi, tx=x.dtype) for c in range(H.shape[0])]
    out = [np.stack([r.filt(x[c, i * chunk:(i + 1) * chunk], scalar=False) for c, r in enumerate(refs)]) for i in range(n)]
    return out, _state4(refs[0]), np.stack([r.history_array() for r in refs])


@pytest.mark.parametrize("tiled", [False, True])
def test_async_calls_equal_the_synchronous_stream(pkg, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, chunk, n = 2.123, 32, 250, 96, 5
    H, x = _signal(21, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _restated_stream(H, rate, Nphi, x, chunk, n)
    sync = _filter(pkg, monkeypatch, H, rate, Nphi, np.complex64, tiled)
    for i in range(n):
        assert_bit_equal(sync.filt(np.ascontiguousarray(x[:, i * chunk:(i + 1) * chunk])), want[i], f"synchronous call {i}")
    sync.close()
    f = _filter(pkg, monkeypatch, H, rate, Nphi, np.complex64, tiled)
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
    assert _state4(f.state) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


@pytest.mark.parametrize("tiled", [False, True])
def test_captured_call_replayed_three_times_equals_the_synchronous_stream(pkg, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, chunk, n = 2.123, 32, 250, 96, 5               # chunk >= historyLen (7)
    H, x = _signal(22, hLen, chunk * n, np.complex64, np.float32)
    want, state, hist = _restated_stream(H, rate, Nphi, x, chunk, n)
    f = _filter(pkg, monkeypatch, H, rate, Nphi, np.float32, tiled)
    xd = torch.from_numpy(np.array(x)).cuda()
    # The stream starts with a plain call and an asynchronous one of the captured size: the schedule's work buffers are allocated
    # by the first device-planned call of a size (allocations cannot be captured).  The graph takes the stream over from there.
    assert_bit_equal(f.filt(xd[:, :chunk].contiguous()).cpu().numpy(), want[0], "plain call")
    bound = f.outputlength_bound(chunk)
    y1 = torch.zeros((NCH, bound), dtype=torch.complex64, device="cuda")
    f.filt_into_async(y1, xd[:, chunk:2 * chunk])
    c1 = f.sync_state()
    assert_bit_equal(y1[:, :c1].cpu().numpy(), want[1], "asynchronous call of the captured size")
    xs = torch.zeros((NCH, chunk), dtype=torch.float32, device="cuda")
    ys = torch.zeros((NCH, bound), dtype=torch.complex64, device="cuda")
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
    assert _state4(f.state) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


@pytest.mark.parametrize("tiled", [False, True])
def test_chained_call_behind_a_decimator(pkg, O, monkeypatch, torch_cuda, tiled):
    """filt_into_async(..., after=prev): the input length of the bank filter's call is the decimator's count, on the device"""
    torch = torch_cuda
    rate, Nphi, hLen = 2.123, 32, 250
    sizes = [1001, 17, 2000]
    H, x = _signal(23, hLen, sum(sizes), np.complex64, np.float32)
    h1 = np.random.default_rng(24).standard_normal(16).astype(np.float32)
    f1 = pkg.FIRFilter(h1, Fraction(1, 4)).bind(np.float32, NCH)
    f2 = _filter(pkg, monkeypatch, H, rate, Nphi, np.float32, tiled)
    o1 = [O.FIRFilter(h1, Fraction(1, 4), tx=np.float32) for _ in range(NCH)]
    o2 = [ComplexTapsArbitraryRestated(H[c], rate, Nphi, tx=np.float32) for c in range(NCH)]
    xd = torch.from_numpy(np.array(x)).cuda()
    mid = torch.zeros((NCH, f1.outputlength_bound(max(sizes))), dtype=torch.float32, device="cuda")
    outs = [torch.zeros((NCH, f2.outputlength_bound(f1.outputlength_bound(s))), dtype=torch.complex64, device="cuda") for s in sizes]
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
            ref = o2[c].filt(o1[c].filt(x[c, pos:pos + s]), scalar=False)
            assert counts[i] == len(ref), (i, c, counts[i], len(ref))
            assert_bit_equal(outs[i][c, :counts[i]].cpu().numpy(), ref, f"chained call {i} channel {c}")
        pos += s
    f2.sync_state()
    assert _state4(f2.state) == _state4(o2[0])
    assert_bit_equal(f2.history, np.stack([r.history_array() for r in o2]), "history after the chained calls")
    f1.close(), f2.close()


# ---- 10. contract edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [np.complex64, np.complex128], ids=lambda t: np.dtype(t).name)
def test_taps_tapsforphase_and_reset(pkg, monkeypatch, th):
    rate, Nphi, hLen, x_len = 0.47, 4, 30, 300
    H, x = _signal(31, hLen, x_len, th, np.float32)
    refs = [ComplexTapsArbitraryRestated(H[c], rate, Nphi, tx=np.float32) for c in range(NCH)]
    f = _filter(pkg, monkeypatch, H, rate, Nphi, np.float32, tiled=True)
    ones = [pkg.FIRFilter.complex_taps_arbitrary(H[c], rate, Nphi).bind(np.float32, 1) for c in range(NCH)]
    pfb, dpfb = f.taps(0), f.taps(1)
    assert pfb.shape == dpfb.shape == (NCH, f.tapsPerPhi, Nphi) and pfb.dtype == np.dtype(th)
    for c in range(NCH):
        assert_bit_equal(pfb[c], refs[c].pfb, f"pfb of channel {c}")
        assert_bit_equal(dpfb[c], refs[c].dpfb, f"dpfb of channel {c}")
        assert_bit_equal(pfb[c], ones[c].taps(0), f"pfb of channel {c} == the one-channel filter's")
        assert_bit_equal(dpfb[c], ones[c].taps(1), f"dpfb of channel {c} == the one-channel filter's")
    for phase in (1.0, 1.25, Nphi + 0.5):
        t = f.tapsforphase(phase)
        assert t.shape == (NCH, f.tapsPerPhi) and t.dtype == np.dtype(th)
        for c in range(NCH):
            assert_bit_equal(t[c], ones[c].tapsforphase(phase), f"tapsforphase({phase}) of channel {c}")
            assert_bit_equal(t[c], refs[c].tapsforphase(phase), f"tapsforphase({phase}) of channel {c} == the restatement's")
    for bad in (0.5, Nphi + 1.0, -1.0):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.tapsforphase(bad)
        assert e.value.code == 1
    want = np.stack([r.filt(x[c], scalar=False) for c, r in enumerate(refs)])
    assert_bit_equal(f.filt(x), want, "first run")
    f.reset()
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == (1, 1.0) and not f.history.any()
    assert_bit_equal(f.filt(x), want, "reset, then the same again")
    f.close()
    for o in ones:
        o.close()


def test_buffer_too_small_wrong_channel_count_fused_and_the_c_abi_errors(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    lib = pkg.load_library()
    F32, F64, C64, C128 = 0, 1, 2, 3
    H, x = _signal(33, 8, 100, np.complex64, np.float32)
    f = _filter(pkg, monkeypatch, H, 1.5, 4, np.float32, tiled=True)
    assert lib.mrhip_set_numerics(f._handle, 1) == 5            # FUSED: no fused form is defined for complex taps
    assert lib.mrhip_set_numerics(f._handle, 0) == 0
    xd = torch.from_numpy(np.array(x)).cuda()
    small = torch.zeros((NCH, 10), dtype=torch.complex64, device="cuda")
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.filt_into(small, xd)                                          # buffer too small: the state stays
    assert e.value.code == 2
    assert (f.state.inputDeficit, f.state.phiAccumulator) == (1, 1.0) and not f.history.any()
    want = np.stack([ComplexTapsArbitraryRestated(H[c], 1.5, 4, tx=np.float32).filt(x[c], scalar=False) for c in range(NCH)])
    assert_bit_equal(f.filt(xd).cpu().numpy(), want, "the same call with room")
    f.close()
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, 1.5, 4).bind(np.float32, NCH + 1)
    assert e.value.code == 1
    out = C.c_void_p()
    for th, hh in ((F32, np.array(H.real).astype(np.float32)), (F64, np.array(H.real).astype(np.float64))):   # real taps: the other constructor
        rc = lib.mrhip_create_arbitrary_bank_ctaps(hh.ctypes.data_as(C.c_void_p), H.shape[1], th, 1.5, 4, F32, NCH, 0, C.byref(out))
        assert rc == 1 and not out.value
        assert "mrhip_create_arbitrary_bank" in lib.mrhip_last_error().decode()
    for th, hh in ((C64, np.array(H)), (C128, np.array(H).astype(np.complex128))):
        p = hh.ctypes.data_as(C.c_void_p)
        for rate in (0.0, -1.0):
            assert lib.mrhip_create_arbitrary_bank_ctaps(p, H.shape[1], th, rate, 4, F32, NCH, 0, C.byref(out)) == 1 and not out.value
        assert lib.mrhip_create_arbitrary_bank_ctaps(p, H.shape[1], th, 1.5, 0, F32, NCH, 0, C.byref(out)) == 1 and not out.value   # bad Nphi
        assert lib.mrhip_create_arbitrary_bank_ctaps(None, H.shape[1], th, 1.5, 4, F32, NCH, 0, C.byref(out)) == 1 and not out.value
        rc = lib.mrhip_create_arbitrary_bank(p, H.shape[1], th, 1.5, 4, F32, NCH, 0, C.byref(out))      # keeps refusing complex taps
        assert rc == 5 and not out.value and "left out" in lib.mrhip_last_error().decode()


def test_equal_rows_equal_the_shared_taps_filter(pkg, monkeypatch):
    rate, Nphi, hLen, x_len = 2.123, 32, 250, 1500
    H, x = _signal(51, hLen, x_len, np.complex64, np.complex64)
    same = np.ascontiguousarray(np.broadcast_to(H[0], (NCH, hLen)))
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    shared = pkg.FIRFilter.complex_taps_arbitrary(H[0], rate, Nphi)      # mrhip_create_arbitrary_ctaps: one h for every channel, as before
    want = shared.filt(np.array(x))
    assert "bank" not in shared.last_kernel_name()
    ss = shared.state
    for tiled in (False, True):
        b = _filter(pkg, monkeypatch, same, rate, Nphi, np.complex64, tiled)
        assert_bit_equal(b.filt(np.array(x)), want, f"equal rows == the shared-taps filter, tiled={tiled}")
        assert b.last_kernel_name() == (TILED if tiled else GENERIC)
        assert_bit_equal(b.history, shared.history, "history")
        st = b.state
        assert _state4(st) + (st.xIdx,) == _state4(ss) + (ss.xIdx,)
        b.close()
    shared.close()


def test_cascade_takes_such_a_stage_through_the_per_stage_calls(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    H, x = _signal(41, 250, 3000, np.complex64, np.float32)
    h2 = np.random.default_rng(42).standard_normal(16).astype(np.float32)
    xd = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.setenv("MRHIP_ARB_BANK_CTAPS_TILED", "1")
    a, b = pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, 2.123, 32), pkg.FIRFilter(h2, Fraction(1, 2))
    by_hand = b.filt(a.filt(xd))
    cas = pkg.FilterCascade(pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, 2.123, 32), pkg.FIRFilter(h2, Fraction(1, 2)))
    y = cas.filt(xd)
    assert cas.stages[0].last_kernel_name() == TILED and y.dtype == torch.complex64
    assert_bit_equal(y.cpu().numpy(), by_hand.cpu().numpy(), "cascade == by hand")
    cas.close(), a.close(), b.close()


def test_filt_multi_with_such_a_filter_equals_the_single_calls(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    rate, Nphi, hLen, x_len = 2.123, 32, 250, 400
    H, x = _signal(43, hLen, x_len, np.complex64, np.float32)
    want = np.stack([ComplexTapsArbitraryRestated(H[c], rate, Nphi, tx=np.float32).filt(x[c], scalar=False) for c in range(NCH)])
    bank = _filter(pkg, monkeypatch, H, rate, Nphi, np.float32, tiled=True)
    plain = pkg.FIRFilter.complex_taps_arbitrary(H[0], rate, Nphi)
    xd = torch.from_numpy(np.array(x)).cuda()
    ys = pkg.filt_multi([bank, plain], [xd, xd[0].contiguous()])
    assert_bit_equal(ys[0].cpu().numpy(), want, "the bank filter's stream")
    assert_bit_equal(ys[1].cpu().numpy(), want[0], "the other stream")
    assert bank.last_kernel_name() == TILED
    bank.close(), plain.close()


def test_ring_is_not_resident(pkg, monkeypatch):
    H, _ = _signal(44, 250, 8, np.complex64, np.float32)
    f = _filter(pkg, monkeypatch, H, 2.123, 32, np.float32, tiled=True)
    with f.open_ring() as ring:
        assert ring.info()["resident"] is False
    f.close()
