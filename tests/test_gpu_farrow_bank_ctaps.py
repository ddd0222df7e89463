"""GPU tests of per-channel complex taps for FIRFarrow (csrc/kernels_bank_farrow_ctaps.hip):
FIRFilter.per_channel_complex_taps_farrow(H, rate, Nphi, polyorder), one FIRFilter(H[c]::Vector{Complex}, rate, Nphi, polyorder) per
channel behind one filter object (mrhip_create_farrow_bank_ctaps).

Bar (include/multirate_hip.h, "Per-channel complex taps for FIRFarrow"): for every channel c the outputs, the per-call counts, the end
state and the history are BIT FOR BIT those of tests/complex_taps_farrow_restatement.py (pinned to the oracle by
tests/test_complex_taps_farrow_cpu.py) on the per-component fit of H[c], fed x[c] -- whole and chunked (a one-sample chunk, an empty
one, chunks shorter than the history), host-scheduled, split, device-planned, captured and chained; they are those of the one-channel
FIRFilter.complex_taps_farrow(H[c], ...) on the GPU; and for real samples re(y) / im(y) are the untouched oracle's outputs with the
banks real(pnfb_c) / imag(pnfb_c) and the outputs of the two real banks per_channel_farrow(real(H)) / per_channel_farrow(imag(H)).
There is one kernel (farrow_bank_ctaps_generic_kernel) and no tolerance anywhere.

The polynomial fit.  The reference pins no bits of polyfit; the bank constructor takes no caller-fitted pnfb, so the restatement is
handed the library's per-component fit of row c (fit_pnfb with mrhip_polyfit), and the fit itself is checked on its own: the bank's pnfb
is bit for bit that fit, the one-channel filter's pnfb, and by components the two real banks' pnfb.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_farrow_restatement import ComplexTapsFarrowRestated, fit_pnfb
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NCH = 3
RATES = [0.47, 1.0, 2.123, 32.0 / 3]
# (Nphi, hLen, polyorder): T = 1 (no history); a constant polynomial; polyorder = Nphi - 1, T = 8 with zero-padded rows; the unrolled
# path (polyorder 4), T = 8; T = 32; T = 33 on the runtime Horner loop
BANKS = [(4, 4, 2), (4, 30, 0), (4, 30, 3), (32, 250, 4), (32, 1024, 4), (8, 264, 2)]
X_LENS = [1, 5, 257, 1500]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
# (tap, sample): the six instantiations (Tx scalar, R, components) = (f32,f32,1) (f32,f64,1) (f64,f64,1) (f32,f32,2) (f32,f64,2) (f64,f64,2)
ALL_TYPES = [(np.complex64, np.float32), (np.complex128, np.float32), (np.complex128, np.float64), (np.complex64, np.complex64),
             (np.complex128, np.complex64), (np.complex64, np.complex128)]
FEW_TYPES = [(np.complex64, np.float32), (np.complex128, np.complex64)]
CASES = [((32, 250, 4), t) for t in ALL_TYPES] + [(b, t) for b in BANKS if b != (32, 250, 4) for t in FEW_TYPES]
KERNEL = "farrow_bank_ctaps_generic_kernel"


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
    """rows that tell channels apart: row 0 random complex, row 1 a single 1j at tap 0, row 2 = row 0 reversed, negated and
    conjugated; further rows random.  A swapped or a shared bank, or swapped components, fail every case."""
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


_FITS = {}


def _fit(pkg, h, Nphi, P):
    """the library's per-component fit of one tap vector (mrhip_polyfit on the real and on the imaginary parts of every row of
    taps2pfb(h, Nphi)); computed once per tap vector"""
    key = (h.tobytes(), h.dtype.name, Nphi, P)
    if key not in _FITS:
        _FITS[key] = fit_pnfb(np.array(h), Nphi, P, pkg.polyfit)
    return _FITS[key]


def _restated(pkg, h, rate, Nphi, P, tx, mod_form=False):
    return ComplexTapsFarrowRestated(len(h), h.dtype, rate, Nphi, P, _fit(pkg, h, Nphi, P), tx=tx, mod_form=1 if mod_form else 0)


def _state2(st):
    return (st.inputDeficit, st.phiAccumulator)


_REFS = {}


def _reference(pkg, seed, rate, Nphi, hLen, P, x_len, th, tx, how, nch=NCH, mod_form=False):
    """the restatement per channel, fed x[c] in the pieces of `how`: (outputs [c][piece], (inputDeficit, phiAccumulator), histories
    [c]); computed once per case and shared"""
    key = (seed, rate, Nphi, hLen, P, x_len, np.dtype(th).name, np.dtype(tx).name, str(how), nch, mod_form)
    if key not in _REFS:
        H, x = _signal(seed, hLen, x_len, th, tx, nch)
        refs = [_restated(pkg, H[c], rate, Nphi, P, tx, mod_form) for c in range(nch)]
        outs = [[r.filt(x[c, a:b], scalar=False) for a, b in _chunks(x_len, how)] for c, r in enumerate(refs)]
        for i in range(len(outs[0])):
            assert len({len(o[i]) for o in outs}) == 1            # (the per-call counts do not depend on the taps)
        states = {(r.inputDeficit, r.phiAccumulator) for r in refs}
        assert len(states) == 1                                   # (nor does the state)
        _REFS[key] = (outs, states.pop(), [r.history_array() for r in refs])
    return _REFS[key]


def _filter(pkg, monkeypatch, H, rate, Nphi, P, tx, force_generic="0"):
    """a bound bank filter; MRHIP_FORCE_GENERIC (read when the device object is created) has no effect on it: there is one kernel"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", force_generic)
    return pkg.FIRFilter.per_channel_complex_taps_farrow(H, rate, Nphi, P).bind(tx, H.shape[0])


def _want_dtype(th, tx):
    return np.dtype(np.complex128 if (th == np.complex128 or np.dtype(tx) in (np.float64, np.complex128)) else np.complex64)


def _run_case(pkg, monkeypatch, rate, Nphi, hLen, P, x_len, th, tx, nch=NCH, chunkings=CHUNKINGS, mod_form=False, force_generic="0"):
    seed = 1000 * Nphi + hLen + x_len
    H, x = _signal(seed, hLen, x_len, th, tx, nch)
    want_dtype = _want_dtype(th, tx)
    for name, how in chunkings.items():
        pieces = _chunks(x_len, how)
        want, state, hists = _reference(pkg, seed, rate, Nphi, hLen, P, x_len, th, tx, how, nch, mod_form)
        assert want[0][0].dtype == want_dtype
        what = f"rate {rate} Nphi {Nphi} hLen {hLen} P {P} x_len {x_len} {name}"
        f = _filter(pkg, monkeypatch, H, rate, Nphi, P, tx, force_generic)
        if mod_form:
            f.set_mod_form(True)
        assert f.output_dtype == want_dtype
        for i, (a, b) in enumerate(pieces):
            y = f.filt(np.ascontiguousarray(x[:, a:b])).reshape(nch, -1)
            assert y.dtype == want_dtype and y.shape == (nch, len(want[0][i])), (what, a, b, y.shape)   # the per-call count
            for c in range(nch):
                assert_bit_equal(y[c], want[c][i], f"{what} chunk [{a}, {b}) channel {c}")
            if y.shape[1] > 0:
                assert f.last_kernel_name() == KERNEL, what
        st = f.state
        assert st.kind == 5 and st.nchannels == nch and st.tap_dtype == (3 if th == np.complex128 else 2)
        assert _state2(st) == state, what
        hist = f.history.reshape(nch, -1)
        assert hist.dtype == np.dtype(tx)
        for c in range(nch):
            assert_bit_equal(hist[c], hists[c], f"{what} history {c}")
        f.close()


def _ids(v):
    return "-".join(np.dtype(t).name for t in v) if isinstance(v[0], type) else "x".join(map(str, v))


# ---- 1. shape sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("bank,types", CASES, ids=_ids)
def test_shape_sweep_equals_the_restatement_per_channel(pkg, monkeypatch, bank, types, rate):
    for x_len in X_LENS:
        _run_case(pkg, monkeypatch, rate, *bank, x_len, *types)


def test_force_generic_has_no_effect(pkg, monkeypatch):
    _run_case(pkg, monkeypatch, 2.123, 32, 250, 4, 257, np.complex64, np.float32, chunkings={"whole": None}, force_generic="1")


# ---- 2. each channel is the one-channel complex-tap filter -------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.47, 2.123])
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.complex64), (np.complex64, np.complex128)], ids=lambda t: np.dtype(t).name)
def test_each_channel_equals_the_one_channel_filter_on_the_gpu(pkg, monkeypatch, th, tx, rate):
    Nphi, hLen, P, x_len = 32, 250, 4, 1500
    H, x = _signal(71, hLen, x_len, th, tx)
    pieces = _chunks(x_len, [1, 0, 7, 2, 400])
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, tx)
    ys = [f.filt(np.ascontiguousarray(x[:, a:b])) for a, b in pieces]
    pn = f.pnfb()
    for c in range(NCH):
        one = pkg.FIRFilter.complex_taps_farrow(np.array(H[c]), rate, Nphi, P).bind(tx, 1)
        for i, (a, b) in enumerate(pieces):
            y1 = one.filt(np.ascontiguousarray(x[c, a:b]))
            assert_bit_equal(ys[i][c], y1.reshape(-1), f"channel {c} chunk [{a}, {b})")                # outputs and per-call counts
        assert "bank" not in one.last_kernel_name()
        assert _state2(one.state) + (one.state.phiIdx,) == _state2(f.state) + (f.state.phiIdx,)
        assert_bit_equal(f.history[c], one.history.reshape(-1), f"history of channel {c}")
        assert_bit_equal(pn[c], one.pnfb(), f"pnfb of channel {c}")
        one.close()
    f.close()


# ---- 3. real samples: by components ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.47, 2.123])
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.float32), (np.complex128, np.float64)], ids=lambda t: np.dtype(t).name)
def test_real_samples_equal_the_oracle_and_the_two_real_banks_by_components(pkg, O, monkeypatch, th, tx, rate):
    Nphi, hLen, P, x_len = 32, 250, 4, 1500
    H, x = _signal(72, hLen, x_len, th, tx)
    rt = np.float32 if th == np.complex64 else np.float64
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, tx)
    y = f.filt(np.array(x))
    pn = f.pnfb()
    assert pn.shape == (NCH, f.tapsPerPhi, P + 1) and pn.dtype == np.complex128
    hr = np.zeros(hLen, dtype=rt)
    for c in range(NCH):                                                       # the untouched oracle on the two component banks
        for part, name in ((np.real, "re"), (np.imag, "im")):
            bank = np.ascontiguousarray(part(pn[c]))
            want = O.FIRFilter(hr, rate, Nphi, tx=tx, polyorder=P, pnfb=bank).filt(x[c])
            assert_bit_equal(np.ascontiguousarray(part(y[c])), want, f"{name}(y) of channel {c} == the oracle with {name}(pnfb)")
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "1")
    for part, name in ((np.real, "re"), (np.imag, "im")):                      # the two real banks on the GPU
        g = pkg.FIRFilter.per_channel_farrow(np.ascontiguousarray(part(H)), rate, Nphi, P).bind(tx, NCH)
        assert_bit_equal(np.ascontiguousarray(part(y)), g.filt(np.array(x)), f"{name}(y) == per_channel_farrow({name}(H))")
        assert_bit_equal(np.ascontiguousarray(part(pn)), g.pnfb(), f"{name}(pnfb) == that filter's pnfb")
        assert _state2(g.state) == _state2(f.state)
        assert_bit_equal(g.history, f.history, "history")
        g.close()
    f.close()


# ---- 4. equal rows, a known answer, the seam ---------------------------------------------------------------------------------
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.complex64)], ids=lambda t: np.dtype(t).name)
def test_equal_rows_equal_the_shared_taps_filter(pkg, monkeypatch, th, tx):
    rate, Nphi, hLen, P, x_len = 2.123, 32, 250, 4, 1500
    H, x = _signal(51, hLen, x_len, th, tx)
    same = np.ascontiguousarray(np.broadcast_to(H[0], (NCH, hLen)))
    for ctaps_tiled in ("0", "1"):
        monkeypatch.setenv("MRHIP_CTAPS_TILED", ctaps_tiled)
        shared = pkg.FIRFilter.complex_taps_farrow(np.array(H[0]), rate, Nphi, P)       # one h for every channel, as before
        want = shared.filt(np.array(x))
        assert "bank" not in shared.last_kernel_name()
        b = _filter(pkg, monkeypatch, same, rate, Nphi, P, tx)
        assert_bit_equal(b.filt(np.array(x)), want, f"equal rows == the shared-taps filter (MRHIP_CTAPS_TILED={ctaps_tiled})")
        assert b.last_kernel_name() == KERNEL
        assert_bit_equal(b.history, shared.history, "history")
        st, ss = b.state, shared.state
        assert _state2(st) + (st.phiIdx, st.xIdx) == _state2(ss) + (ss.phiIdx, ss.xIdx)
        b.close(), shared.close()


def test_known_answer_running_sums_scaled_per_channel(pkg, monkeypatch):
    """H[c] = s_c * ones(Nphi * T) with the complex scale s_c = (c + 1) + (c + 2)im, x = ones: every row of pfb_c is constant, its
    fitted polynomial is s_c plus higher coefficients of about 1e-16 that vanish when the tap's components are rounded to Float32, so
    every tap is s_c and an output is s_c times the number of ones in its window: y_c[k] = s_c * min(n_k, T).  Rate 1.0: every sample
    gives an output, n_k = k.  Rate 0.5: every second sample (1, 3, 5, ...) gives one, n_k = 2k - 1."""
    Nphi, T, P = 32, 4, 4
    scale = (np.arange(1, NCH + 1) + 1j * np.arange(2, NCH + 2)).astype(np.complex64)
    H = np.outer(scale, np.ones(Nphi * T)).astype(np.complex64)
    x = np.ones((NCH, 10), dtype=np.float32)
    k = np.arange(1, 11)
    for rate, arrived in ((1.0, k), (0.5, 2 * k[:5] - 1)):
        f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
        y = f.filt(x)
        assert y.dtype == np.complex64 and f.last_kernel_name() == KERNEL
        assert np.array_equal(y, scale[:, None] * np.minimum(arrived, T).astype(np.float32)), (rate, y)
        assert np.array_equal(y[:, -1], 4 * scale)
        f.close()


@pytest.mark.parametrize("rate,plus", [(0.47, 2), (2.123, 7)])
def test_seam_outputs_start_from_plus_zero_per_component(pkg, monkeypatch, rate, plus):
    """negative constant rows in both components, x = 0: every product is -0.0, and so is every sum of them -- except on the seam
    (the outputs whose window still reaches into the history of a call: n < tapsPerPhi), which start from +0.0 per component
    (support.jl:46): 0 + (-0) = +0.  The first `plus` outputs of EACH call are +0.0, the rest -0.0."""
    Nphi, T, P, x_len = 32, 4, 4, 40
    H = -np.outer(np.arange(1, NCH + 1) * (1 + 2j), np.ones(Nphi * T)).astype(np.complex64)
    x = np.zeros((NCH, x_len), dtype=np.float32)
    refs = [_restated(pkg, H[c], rate, Nphi, P, np.float32) for c in range(NCH)]
    want = [np.stack([r.filt(x[c], scalar=False) for c, r in enumerate(refs)]) for _ in range(2)]
    for w in want:
        for part in (w.real, w.imag):
            sign = np.signbit(part)
            assert not part.any() and not sign[:, :plus].any() and sign[:, plus:].all() and w.shape[1] > plus     # (the case is not vacuous)
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
    for i in range(2):
        y = f.filt(x)
        assert f.last_kernel_name() == KERNEL
        assert_bit_equal(y, want[i], f"signs of zero, call {i}")
    f.close()


# ---- 5. channel counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 33])
def test_channel_counts(pkg, monkeypatch, nch):
    _run_case(pkg, monkeypatch, 2.123, 32, 250, 4, 707, np.complex64, np.float32, nch=nch, chunkings={"whole": None})
    _run_case(pkg, monkeypatch, 2.123, 32, 250, 4, 707, np.complex128, np.complex64, nch=nch, chunkings={"prime": 97})


# ---- 6. call paths, each against the synchronous stream ----------------------------------------------------------------------
@pytest.mark.parametrize("tx", [np.float32, np.complex64], ids=lambda t: np.dtype(t).name)
def test_split_call_places_every_piece_and_leaves_the_right_history(pkg, monkeypatch, torch_cuda, tx):
    """MRHIP_LAUNCH_MAX=4099: a piece per 4099 outputs, each written at its own offset of y (in OUTPUT elements: real samples give
    a complex output); the continuation pieces have no seam.  Against the same call in one piece, and against the restatement."""
    torch = torch_cuda
    rate, Nphi, hLen, P, x_len, nch = 1.37, 32, 250, 4, 30_011, 2
    H, x = _signal(9, hLen, x_len, np.complex64, tx, nch)
    want, state, hists = _reference(pkg, 9, rate, Nphi, hLen, P, x_len, np.complex64, tx, None, nch)
    xd = torch.from_numpy(np.array(x)).cuda()
    whole = _filter(pkg, monkeypatch, H, rate, Nphi, P, tx)
    y0 = whole.filt(xd).cpu().numpy()
    h0 = whole.history
    whole.close()
    monkeypatch.setenv("MRHIP_LAUNCH_MAX", "4099")
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, tx)
    y = f.filt(xd).cpu().numpy()
    assert y.shape[1] > 10 * 4099 and f.last_kernel_name() == KERNEL              # (eleven pieces)
    assert_bit_equal(y, y0, "split call == the call in one piece")
    assert_bit_equal(y, np.stack([w[0] for w in want]), "split call == the restatement")
    assert _state2(f.state) == state
    assert_bit_equal(f.history, h0, "history == the one-piece call's")
    assert_bit_equal(f.history, np.stack(hists), "history == the restatement's")
    assert_bit_equal(f.history[1], x[1, -f.historyLen:], "history == the last samples")
    f.close()


def test_host_scheduled_calls_under_the_older_mod_form(pkg, monkeypatch):
    """set_mod_form(True) with an Nphi that is no power of two: the schedule is evaluated on the host"""
    _run_case(pkg, monkeypatch, 0.47, 6, 30, 3, 1500, np.complex64, np.float32, chunkings={"whole": None, "prime": 97}, mod_form=True)
    _run_case(pkg, monkeypatch, 0.47, 6, 30, 3, 257, np.complex128, np.complex64, chunkings={"ragged": [1, 0, 7, 2]}, mod_form=True)


def _sync_stream(pkg, monkeypatch, H, rate, Nphi, P, x, chunk, n):
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, x.dtype)
    out = [f.filt(np.ascontiguousarray(x[:, i * chunk:(i + 1) * chunk])).reshape(x.shape[0], -1) for i in range(n)]
    state, hist = _state2(f.state), f.history
    f.close()
    refs = [_restated(pkg, H[c], rate, Nphi, P, x.dtype) for c in range(H.shape[0])]       # (the synchronous stream is the restatement's)
    for i in range(n):
        for c, r in enumerate(refs):
            assert_bit_equal(out[i][c], r.filt(x[c, i * chunk:(i + 1) * chunk], scalar=False), f"synchronous call {i} channel {c}")
    return out, state, hist


def test_async_calls_equal_the_synchronous_stream(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    rate, Nphi, hLen, P, chunk, n = 2.123, 32, 250, 4, 96, 5
    H, x = _signal(21, hLen, chunk * n, np.complex64, np.complex64)
    want, state, hist = _sync_stream(pkg, monkeypatch, H, rate, Nphi, P, x, chunk, n)
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.complex64)
    xd = torch.from_numpy(np.array(x)).cuda()
    bound = f.outputlength_bound(chunk)
    ys = torch.zeros((n, NCH, bound), dtype=torch.complex64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    for i in range(n):
        f.filt_into_async(ys[i], xd[:, i * chunk:(i + 1) * chunk], cnt[i:i + 1])
    last = f.sync_state()
    assert f.last_kernel_name() == KERNEL                                 # the kernel takes the count from the call record
    counts = cnt.cpu().tolist()
    assert counts == [w.shape[1] for w in want] and last == counts[-1]
    for i in range(n):
        assert_bit_equal(ys[i, :, :counts[i]].cpu().numpy(), want[i], f"asynchronous call {i}")
    assert _state2(f.state) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


def test_captured_call_replayed_three_times_equals_the_synchronous_stream(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    rate, Nphi, hLen, P, chunk, n = 2.123, 32, 250, 4, 96, 5            # chunk >= historyLen (7)
    H, x = _signal(22, hLen, chunk * n, np.complex64, np.float32)
    want, state, hist = _sync_stream(pkg, monkeypatch, H, rate, Nphi, P, x, chunk, n)
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
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
    assert f.last_kernel_name() == KERNEL
    assert _state2(f.state) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


def test_chained_call_behind_a_decimator(pkg, monkeypatch, torch_cuda):
    """filt_into_async(..., after=prev): the input length of the bank filter's call is the decimator's count, on the device.  Against
    the two filters called synchronously by hand, piece by piece."""
    torch = torch_cuda
    rate, Nphi, hLen, P = 2.123, 32, 250, 4
    sizes = [1001, 17, 2000]
    H, x = _signal(23, hLen, sum(sizes), np.complex64, np.float32)
    h1 = np.random.default_rng(24).standard_normal(16).astype(np.float32)
    xd = torch.from_numpy(np.array(x)).cuda()
    s1 = pkg.FIRFilter(h1, Fraction(1, 4)).bind(np.float32, NCH)
    s2 = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
    want, pos = [], 0
    for s in sizes:
        want.append(s2.filt(s1.filt(xd[:, pos:pos + s].contiguous())).cpu().numpy())
        pos += s
    state, hist = _state2(s2.state), s2.history
    s1.close(), s2.close()
    f1 = pkg.FIRFilter(h1, Fraction(1, 4)).bind(np.float32, NCH)
    f2 = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
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
    assert f2.last_kernel_name() == KERNEL
    counts = cnt.cpu().tolist()
    assert counts == [w.shape[1] for w in want]
    for i in range(len(sizes)):
        assert_bit_equal(outs[i][:, :counts[i]].cpu().numpy(), want[i], f"chained call {i}")
    f2.sync_state()
    assert _state2(f2.state) == state
    assert_bit_equal(f2.history, hist, "history after the chained calls")
    f1.close(), f2.close()


# ---- 7. accessors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [np.complex64, np.complex128], ids=lambda t: np.dtype(t).name)
def test_pnfb_tapsforphase_and_reset(pkg, monkeypatch, th):
    rate, Nphi, hLen, P, x_len = 0.47, 4, 30, 3, 300
    H, x = _signal(31, hLen, x_len, th, np.float32)
    refs = [_restated(pkg, H[c], rate, Nphi, P, np.float32) for c in range(NCH)]
    f = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
    pn = f.pnfb()
    assert pn.shape == (NCH, f.tapsPerPhi, P + 1) and pn.dtype == np.complex128
    for c in range(NCH):
        assert_bit_equal(pn[c], refs[c].pnfb, f"pnfb of channel {c} == the per-component fit of row {c}, stored in the tap type")
    for phase in (0.0, 1.25, Nphi + 1.0):
        t = f.tapsforphase(phase)
        assert t.shape == (NCH, f.tapsPerPhi) and t.dtype == np.dtype(th)
        for c in range(NCH):
            assert_bit_equal(t[c], refs[c].tapsforphase(phase), f"tapsforphase({phase}) of channel {c}")
    for bad in (-0.5, Nphi + 1.5):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.tapsforphase(bad)
        assert e.value.code == 1
    want = np.stack([r.filt(x[c], scalar=False) for c, r in enumerate(refs)])
    assert_bit_equal(f.filt(np.array(x)), want, "first run")
    f.reset()
    st = f.state
    assert _state2(st) == (1, 1.0) and not f.history.any()
    assert_bit_equal(f.filt(np.array(x)), want, "reset, then the same again")
    f.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------
def test_buffer_too_small_wrong_channel_count_fused_and_the_c_abi_errors(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    lib = pkg.load_library()
    F32, F64, C64, C128 = 0, 1, 2, 3
    H, x = _signal(33, 8, 100, np.complex64, np.float32)
    f = _filter(pkg, monkeypatch, H, 1.5, 4, 2, np.float32)
    xd = torch.from_numpy(np.array(x)).cuda()
    small = torch.zeros((NCH, 10), dtype=torch.complex64, device="cuda")
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.filt_into(small, xd)                                          # buffer too small: the state stays
    assert e.value.code == 2
    assert _state2(f.state) == (1, 1.0) and not f.history.any()
    want = np.stack([_restated(pkg, H[c], 1.5, 4, 2, np.float32).filt(x[c], scalar=False) for c in range(NCH)])
    assert_bit_equal(f.filt(xd).cpu().numpy(), want, "the same call with room")
    assert lib.mrhip_set_numerics(f._handle, 1) == 5                    # FUSED: no fused form is defined
    assert lib.mrhip_set_numerics(f._handle, 0) == 0
    f.close()
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps_farrow(H, 1.5, 4, 2).bind(np.float32, NCH + 1)
    assert e.value.code == 1
    sentinel = 0xDEAD
    out = C.c_void_p(sentinel)
    for th, hh in ((F32, np.array(H).real.astype(np.float32)), (F64, np.array(H).real.astype(np.float64))):    # real taps: the real-tap entry
        out.value = sentinel
        rc = lib.mrhip_create_farrow_bank_ctaps(hh.ctypes.data_as(C.c_void_p), H.shape[1], th, 1.5, 4, 2, F32, NCH, 0, C.byref(out))
        assert rc == 1 and not out.value
        assert "mrhip_create_farrow_bank" in lib.mrhip_last_error().decode()
    for th, hh in ((C64, np.array(H)), (C128, np.array(H).astype(np.complex128))):
        p = hh.ctypes.data_as(C.c_void_p)
        out.value = sentinel
        rc = lib.mrhip_create_farrow_bank(p, H.shape[1], th, 1.5, 4, 2, F32, NCH, 0, C.byref(out))             # the older entry: as before
        assert rc == 5 and not out.value
        assert "left out" in lib.mrhip_last_error().decode()
        for P in (4, 5, 33, -1):                                        # polyorder >= Nphi, > 32, < 0
            out.value = sentinel
            assert lib.mrhip_create_farrow_bank_ctaps(p, H.shape[1], th, 1.5, 4, P, F32, NCH, 0, C.byref(out)) == 1 and not out.value
        for rate in (0.0, -1.0):
            out.value = sentinel
            assert lib.mrhip_create_farrow_bank_ctaps(p, H.shape[1], th, rate, 4, 2, F32, NCH, 0, C.byref(out)) == 1 and not out.value
        out.value = sentinel
        assert lib.mrhip_create_farrow_bank_ctaps(p, H.shape[1], th, 1.5, 0, 0, F32, NCH, 0, C.byref(out)) == 1 and not out.value   # bad Nphi
        out.value = sentinel
        assert lib.mrhip_create_farrow_bank_ctaps(p, H.shape[1], th, 1.5, 4, 2, F32, 0, 0, C.byref(out)) == 1 and not out.value     # no channel
        out.value = sentinel
        assert lib.mrhip_create_farrow_bank_ctaps(None, H.shape[1], th, 1.5, 4, 2, F32, NCH, 0, C.byref(out)) == 1 and not out.value


# ---- 9. neighbours -----------------------------------------------------------------------------------------------------------
def test_cascade_takes_such_a_stage_through_the_per_stage_calls(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    H, x = _signal(41, 250, 3000, np.complex64, np.float32)
    h2 = np.random.default_rng(42).standard_normal(16).astype(np.float32)
    xd = torch.from_numpy(np.array(x)).cuda()
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    make = lambda: pkg.FIRFilter.per_channel_complex_taps_farrow(H, 2.123, 32, 4)
    a, b = make(), pkg.FIRFilter(h2, Fraction(1, 2))
    by_hand = b.filt(a.filt(xd))
    cas = pkg.FilterCascade(make(), pkg.FIRFilter(h2, Fraction(1, 2)))
    y = cas.filt(xd)
    assert cas.stages[0].last_kernel_name() == KERNEL and y.dtype == torch.complex64
    assert_bit_equal(y.cpu().numpy(), by_hand.cpu().numpy(), "cascade == by hand")
    cas.close(), a.close(), b.close()


def test_filt_multi_with_such_a_filter_equals_the_single_calls(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    rate, Nphi, hLen, P, x_len = 2.123, 32, 250, 4, 400
    H, x = _signal(43, hLen, x_len, np.complex64, np.float32)
    xd = torch.from_numpy(np.array(x)).cuda()
    single = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
    want = single.filt(xd).cpu().numpy()
    single.close()
    assert_bit_equal(want, np.stack([_restated(pkg, H[c], rate, Nphi, P, np.float32).filt(x[c], scalar=False) for c in range(NCH)]), "single call")
    bank = _filter(pkg, monkeypatch, H, rate, Nphi, P, np.float32)
    plain = pkg.FIRFilter.complex_taps_farrow(np.array(H[0]), rate, Nphi, P)
    ys = pkg.filt_multi([bank, plain], [xd, xd[0].contiguous()])
    assert_bit_equal(ys[0].cpu().numpy(), want, "the bank filter's stream")
    assert_bit_equal(ys[1].cpu().numpy().reshape(-1), want[0], "the other stream")
    assert bank.last_kernel_name() == KERNEL
    bank.close(), plain.close()


def test_ring_is_not_resident(pkg, monkeypatch):
    H, _ = _signal(44, 250, 8, np.complex64, np.float32)
    f = _filter(pkg, monkeypatch, H, 2.123, 32, 4, np.float32)
    with f.open_ring() as ring:
        assert ring.info()["resident"] is False
    f.close()
