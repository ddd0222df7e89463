"""GPU tests of FIRFarrow with complex taps (csrc/kernels_ctaps_farrow.hip; mrhip_create_farrow_ctaps,
mrhip_create_farrow_pnfb_ctaps, FIRFilter.complex_taps_farrow).

Bar: farrow_ctaps_tiled_kernel (MRHIP_CTAPS_TILED=1) == farrow_ctaps_generic_kernel (MRHIP_CTAPS_TILED=0) ==
tests/complex_taps_farrow_restatement.py, BIT FOR BIT -- outputs, per-call counts, end state and history -- and, for real
samples, == the untouched oracle by components (re(y) / im(y) are its outputs with the banks real(pnfb) / imag(pnfb)).  The
restatement itself is pinned to the oracle by tests/test_complex_taps_farrow_cpu.py.  All sides get the SAME coefficients
(mrhip_create_farrow_pnfb_ctaps): the reference pins no bits of the fit.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_farrow_restatement import ComplexTapsFarrowRestated, fit_pnfb
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NCH = 3
TYPES = [(np.complex64, np.float32), (np.complex128, np.float64), (np.complex64, np.complex64), (np.complex64, np.complex128),
         (np.complex128, np.complex64)]
RATES = [0.47, 1.0, 2.123, 32.0 / 3]
# (Nphi, hLen, polyorder): T = 1 (no history); a constant polynomial; polyorder = Nphi - 1; T = 8; T = 32; T = 33
BANKS = [(4, 4, 2), (4, 30, 0), (4, 30, 3), (32, 250, 4), (32, 1024, 4), (8, 264, 2)]
X_LENS = [1, 5, 257, 1500]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
GENERIC, TILED = "farrow_ctaps_generic_kernel", "farrow_ctaps_tiled_kernel"


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


_BANK_CACHE = {}


def _bank(pkg, Nphi, hLen, polyorder, th):
    """complex taps and their per-component fit (mrhip_polyfit), computed once per bank and tap type"""
    key = (Nphi, hLen, polyorder, np.dtype(th).name)
    if key not in _BANK_CACHE:
        rng = np.random.default_rng(1000 * Nphi + hLen + polyorder)
        h = ((rng.standard_normal(hLen) + 1j * rng.standard_normal(hLen)) / hLen).astype(th)
        _BANK_CACHE[key] = (h, fit_pnfb(h, Nphi, polyorder, pkg.polyfit))
    return _BANK_CACHE[key]


def _samples(seed, x_len, tx, nch=NCH):
    rng = np.random.default_rng(seed)
    x = rng.random((nch, x_len)) - 0.5
    if np.dtype(tx).kind == "c":
        x = x + 1j * (rng.random((nch, x_len)) - 0.5)
    return x.astype(tx)


def _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, tx, nch, tiled):
    """a bound filter on the tiled kernel wherever its LDS plan fits (MRHIP_CTAPS_TILED=1) or on the universal one (=0)"""
    monkeypatch.setenv("MRHIP_FORCE_GENERIC", "0")
    monkeypatch.setenv("MRHIP_CTAPS_TILED", "1" if tiled else "0")
    return pkg.FIRFilter.complex_taps_farrow(h, rate, Nphi, polyorder, pnfb=pnfb).bind(tx, nch)


def _restated(h, rate, Nphi, polyorder, pnfb, tx):
    return ComplexTapsFarrowRestated(len(h), h.dtype, rate, Nphi, polyorder, pnfb, tx=tx)


def _oracle_by_components(O, h, rate, Nphi, polyorder, pnfb, x):
    """real samples: per channel, the oracle's outputs with the banks real(pnfb) and imag(pnfb) (rounded to the tap type as the
    library stores them), put together"""
    rt = np.float32 if h.dtype == np.complex64 else np.float64
    hr = np.zeros(len(h), dtype=rt)
    pr = np.ascontiguousarray(pnfb.real).astype(rt).astype(np.float64)
    pi = np.ascontiguousarray(pnfb.imag).astype(rt).astype(np.float64)
    out = []
    for c in range(x.shape[0]):
        yr = O.FIRFilter(hr, rate, Nphi, tx=x.dtype, polyorder=polyorder, pnfb=pr).filt(x[c])
        yi = O.FIRFilter(hr, rate, Nphi, tx=x.dtype, polyorder=polyorder, pnfb=pi).filt(x[c])
        y = np.empty(len(yr), dtype=np.complex64 if yr.dtype == np.float32 else np.complex128)
        y.real, y.imag = yr, yi
        out.append(y)
    return np.stack(out)


# ---- 1. shape sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th,tx", TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("rate", RATES)
def test_shape_sweep_tiled_equals_universal_equals_restatement(pkg, monkeypatch, rate, th, tx):
    want_dtype = np.complex128 if (th == np.complex128 or np.dtype(tx) in (np.float64, np.complex128)) else np.complex64
    for Nphi, hLen, polyorder in BANKS:
        h, pnfb = _bank(pkg, Nphi, hLen, polyorder, th)
        for x_len in X_LENS:
            x = _samples(hLen + x_len, x_len, tx)
            for name, how in CHUNKINGS.items():
                pieces = _chunks(x_len, how)
                refs = [_restated(h, rate, Nphi, polyorder, pnfb, tx) for _ in range(NCH)]
                want = [[r.filt(x[c, a:b], scalar=False) for a, b in pieces] for c, r in enumerate(refs)]
                for tiled in (False, True):
                    what = f"Nphi {Nphi} hLen {hLen} polyorder {polyorder} x_len {x_len} {name} tiled={tiled}"
                    f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, tx, NCH, tiled)
                    assert f.output_dtype == want_dtype
                    for i, (a, b) in enumerate(pieces):
                        y = f.filt(np.ascontiguousarray(x[:, a:b]))
                        assert y.dtype == want_dtype and y.shape == (NCH, len(want[0][i])), (what, a, b, y.shape)
                        for c in range(NCH):
                            assert_bit_equal(y[c], want[c][i], f"{what} chunk [{a}, {b}) channel {c}")
                        if y.shape[1] > 0:
                            assert f.last_kernel_name() == (TILED if tiled else GENERIC), what
                    st = f.state
                    assert st.kind == 5 and st.tap_dtype == (3 if th == np.complex128 else 2)
                    assert (st.inputDeficit, st.phiAccumulator) == (refs[0].inputDeficit, refs[0].phiAccumulator), what
                    hist = f.history.reshape(NCH, -1)
                    assert hist.dtype == np.dtype(tx)
                    for c in range(NCH):
                        assert_bit_equal(hist[c], refs[c].history_array(), f"{what} history {c}")
                    f.close()


# ---- 2. signed zeros at the seam -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.float64)], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("tiled", [False, True])
def test_signed_zeros_at_the_seam(pkg, monkeypatch, tiled, th, tx):
    """x all -0.0 with positive taps: outputs with xIdx < tapsPer𝜙 are +0.0, later ones -0.0, per component.  With the default
    history (+0.0) and -- the only place the start-from-zero rule itself shows -- with a history of -0.0, where every product of
    a seam output is -0.0 and only `0 + p` makes it +0.0."""
    Nphi, T, n = 4, 3, 300                                     # (two tiles)
    h = np.full(Nphi * T, 1 + 2j, dtype=th)
    pnfb = np.full((T, 1), 1 + 2j)
    x = np.full((2, n), -0.0, dtype=tx)
    for neg_history in (False, True):
        f = _filter(pkg, monkeypatch, h, 1.0, Nphi, 0, pnfb, tx, 2, tiled)
        r = _restated(h, 1.0, Nphi, 0, pnfb, tx)
        if neg_history:
            f.set_history(np.full((2, T - 1), -0.0, dtype=tx))
            r.history = [(r.R(-0.0),)] * (T - 1)
        y = f.filt(x)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert y.shape == (2, n) and not y.any()
        for c in range(2):
            for part in (y[c].real, y[c].imag):
                assert list(np.signbit(part)) == [False] * (T - 1) + [True] * (n - T + 1), (neg_history, c)
        assert_bit_equal(y[0], r.filt(x[0], scalar=False), "restatement")
        f.close()


# ---- 3. a tile whose run exceeds the planned span ----------------------------------------------------------------------------------
def test_over_span_tiles_read_global_memory_and_equal_the_universal_kernel_and_the_oracle(pkg, O, monkeypatch):
    """rate 1/50: a full tile of 256 outputs runs over 12 750 samples, more than the 40 KiB of samples the plan gives a tile
    (10 240 Float32 samples): the three full tiles read their windows from global memory, the last (32 outputs) is staged"""
    rate, Nphi, hLen, polyorder, x_len, nch = 1.0 / 50, 32, 250, 4, 40_000, 2
    h, pnfb = _bank(pkg, Nphi, hLen, polyorder, np.complex64)
    x = _samples(7, x_len, np.float32, nch=nch)
    ys = {}
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, np.float32, nch, tiled)
        ys[tiled] = f.filt(x)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        ys[tiled, "hist"], ys[tiled, "state"] = f.history, (f.state.inputDeficit, f.state.phiAccumulator)
        f.close()
    assert ys[True].shape == (nch, 800)
    assert_bit_equal(ys[True], ys[False], "tiled == universal")
    assert_bit_equal(ys[True, "hist"], ys[False, "hist"], "history")
    assert ys[True, "state"] == ys[False, "state"]
    assert_bit_equal(ys[True], _oracle_by_components(O, h, rate, Nphi, polyorder, pnfb, x), "oracle by components")


# ---- 4. channel groups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 5, 9, 33])
def test_channel_groups_every_cpl_and_a_ragged_last_group(pkg, O, monkeypatch, nch):
    rate, Nphi, hLen, polyorder, x_len = 2.123, 32, 250, 4, 1000
    h, pnfb = _bank(pkg, Nphi, hLen, polyorder, np.complex64)
    x = _samples(50 + nch, x_len, np.float32, nch=nch)
    want = _oracle_by_components(O, h, rate, Nphi, polyorder, pnfb, x)
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, np.float32, nch, tiled)
        y = f.filt(x).reshape(nch, -1)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert_bit_equal(y, want, f"{nch} channels, tiled={tiled}")
        f.close()


# ---- 5. a call that mrhip_filt_device splits into pieces ------------------------------------------------------------------------------
def test_split_call_places_every_piece_by_the_output_element_size_and_only_the_first_has_a_seam(pkg, O, monkeypatch, torch_cuda):
    """MRHIP_LAUNCH_MAX=4099: eight pieces; real samples and a complex output -- a y offset taken in sample-size units would put
    every piece after the first at half its place.  Then the same call over -0.0 samples behind a -0.0 history: +0.0 where
    xIdx < tapsPer𝜙 in the CALL, -0.0 everywhere else -- a continuation piece takes no seam."""
    torch = torch_cuda
    rate, Nphi, hLen, polyorder, x_len, nch = 1.37, 32, 250, 4, 30_011, 2
    h, pnfb = _bank(pkg, Nphi, hLen, polyorder, np.complex64)
    x = _samples(9, x_len, np.float32, nch=nch)
    want = _oracle_by_components(O, h, rate, Nphi, polyorder, pnfb, x)
    xd = torch.from_numpy(x).cuda()
    monkeypatch.setenv("MRHIP_LAUNCH_MAX", "4099")
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, np.float32, nch, tiled)
        y = f.filt(xd).cpu().numpy()
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert_bit_equal(y, want, f"split call, tiled={tiled}")
        assert_bit_equal(f.history.reshape(nch, -1)[1], x[1, -(f.historyLen):], "history")
        f.close()
    T = 8
    ones = np.full((T, 1), 1 + 2j)
    hz = np.full(Nphi * T, 1 + 2j, dtype=np.complex64)
    xz = torch.full((nch, x_len), -0.0, dtype=torch.float32, device="cuda")
    for tiled in (True, False):
        f = _filter(pkg, monkeypatch, hz, 1.0, Nphi, 0, ones, np.float32, nch, tiled)
        f.set_history(np.full((nch, T - 1), -0.0, dtype=np.float32))
        y = f.filt(xz).cpu().numpy()
        assert y.shape == (nch, x_len) and not y.any()
        for part in (y.real, y.imag):
            assert not np.signbit(part[:, :T - 1]).any() and np.signbit(part[:, T - 1:]).all(), f"tiled={tiled}"
        f.close()


# ---- 6. asynchronous and captured calls -------------------------------------------------------------------------------------
def _sync_stream(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, x, chunk, n):
    f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, x.dtype, x.shape[0], tiled=False)
    out = [f.filt(np.ascontiguousarray(x[:, i * chunk:(i + 1) * chunk])).reshape(x.shape[0], -1) for i in range(n)]
    st = f.state
    hist = f.history
    f.close()
    return out, (st.inputDeficit, st.phiAccumulator), hist


@pytest.mark.parametrize("tiled", [False, True])
def test_async_calls_equal_the_synchronous_stream(pkg, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, polyorder, chunk, n = 2.123, 32, 250, 4, 96, 5
    h, pnfb = _bank(pkg, Nphi, hLen, polyorder, np.complex64)
    x = _samples(21, chunk * n, np.complex64)
    want, state, hist = _sync_stream(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, x, chunk, n)
    f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, np.complex64, NCH, tiled)
    xd = torch.from_numpy(x).cuda()
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
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == state
    assert_bit_equal(f.history, hist, "history after the asynchronous calls")
    f.close()


@pytest.mark.parametrize("tiled", [False, True])
def test_captured_call_replayed_three_times_equals_the_synchronous_stream(pkg, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    rate, Nphi, hLen, polyorder, chunk, n = 2.123, 32, 250, 4, 96, 5   # chunk >= historyLen (7)
    h, pnfb = _bank(pkg, Nphi, hLen, polyorder, np.complex64)
    x = _samples(22, chunk * n, np.complex64)
    want, state, hist = _sync_stream(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, x, chunk, n)
    f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, np.complex64, NCH, tiled)
    xd = torch.from_numpy(x).cuda()
    # The stream starts with a plain call and an asynchronous one of the captured size: the schedule's work buffers are allocated
    # by the first device-planned call of a size (allocations cannot be captured).  The graph takes the stream over from there.
    assert_bit_equal(f.filt(xd[:, :chunk].contiguous()).cpu().numpy(), want[0], "plain call")
    bound = f.outputlength_bound(chunk)
    y1 = torch.zeros((NCH, bound), dtype=torch.complex64, device="cuda")
    f.filt_into_async(y1, xd[:, chunk:2 * chunk])
    c1 = f.sync_state()
    assert_bit_equal(y1[:, :c1].cpu().numpy(), want[1], "asynchronous call of the captured size")
    xs = torch.zeros((NCH, chunk), dtype=torch.complex64, device="cuda")
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
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == state
    assert_bit_equal(f.history, hist, "history after the replays")
    f.close()


# ---- 7. tapsforphase, get_pnfb, the library's own fit, reset -----------------------------------------------------------------
@pytest.mark.parametrize("th", [np.complex64, np.complex128])
def test_tapsforphase_get_pnfb_own_fit_and_reset(pkg, monkeypatch, th):
    rate, Nphi, hLen, polyorder, x_len = 0.47, 4, 30, 2, 300
    h, pnfb = _bank(pkg, Nphi, hLen, polyorder, th)
    x = _samples(31, x_len, np.float32, nch=1)
    r = _restated(h, rate, Nphi, polyorder, pnfb, np.float32)
    f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, np.float32, 1, tiled=True)
    got = f.pnfb()
    assert got.dtype == np.complex128 and got.shape == (r.T, polyorder + 1)
    assert_bit_equal(got, r.pnfb, "pnfb as stored (rounded to the tap type per component)")
    # mrhip_create_farrow_ctaps (its own fit) == mrhip_create_farrow_pnfb_ctaps fed two mrhip_polyfit fits per row
    own = pkg.FIRFilter.complex_taps_farrow(h, rate, Nphi, polyorder).bind(np.float32, 1)
    assert_bit_equal(own.pnfb(), got, "the library's own fit")
    own.close()
    for phase in (0.0, 1.0, 1.25, Nphi + 0.5, Nphi + 1.0):
        t = f.tapsforphase(phase)
        assert t.dtype == th and t.shape == (r.T,)
        assert_bit_equal(t, r.tapsforphase(phase), f"tapsforphase({phase})")
    for bad in (-0.5, Nphi + 1.5):
        with pytest.raises(pkg.MultirateHIPError) as e:
            f.tapsforphase(bad)
        assert e.value.code == 1
    y1 = f.filt(x[0])
    assert_bit_equal(y1, r.filt(x[0], scalar=False), "first run")
    f.reset()
    st = f.state
    assert (st.inputDeficit, st.phiAccumulator) == (1, 1.0) and not f.history.any()
    assert_bit_equal(f.filt(x[0]), y1, "reset, then the same again")
    f.close()


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------
def test_contract_edges(pkg, monkeypatch, torch_cuda):
    lib = pkg.load_library()
    F32, F64, C64, C128 = 0, 1, 2, 3
    h = np.full(8, 0.5 - 0.25j, dtype=np.complex64)
    f = pkg.FIRFilter.complex_taps_farrow(h, 1.5, 4, 2).bind(np.float32, 1)
    assert lib.mrhip_set_numerics(f._handle, 1) == 5            # FUSED: no fused form is defined
    assert lib.mrhip_set_numerics(f._handle, 0) == 0
    f.close()
    out = C.c_void_p()
    coef = np.ones(2 * 3 * 2, dtype=np.float64)                 # [T = 2][polyorder + 1 = 3] pairs
    for th, hh in ((F32, h.real.astype(np.float32)), (F64, h.real.astype(np.float64))):      # real taps: the existing constructors
        assert lib.mrhip_create_farrow_ctaps(hh.ctypes.data_as(C.c_void_p), len(hh), th, 1.5, 4, 2, F32, 1, 0, C.byref(out)) == 1
        assert not out.value
        assert lib.mrhip_create_farrow_pnfb_ctaps(coef.ctypes.data_as(C.c_void_p), 8, th, 1.5, 4, 2, F32, 1, 0, C.byref(out)) == 1
        assert not out.value
    for th, hh in ((C64, h), (C128, h.astype(np.complex128))):
        p = hh.ctypes.data_as(C.c_void_p)
        assert lib.mrhip_create_farrow(p, len(hh), th, 1.5, 4, 2, F32, 1, 0, C.byref(out)) == 5 and not out.value
        assert lib.mrhip_create_farrow_pnfb(coef.ctypes.data_as(C.c_void_p), 8, th, 1.5, 4, 2, F32, 1, 0, C.byref(out)) == 5 and not out.value
        for polyorder in (4, 33):                                # polyorder > min(32, Nphi - 1)
            assert lib.mrhip_create_farrow_ctaps(p, len(hh), th, 1.5, 4, polyorder, F32, 1, 0, C.byref(out)) == 1 and not out.value
        assert lib.mrhip_create_farrow_ctaps(p, len(hh), th, 1.5, 64, 33, F32, 1, 0, C.byref(out)) == 1 and not out.value
        assert lib.mrhip_create_farrow_ctaps(p, len(hh), th, 1.5, 4, -1, F32, 1, 0, C.byref(out)) == 1 and not out.value
        for rate in (0.0, -1.0):                                 # "rate must be greater than 0"
            assert lib.mrhip_create_farrow_ctaps(p, len(hh), th, rate, 4, 2, F32, 1, 0, C.byref(out)) == 1 and not out.value
            assert lib.mrhip_create_farrow_pnfb_ctaps(coef.ctypes.data_as(C.c_void_p), 8, th, rate, 4, 2, F32, 1, 0, C.byref(out)) == 1
            assert not out.value
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.ShardedFIRFilter(h, 1.5, 2, [0], Nphi=4, polyorder=2)       # sharded filters keep refusing complex taps
    assert e.value.code == 5


# ---- 9. cascade ----------------------------------------------------------------------------------------------------------------
def test_cascade_takes_such_a_stage_through_the_per_stage_calls(pkg, monkeypatch, torch_cuda):
    """a cascade runs its stages as plain calls, so a complex-tap FIRFarrow is a stage like any FIRFarrow: Float32 in, Complex64
    between the stages, a real-tap decimator behind it == the two filters called by hand"""
    torch = torch_cuda
    h, pnfb = _bank(pkg, 32, 250, 4, np.complex64)
    x = _samples(41, 3000, np.float32, nch=2)
    h2 = np.random.default_rng(42).standard_normal(16).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    monkeypatch.setenv("MRHIP_CTAPS_TILED", "1")
    make = lambda: pkg.FIRFilter.complex_taps_farrow(h, 2.123, 32, 4, pnfb=pnfb)
    a, b = make(), pkg.FIRFilter(h2, Fraction(1, 2))
    by_hand = b.filt(a.filt(xd))
    cas = pkg.FilterCascade(make(), pkg.FIRFilter(h2, Fraction(1, 2)))
    y = cas.filt(xd)
    assert cas.stages[0].last_kernel_name() == TILED and y.dtype == torch.complex64
    assert_bit_equal(y.cpu().numpy(), by_hand.cpu().numpy(), "cascade == by hand")
    cas.close(), a.close(), b.close()


# ---- 10. known answer ------------------------------------------------------------------------------------------------------------
def test_known_answer_running_window_sum(pkg, monkeypatch):
    """h = (1+2im) * ones(Nphi * T), polyorder 0: every row of the bank is constant, its fit is the constant, so every tap of
    every phase is 1+2im.  Rate 1.0: every sample gives an output; x = 1..n: y[k] = (1+2im) * (sum of the last T samples that
    have arrived), exactly (small integers)."""
    Nphi, T, n = 4, 3, 300
    h = np.full(Nphi * T, 1 + 2j, dtype=np.complex64)
    x = np.arange(1, n + 1, dtype=np.float32)
    ext = np.concatenate([np.zeros(T - 1), x.astype(np.float64)])
    window = np.array([ext[k:k + T].sum() for k in range(n)])
    for tiled in (False, True):
        monkeypatch.setenv("MRHIP_CTAPS_TILED", "1" if tiled else "0")
        f = pkg.FIRFilter.complex_taps_farrow(h, 1.0, Nphi, 0).bind(np.float32, 1)     # (the library's own fit)
        assert np.array_equal(f.pnfb(), np.full((T, 1), 1 + 2j))
        y = f.filt(x)
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        assert y.dtype == np.complex64
        assert np.array_equal(y, (window * (1 + 2j)).astype(np.complex64)), (tiled, y[:8])
        f.close()


# ---- 11. the default rule ----------------------------------------------------------------------------------------------------------
def test_default_rule_takes_only_the_measured_shapes_and_changes_no_bit(pkg, monkeypatch):
    """MRHIP_CTAPS_TILED unset: the tiled kernel where it was measured and faster (profiles/r07/ctaps_farrow.txt: Float32 arithmetic,
    32 taps per phase, 21 000 outputs a channel and more), the universal kernel everywhere else -- the same bits either way"""
    rate, Nphi, hLen, polyorder = 2.123, 32, 1024, 4
    for th, x_len, want in ((np.complex64, 12_000, TILED), (np.complex64, 1500, GENERIC), (np.complex128, 12_000, GENERIC)):
        h, pnfb = _bank(pkg, Nphi, hLen, polyorder, th)
        x = _samples(61, x_len, np.float32, nch=2)
        f = _filter(pkg, monkeypatch, h, rate, Nphi, polyorder, pnfb, np.float32, 2, tiled=False)
        y0 = f.filt(x)
        assert f.last_kernel_name() == GENERIC
        f.close()
        monkeypatch.delenv("MRHIP_CTAPS_TILED")
        f = pkg.FIRFilter.complex_taps_farrow(h, rate, Nphi, polyorder, pnfb=pnfb).bind(np.float32, 2)
        y = f.filt(x)
        assert f.last_kernel_name() == want, (np.dtype(th).name, x_len)
        assert_bit_equal(y, y0, f"default == universal, {np.dtype(th).name} taps, {x_len} samples")
        f.close()
