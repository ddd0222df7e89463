"""GPU tests of the FIRFarrow fit on the device (include/multirate_hip.h, "The FIRFarrow fit on the device for the filters with
per-channel rates"): mrhip_set_channel_taps_farrow_device and mrhip_set_channel_ctaps_farrow_device (rates_farrow_fit_kernel,
csrc/kernels_rates_farrow_fit.hip), through FIRFilter.set_channel_taps_farrow_device / .set_channel_ctaps_farrow_device and ctypes.

Bar: everything is BIT FOR BIT, no tolerance anywhere.  The banks a device call fits are those of the host call with the same matrix
and those of the one-channel filters; after a device install every channel is its one-channel filter (outputs, counts, end state,
history) through the plain call, the ragged call and the device-lengths call, on the universal and the multi kernels; a loop of filter
call, taps derived from the outputs by torch ON the device, device fit, new rates, filter call equals piece by piece the twin driven
through the host calls with the same values, and one-channel filters rebuilt per piece; refusals change nothing; host and device
installs mix, reset() keeps what the device installed, a first call on a shared bank allocates once (the device's free memory around
three calls); every bank receives its own coefficients (that no lane writes outside the banks is the stand-alone program's case, which
runs the kernel's index maps over a guard-padded buffer: tests/test_rates_farrow_fit_device_cpu.py).  The one-channel filters are the
library's own (FIRFilter(h, rate, Nphi, polyorder), FIRFilter.complex_taps_farrow), which tests/test_gpu_parity.py and
tests/test_gpu_complex_taps_farrow.py hold to the oracle.  The shapes are the smallest at which this can go wrong.
"""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_rates_bank_farrow as FB
from conftest import assert_bit_equal
from test_gpu_rates_farrow import R3, R4, R67, _check_end, _chunks, _state5, _tt

pytestmark = pytest.mark.gpu

CGENERIC, CMULTI = "farrow_rates_ctaps_generic", "farrow_rates_ctaps_multi"
PHASES = (1.0, 2.375)
# (Nphi, hLen, polyorder): T = 1; zero padding and m = n (exact interpolation); the division path; the measured shape; 32 taps a phase;
# and one shape on the far side of each boundary of the launch plan (32, 16 and 8 lanes a workgroup; Nphi = 1024 is the bound: blocks of 8
# threads and exactly 64 KiB of LDS), T = 2
SHAPES = [(4, 4, 1), (4, 30, 3), (3, 40, 2), (32, 250, 4), (32, 1024, 4), (160, 320, 3), (512, 1024, 4), (1024, 2048, 4)]
TAPS = [np.float32, np.float64, np.complex64, np.complex128]
PIECES = [0, 1, 5, 64]                                      # ... and the rest of 400 samples
X_LEN = 400


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


_SIGNALS = {}


def _signal(seed, Nphi, hLen, x_len, th, tx, nch):
    """one tap vector per channel (about unit gain per phase; a full mantissa each), all different, and one row of samples per channel"""
    key = (seed, Nphi, hLen, x_len, np.dtype(th).name, np.dtype(tx).name, nch)
    if key not in _SIGNALS:
        rng = np.random.default_rng(seed)
        H = rng.standard_normal((nch, hLen)) * Nphi / max(hLen, 1)
        if np.dtype(th).kind == "c":
            H = H + 1j * rng.standard_normal((nch, hLen)) * Nphi / max(hLen, 1)
        H = H.astype(th)
        x = (rng.random((nch, x_len)) - 0.5).astype(tx)
        assert len({H[c].tobytes() for c in range(nch)}) == nch
        H.setflags(write=False), x.setflags(write=False)
        _SIGNALS[key] = (H, x)
    return _SIGNALS[key]


def _env(monkeypatch, multi):
    FB._env(monkeypatch, multi)
    monkeypatch.setenv("MRHIP_FARROW_RATES_CTAPS_MULTI", "1")


def _rates_filter(pkg, H, rates, Nphi, P, tx, fused=False):
    """the filter the updates are made on: ONE shared bank fitted from another tap vector (row 0's real part)"""
    numerics = pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT
    return pkg.FIRFilter.per_channel_rates_farrow(np.ascontiguousarray(np.array(H[0]).real), rates, Nphi, P, numerics=numerics).bind(tx, len(rates))


def _one_channel(pkg, h, rate, Nphi, P, tx, fused=False):
    if np.dtype(h.dtype).kind == "c":
        return pkg.FIRFilter.complex_taps_farrow(np.array(h), float(rate), Nphi, P).bind(tx, 1)
    return pkg.FIRFilter(np.array(h), float(rate), Nphi, P, numerics=pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT).bind(tx, 1)


def _install(f, torch, H, device=True):
    cplx = np.dtype(H.dtype).kind == "c"
    if device:
        (f.set_channel_ctaps_farrow_device if cplx else f.set_channel_taps_farrow_device)(_dev(torch, H))
    else:
        (f.set_channel_ctaps_farrow if cplx else f.set_channel_taps_farrow)(np.array(H))


def _queries(f):
    return (f.pnfb(),) + tuple(f.tapsforphase(p) for p in PHASES)


def _assert_rows_equal(ya, yb, what):
    """filt of a filter with per-channel rates: one tensor per channel"""
    assert len(ya) == len(yb), what
    for c, (ra, rb) in enumerate(zip(ya, yb)):
        assert_bit_equal(ra.cpu().numpy(), rb.cpu().numpy(), f"{what}: channel {c}")


# ---- banks as fitted ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", TAPS, ids=[np.dtype(t).name for t in TAPS])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}p{s[2]}" for s in SHAPES])
def test_the_banks_are_those_of_the_host_call_and_of_the_one_channel_filters(pkg, monkeypatch, torch_cuda, shape, th):
    """3 channels, and 67 (several waves of the fit kernel and a partial last one); two installs each: the first allocates the banks and
    uploads the fit's table, the second reuses both"""
    torch = torch_cuda
    Nphi, hLen, P = shape
    tx, T = np.float32, -(-hLen // Nphi)
    cplx = np.dtype(th).kind == "c"
    _env(monkeypatch, False)
    for nch, rates in ((3, R3), (67, R67)):
        f, twin = None, None
        for k in range(2):
            H, _ = _signal(9000 + 10 * Nphi + hLen + k, Nphi, hLen, 8, th, tx, nch)
            if f is None:
                f, twin = _rates_filter(pkg, H, rates, Nphi, P, tx), _rates_filter(pkg, H, rates, Nphi, P, tx)
            _install(f, torch, H), _install(twin, torch, H, device=False)
            got, want = _queries(f), _queries(twin)
            assert got[0].shape == (nch, T, P + 1) and got[0].dtype == (np.complex128 if cplx else np.float64) and got[1].shape == (nch, T)
            for g, w, name in zip(got, want, ("pnfb",) + tuple(f"tapsforphase({p})" for p in PHASES)):
                assert g.dtype == w.dtype
                assert_bit_equal(g, w, f"nch {nch} install {k}: {name}, device fit against host fit")
            assert len({got[0][c].tobytes() for c in range(nch)}) == nch                      # every channel has a bank of its own
            for c in range(nch) if nch == 3 else (0, 1, 33, 65, 66):
                one = _one_channel(pkg, H[c], rates[c], Nphi, P, tx)
                assert_bit_equal(got[0][c], one.pnfb(), f"nch {nch} install {k}: bank of channel {c} against the one-channel filter")
                one.close()
        assert f.output_dtype == twin.output_dtype == np.dtype(np.result_type(th, tx))
        f.close(), twin.close()


# ---- every channel is its one-channel filter ----------------------------------------------------------------------------------------
KINDS = {"real-strict": (np.float32, False), "real-fused": (np.float32, True), "complex-strict": (np.complex64, False)}
_REFS = {}


def _one_channel_reference(pkg, torch, kind, rates, Nphi, hLen, P, tx, pieces):
    """per channel, the one-channel filter of (H[c], rates[c]) fed x[c] in `pieces`: (outputs [c][piece], end states, histories); once
    per (kind, rates), shared by the kernels and the call paths"""
    key = (kind, tuple(rates))
    if key not in _REFS:
        th, fused = KINDS[kind]
        H, x = _signal(9500 + len(rates), Nphi, hLen, X_LEN, th, tx, len(rates))
        xd = _dev(torch, x)
        outs, states, hists = [], [], []
        for c, r in enumerate(rates):
            one = _one_channel(pkg, H[c], r, Nphi, P, tx, fused)
            empty = np.zeros(0, dtype=one.output_dtype)                       # (a piece of no samples moves nothing)
            outs.append([one.filt(xd[c, a:b]).cpu().numpy() if b > a else empty for a, b in pieces])
            states.append(_state5(one.state)), hists.append(np.array(one.history))
            one.close()
        _REFS[key] = (outs, states, hists)
    return _REFS[key]


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
@pytest.mark.parametrize("rates", [R4, R67], ids=["R4", "nch67"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_channel_is_its_one_channel_filter(pkg, monkeypatch, torch_cuda, kind, rates, multi):
    torch = torch_cuda
    Nphi, hLen, P, tx = 32, 250, 4, np.float32
    th, fused = KINDS[kind]
    nch = len(rates)
    pieces = _chunks(X_LEN, PIECES)
    assert pieces == [(0, 0), (0, 1), (1, 6), (6, 70), (70, 400)]
    H, x = _signal(9500 + nch, Nphi, hLen, X_LEN, th, tx, nch)
    xd = _dev(torch, x)
    outs, states, hists = _one_channel_reference(pkg, torch, kind, rates, Nphi, hLen, P, tx, pieces)
    _env(monkeypatch, multi)
    name = (CMULTI if multi else CGENERIC) if np.dtype(th).kind == "c" else (FB.MULTI if multi else FB.GENERIC)
    for through in ("plain", "ragged", "device lengths"):
        f = _rates_filter(pkg, H, rates, Nphi, P, tx, fused)
        _install(f, torch, H)                                               # before the first call: the shared bank never filters
        out_dtype = _tt(torch, f.output_dtype)
        for i, (a, b) in enumerate(pieces):
            what = f"{kind} nch {nch} {through} piece {i} [{a}, {b})"
            y = torch.zeros((nch, f.outputlength_bound(b - a)), dtype=out_dtype, device="cuda")
            if through == "plain":
                counts = f.filt_into(y, xd[:, a:b])
            elif through == "ragged":
                counts = f.filt_into(y, xd[:, a:b], lengths=[b - a] * nch)
            else:
                lens = torch.full((nch,), b - a, dtype=torch.int64, device="cuda")
                counts = f.filt_rates_async(y, xd[:, a:b], lengths=lens, max_length=b - a).cpu().numpy()
            want = [len(outs[c][i]) for c in range(nch)]
            assert list(counts) == want, (what, list(counts), want)
            yh = y.cpu().numpy()
            for c in range(nch):
                assert_bit_equal(yh[c, :want[c]], outs[c][i], f"{what}: channel {c}")
            if b > a:
                assert f.last_kernel_name() == name, what
        _check_end(f, states, hists, f"{kind} nch {nch} {through}")
        f.close()


# ---- a loop that never meets the host -----------------------------------------------------------------------------------------------
LOOP_LO, LOOP_HI = 0.009, 12.0


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_a_loop_that_never_meets_the_host(pkg, monkeypatch, torch_cuda, multi):
    """four rounds of: filter; new taps derived from the round's outputs by torch ops on the device (a stand-in for a block-LMS step);
    set_channel_taps_farrow_device; set_channel_rates_device; and the next round filters with them.  Nothing is read back before the
    loop is over.  Then: the twin driven through the host calls with the same values, and one-channel filters rebuilt per piece."""
    torch = torch_cuda
    Nphi, hLen, P, nch, tx, n = 32, 250, 4, 4, np.float32, 150
    H0, x = _signal(9600, Nphi, hLen, 4 * n, np.float32, tx, nch)
    pieces = _chunks(4 * n, n)
    xd, base_r = _dev(torch, x), _dev(torch, np.array(R4, dtype=np.float64))
    _env(monkeypatch, multi)
    f = _rates_filter(pkg, H0, R4, Nphi, P, tx)
    H_d, rates_d = _dev(torch, H0), base_r
    f.set_channel_taps_farrow_device(H_d)                                   # (the first install allocates and waits once)
    f.set_channel_rates_device(rates_d, LOOP_LO, LOOP_HI)
    kept, ys, cnts = [], [], []
    for i, (a, b) in enumerate(pieces):
        y = torch.zeros((nch, f.outputlength_bound(b - a)), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(nch, dtype=torch.int64, device="cuda")
        f._filt_into_rates(y, xd[:, a:b], counts=cnt)                       # (returns without waiting; the counts stay on the device)
        kept.append((rates_d, H_d)), ys.append(y), cnts.append(cnt)
        err = y[:, :hLen] if y.shape[1] >= hLen else torch.nn.functional.pad(y, (0, hLen - y.shape[1]))
        H_d = (H_d * (1.0 - 0.01 * (i + 1)) + 0.003 * torch.roll(err, shifts=i + 1, dims=-1)).contiguous()     # taps from the outputs
        rates_d = (base_r * (1.0 + 0.002 * (i + 1))).contiguous()
        assert H_d.dtype == torch.float32 and H_d.shape == (nch, hLen)
        f.set_channel_taps_farrow_device(H_d)
        f.set_channel_rates_device(rates_d, LOOP_LO, LOOP_HI)
    assert f.last_kernel_name() == (FB.MULTI if multi else FB.GENERIC)
    values = [(r.cpu().numpy(), h.cpu().numpy()) for r, h in kept]        # only now does the host learn anything
    last_H = H_d.cpu().numpy()
    got = [(y.cpu().numpy(), c.cpu().numpy()) for y, c in zip(ys, cnts)]
    assert len({h.tobytes() for _, h in values}) == len(pieces)
    twin = _rates_filter(pkg, H0, R4, Nphi, P, tx)
    ones = [None] * nch
    for i, (a, b) in enumerate(pieces):
        twin.set_channel_taps_farrow(values[i][1])
        twin.set_channel_rates(values[i][0])
        yt = torch.zeros((nch, twin.outputlength_bound(b - a)), dtype=torch.float32, device="cuda")
        counts = twin.filt_into(yt, xd[:, a:b])
        assert list(got[i][1]) == list(counts), (i, list(got[i][1]), list(counts))
        yth = yt.cpu().numpy()
        for c in range(nch):
            assert_bit_equal(got[i][0][c, :counts[c]], yth[c, :counts[c]], f"piece {i}, channel {c}: device calls against host calls")
            new = _one_channel(pkg, values[i][1][c], values[i][0][c], Nphi, P, tx)       # rebuilt per piece, state and history handed over
            if ones[c] is not None:
                st = ones[c].state
                new.set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
                new.set_history(np.array(ones[c].history))
                ones[c].close()
            ones[c] = new
            want = new.filt(xd[c, a:b]).cpu().numpy()
            assert counts[c] == len(want), (i, c)
            assert_bit_equal(got[i][0][c, :counts[c]], want, f"piece {i}, channel {c}: against the one-channel filter rebuilt for the piece")
    fs, ts = f.channel_states, twin.channel_states
    assert [_state5(s) + (s.last_count,) for s in fs] == [_state5(s) + (s.last_count,) for s in ts]
    assert [_state5(s)[:4] for s in fs] == [_state5(o.state)[:4] for o in ones]
    assert_bit_equal(f.history, twin.history, "history after the loop")
    twin.set_channel_taps_farrow(last_H)                                    # (the loop's last install, which no call has used yet)
    for g, w in zip(_queries(f), _queries(twin)):
        assert_bit_equal(g, w, "banks after the loop")
    for o in ones:
        o.close()
    f.close(), twin.close()


# ---- refusals change nothing --------------------------------------------------------------------------------------------------------
def _everything(f):
    """banks, states, history and the output type"""
    return (f.pnfb().tobytes(), [_state5(s) + (s.rate, s.last_count) for s in f.channel_states], np.array(f.history).tobytes(), str(f.output_dtype))


def test_refusals_change_nothing(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    lib = pkg.load_library()
    Nphi, hLen, P, n, nch, tx = 32, 250, 4, 200, 3, np.float32
    H, x = _signal(9700, Nphi, hLen, 2 * n, np.float32, tx, nch)
    CH, _ = _signal(9701, Nphi, hLen, 8, np.complex64, tx, nch)
    xd, Hd, CHd = _dev(torch, x), _dev(torch, H), _dev(torch, CH)
    Hd64, CHd128 = Hd.double(), CHd.to(torch.complex128)
    _env(monkeypatch, False)
    mk = lambda **kw: _rates_filter(pkg, H, R3, Nphi, P, tx, **kw)
    shared, shared_twin, real, real_twin, cplx, cplx_twin, fused = mk(), mk(), mk(), mk(), mk(), mk(), mk(fused=True)
    for g in (real, real_twin):
        g.set_channel_taps_farrow(np.array(H))
    for g in (cplx, cplx_twin):
        g.set_channel_ctaps_farrow(np.array(CH))
    arb = pkg.FIRFilter.per_channel_rates(np.array(H[0]), R3, Nphi).bind(tx, nch)
    one = pkg.FIRFilter(np.array(H[0]), 2.123, Nphi, P).bind(tx, nch)
    bank = pkg.FIRFilter.per_channel_farrow(np.array(H), 2.123, Nphi, P).bind(tx, nch)
    big_h = np.ones(2 * 1025, dtype=np.float32)
    big = pkg.FIRFilter.per_channel_rates_farrow(big_h, R3, 1025, 2).bind(tx, nch)                   # Nphi above the bound
    deficient = pkg.FIRFilter.per_channel_rates_farrow(np.ones(8, dtype=np.float32), R3, 2, 3, pnfb=np.ones((4, 4))).bind(tx, nch)      # polyorder + 1 > Nphi
    pairs = ((shared, shared_twin), (real, real_twin), (cplx, cplx_twin))
    firsts = [[g.filt(xd[:, :n]) for g in p] for p in pairs]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    TF, CF = lib.mrhip_set_channel_taps_farrow_device, lib.mrhip_set_channel_ctaps_farrow_device
    WT, WC = "mrhip_set_channel_taps_farrow_device", "mrhip_set_channel_ctaps_farrow_device"

    def refused(rc, code, *texts):
        msg = lib.mrhip_last_error().decode()
        assert rc == code, (rc, code, texts, msg)
        for t in texts:
            assert t in msg, (t, msg)

    before = [[_everything(g) for g in pr] for pr in pairs]
    refused(TF(None, p(Hd), hLen, 0, stream), 1, WT + ": NULL filter")
    refused(CF(None, p(CHd), hLen, 2, stream), 1, WC + ": NULL filter")
    refused(TF(arb._handle, p(Hd), hLen, 0, stream), 1, WT + ":", "mrhip_create_arbitrary_rates takes mrhip_set_channel_taps_device")
    refused(CF(arb._handle, p(CHd), hLen, 2, stream), 1, WC + ":", "mrhip_create_arbitrary_rates takes mrhip_set_channel_ctaps_device")
    for g in (one, bank):
        refused(TF(g._handle, p(Hd), hLen, 0, stream), 1, WT + " takes a filter of mrhip_create_farrow_rates")
        refused(CF(g._handle, p(CHd), hLen, 2, stream), 1, WC + " takes a filter of mrhip_create_farrow_rates")
    for g in (shared, real):
        refused(TF(g._handle, None, hLen, 0, stream), 1, WT + ": h is NULL")
        refused(TF(g._handle, p(Hd), hLen - 1, 0, stream), 1, WT + ": hLen must be the filter's")
        refused(TF(g._handle, p(Hd), hLen, 9, stream), 1, WT + ": bad tap dtype")
        refused(TF(g._handle, p(CHd), hLen, 2, stream), 5, WT + ": complex taps with per-channel rates are left out")
        refused(TF(g._handle, p(Hd64), hLen, 1, stream), 1, WT + ": the taps must have the filter's tap dtype")
    for g in (shared, real, cplx):
        refused(CF(g._handle, None, hLen, 2, stream), 1, WC + ": h is NULL")
        refused(CF(g._handle, p(CHd), hLen + 1, 2, stream), 1, WC + ": hLen must be the filter's")
        refused(CF(g._handle, p(CHd), hLen, -1, stream), 1, WC + ": bad tap dtype")
        refused(CF(g._handle, p(Hd), hLen, 0, stream), 1, WC + ":", "real taps go through mrhip_set_channel_taps_farrow_device")
        refused(CF(g._handle, p(CHd128), hLen, 3, stream), 1, WC + ": the taps must be the complex type of the filter's tap precision")
    refused(CF(fused._handle, p(CHd), hLen, 2, stream), 5, WC + ":", "FUSED")                            # FUSED with complex taps
    refused(CF(fused._handle, p(CHd), hLen - 1, 2, stream), 1, WC + ": hLen")                            # (the lengths before the numerics)
    refused(TF(cplx._handle, p(Hd), hLen, 0, stream), 5, WT + ":", "going back to real taps is left out")
    big_d = torch.ones((nch, 2 * 1025), dtype=torch.float32, device="cuda")
    refused(TF(big._handle, p(big_d), 2 * 1025, 0, stream), 5, WT + ":", "Nphi up to 1024", "mrhip_set_channel_taps_farrow fits on the host")
    refused(CF(big._handle, p(big_d.to(torch.complex64)), 2 * 1025, 2, stream), 5, WC + ":", "Nphi up to 1024", "mrhip_set_channel_ctaps_farrow fits on the host")
    small_d = torch.ones((nch, 8), dtype=torch.float32, device="cuda")
    refused(TF(deficient._handle, p(small_d), 8, 0, stream), 1, WT + ": polynomial fit is rank deficient")
    refused(CF(deficient._handle, p(small_d.to(torch.complex64)), 8, 2, stream), 1, WC + ": polynomial fit is rank deficient")
    refused(lib.mrhip_set_channel_taps_farrow(deficient._handle, C.c_void_p(np.ones((nch, 8), dtype=np.float32).ctypes.data), 8, 0), 1,
            "mrhip_set_channel_taps_farrow: polynomial fit is rank deficient")                           # (the host call's answer, as before)
    # a capturing stream: status 5, nothing captured
    gr, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device="cuda")
    with torch.cuda.graph(gr, stream=s):
        scratch.add_(1.0)                                                   # (so that the graph is not empty)
        rcs = []
        for g in (shared, real):
            rcs += [TF(g._handle, p(Hd), hLen, 0, C.c_void_p(s.cuda_stream)), lib.mrhip_last_error().decode()]
        for g in (shared, cplx):
            rcs += [CF(g._handle, p(CHd), hLen, 2, C.c_void_p(s.cuda_stream)), lib.mrhip_last_error().decode()]
    torch.cuda.synchronize()
    assert tuple(rcs[0::2]) == (5, 5, 5, 5) and all("captur" in m for m in rcs[1::2]), rcs
    assert all(WT in m for m in rcs[1:4:2]) and all(WC in m for m in rcs[5::2]), rcs
    # the Python methods: wrong kinds, shapes and dtypes; a refused call changes no mirror
    for g, call, code in ((arb, lambda: arb.set_channel_taps_farrow_device(Hd), 1), (one, lambda: one.set_channel_ctaps_farrow_device(CHd), 1),
                          (shared, lambda: shared.set_channel_taps_farrow_device(Hd[:, :-1].contiguous()), 1), (shared, lambda: shared.set_channel_taps_farrow_device(Hd64), 1),
                          (shared, lambda: shared.set_channel_taps_farrow_device(Hd.t().contiguous().t()), 1), (shared, lambda: shared.set_channel_ctaps_farrow_device(CHd128), 1),
                          (shared, lambda: shared.set_channel_ctaps_farrow_device(Hd), 1), (fused, lambda: fused.set_channel_ctaps_farrow_device(CHd), 5),
                          (cplx, lambda: cplx.set_channel_taps_farrow_device(Hd), 5), (big, lambda: big.set_channel_taps_farrow_device(big_d), 5),
                          (deficient, lambda: deficient.set_channel_taps_farrow_device(small_d), 1)):
        mirror = (g._chan_farrow, g._farrow_ctaps)
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == code, str(e.value)
        assert (g._chan_farrow, g._farrow_ctaps) == mirror
    # what answered before answers as before
    refused(lib.mrhip_set_channel_taps_device(shared._handle, p(Hd), hLen, 0, stream), 5, "mrhip_set_channel_taps_device: the fit of a FIRFarrow filter's rows on the device is left out",
            "mrhip_set_channel_pnfb_device")
    # nothing changed: banks, states, history -- and the next call's outputs equal the twin's, which was never asked
    for pr, bf, first in zip(pairs, before, firsts):
        assert [_everything(g) for g in pr] == bf
        _assert_rows_equal(first[0], first[1], "the first call")
        ya, yb = pr[0].filt(xd[:, n:]), pr[1].filt(xd[:, n:])
        _assert_rows_equal(ya, yb, "the call after the refusals")
        assert pr[0].last_kernel_name() == pr[1].last_kernel_name()
    assert shared.last_kernel_name() == FB.SHARED[False]                     # the shared bank is still the shared bank
    for g in (shared, shared_twin, real, real_twin, cplx, cplx_twin, fused, arb, one, bank, big, deficient):
        g.close()


# ---- installs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_host_and_device_installs_mix_and_reset_keeps_the_banks(pkg, monkeypatch, torch_cuda, cplx):
    """device, host, device, host installs of four different matrices between calls, on a filter whose first call ran on the shared
    bank; the twin takes the host call every time.  Then reset(): the banks stay, the states start over."""
    torch = torch_cuda
    Nphi, hLen, P, n, nch, tx = 32, 250, 4, 120, 3, np.float32
    th = np.complex64 if cplx else np.float32
    _, x = _signal(9800, Nphi, hLen, 6 * n, th, tx, nch)
    Hs = [_signal(9801 + k, Nphi, hLen, 8, th, tx, nch)[0] for k in range(4)]
    xd = _dev(torch, x)
    _env(monkeypatch, False)
    f, twin = _rates_filter(pkg, Hs[0], R3, Nphi, P, tx), _rates_filter(pkg, Hs[0], R3, Nphi, P, tx)
    ya, yb = f.filt(xd[:, :n]), twin.filt(xd[:, :n])                           # the shared bank filters first
    assert f.last_kernel_name() == FB.SHARED[False]
    _assert_rows_equal(ya, yb, "piece 0")
    for k, H in enumerate(Hs):
        _install(f, torch, H, device=k % 2 == 0), _install(twin, torch, H, device=False)
        a, b = (k + 1) * n, (k + 2) * n
        ya, yb = f.filt(xd[:, a:b]), twin.filt(xd[:, a:b])
        assert ya[0].dtype == _tt(torch, np.complex64 if cplx else np.float32)
        _assert_rows_equal(ya, yb, f"piece {k + 1}")
        for g, w in zip(_queries(f), _queries(twin)):
            assert_bit_equal(g, w, f"banks after install {k}")
    assert [_state5(s) for s in f.channel_states] == [_state5(s) for s in twin.channel_states]
    assert_bit_equal(f.history, twin.history, "history")
    _install(f, torch, Hs[0])                                               # a device install is the last one before reset()
    _install(twin, torch, Hs[0], device=False)
    f.reset(), twin.reset()
    assert [(s.phiAccumulator, s.inputDeficit) for s in f.channel_states] == [(1.0, 1)] * nch
    assert_bit_equal(f.pnfb(), twin.pnfb(), "reset() keeps what the device installed")
    ys = f.filt(xd[:, :n])
    for c in range(nch):
        one = _one_channel(pkg, Hs[0][c], R3[c], Nphi, P, tx)
        assert_bit_equal(f.pnfb()[c], one.pnfb(), f"bank of channel {c} after reset()")
        assert_bit_equal(ys[c].cpu().numpy(), one.filt(xd[c, :n]).cpu().numpy(), f"channel {c} after reset(): a one-channel filter from its first sample")
        one.close()
    f.close(), twin.close()


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_a_first_call_on_a_shared_bank_allocates_once(pkg, monkeypatch, torch_cuda, cplx):
    """the device's free memory (hipMemGetInfo through torch) around three installs on a filter whose bank is still shared, with banks
    large enough to show: 4096 channels of 64 rows and 5 coefficients, 10 MiB (complex: 20 MiB).  The first call takes about the banks'
    size (the new banks, less the one shared bank it frees, plus the fit's table); the second and the third take nothing.  The bounds
    are half the banks' size and a quarter of it: wide enough for the allocator's granularity and for whatever else runs on the device,
    narrow enough that a second allocation of the banks, or a leak of them per call, cannot pass."""
    torch = torch_cuda
    Nphi, hLen, P, nch, tx = 32, 2048, 4, 4096, np.float32
    bank_bytes = nch * (hLen // Nphi) * (P + 1) * 8 * (2 if cplx else 1)
    rng = np.random.default_rng(9850)
    h = (rng.standard_normal(hLen) * Nphi / hLen).astype(np.float32)
    _env(monkeypatch, False)
    f = pkg.FIRFilter.per_channel_rates_farrow(h, np.linspace(2.0, 2.25, nch), Nphi, P).bind(tx, nch)
    Hd = torch.randn((nch, hLen), dtype=torch.complex64 if cplx else torch.float32, device="cuda") * (Nphi / hLen)
    install = f.set_channel_ctaps_farrow_device if cplx else f.set_channel_taps_farrow_device
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info()[0]]
    for _ in range(3):
        install(Hd)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    taken = [free[k] - free[k + 1] for k in range(3)]
    print(f"bank bytes {bank_bytes}; taken by the three calls: {taken}")
    assert bank_bytes // 2 <= taken[0] <= 2 * bank_bytes, (bank_bytes, taken)
    assert abs(taken[1]) <= bank_bytes // 4 and abs(taken[2]) <= bank_bytes // 4, (bank_bytes, taken)
    assert f.pnfb().shape == (nch, hLen // Nphi, P + 1)
    f.close()


# ---- each bank receives its own coefficients ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", TAPS, ids=[np.dtype(t).name for t in TAPS])
def test_each_bank_receives_its_own_coefficients_and_nothing_else(pkg, monkeypatch, torch_cuda, th):
    """every bank is poisoned through the host's coefficient call first; after the device fit bank c holds the fit of H[c] in every
    coefficient and no poison is left anywhere; channels whose rows are equal get equal banks, all others differ.  67 channels of 14
    rows and 3 coefficients: 938 (complex: 1876) lanes, a partial last workgroup."""
    torch = torch_cuda
    Nphi, hLen, P, nch, tx = 3, 40, 2, 67, np.float32
    cplx = np.dtype(th).kind == "c"
    T = -(-hLen // Nphi)
    H = np.array(_signal(9900, Nphi, hLen, 8, th, tx, nch)[0])
    H[66] = H[0]
    _env(monkeypatch, False)
    h0 = np.ascontiguousarray(H[0].real)
    f = pkg.FIRFilter.per_channel_rates_farrow(h0, R67, Nphi, P).bind(tx, nch)
    poison = np.full((nch, T, P + 1), 12345.0)
    if cplx:
        f.set_channel_pnfb_ctaps(poison * (1 + 1j))
    else:
        f.set_channel_pnfb(poison)
    assert (f.pnfb().real == 12345.0).all()
    _install(f, torch, H)
    got = f.pnfb()
    assert got.shape == (nch, T, P + 1) and not (got.real == 12345.0).any() and not (got.imag == 12345.0).any()
    assert np.isfinite(got.view(np.float64)).all()
    for c in range(nch):
        one = _one_channel(pkg, H[c], R67[c], Nphi, P, tx)
        assert_bit_equal(got[c], one.pnfb(), f"bank of channel {c}")
        one.close()
    assert got[66].tobytes() == got[0].tobytes() and len({got[c].tobytes() for c in range(nch)}) == nch - 1
    f.close()
