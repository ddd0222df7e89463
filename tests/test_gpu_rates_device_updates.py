"""GPU tests of the device-resident updates of the filters with per-channel rates (include/multirate_hip.h, "Device-resident updates for
the filters with per-channel rates"): mrhip_set_channel_rates_device (rates_set_kernel, csrc/kernels_rates_arb.hip),
mrhip_set_channel_taps_device and mrhip_set_channel_pnfb_device (csrc/kernels_rates_bank_build.hip), through
FIRFilter.set_channel_rates_device / .set_channel_taps_device / .set_channel_pnfb_device and through ctypes.

Bar: everything is BIT FOR BIT, no tolerance anywhere.  The banks a device install builds are those of the host install and of
mrhip_taps2pfb per row; after a device install every channel is the oracle's one-channel filter (outputs, counts, end state, history);
a loop of filter call, new rates and taps computed by torch ON the device, device install, filter call -- in which nothing is read back
and nothing waits between the first and the last piece -- equals piece by piece the twin driven through the host calls with the same
values and, for Float32, the oracle's filters rebuilt per piece; a rate the kernel refuses (NaN, 0, negative, below 2^-30, outside the
declared range) leaves its channel at the old rate in every bit and is reported; host refusals change nothing; a call after
set_channel_rates_device writes row c in [0, count_c) and nothing else.  Signals, references and _check_end are those of
tests/test_gpu_rates_arb.py / test_gpu_rates_bank_arb.py; the shapes are the smallest at which this can go wrong.
"""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_rates_bank_farrow as FB
from conftest import assert_bit_equal
from output_bounds_cases import LAYOUTS, make_buffer, row_pad
from test_gpu_rates_arb import CASES, R3, R4, R67, _assert_rows_only_written, _check_end, _chunks, _state5, _tt
from test_gpu_rates_arb import _signal as _shared_signal
from test_gpu_rates_bank_arb import GENERIC, SHARED, TILED, _env, _reference, _signal

pytestmark = pytest.mark.gpu

PHASES = (1.0, 2.5, 3.999)        # (every bank has at least 3 phases)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def _numerics(pkg, fused):
    return pkg.NUMERICS_FUSED if fused else pkg.NUMERICS_STRICT


def _queries(f):
    return (f.taps(0), f.taps(1)) + tuple(f.tapsforphase(p) for p in PHASES)


# ---- banks as built ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank,types", CASES, ids=[f"{b[0]}x{b[1]}-{np.dtype(t[0]).name}-{np.dtype(t[1]).name}" for b, t in CASES])
def test_the_banks_are_those_of_the_host_install_and_of_taps2pfb(pkg, monkeypatch, torch_cuda, bank, types):
    torch = torch_cuda
    (Nphi, hLen), (th, tx) = bank, types
    H, _ = _signal(4000 + Nphi + hLen, Nphi, hLen, 8, th, tx, 3)
    _env(monkeypatch, False)
    f = pkg.FIRFilter.per_channel_rates(np.array(H[1]), R3, Nphi).bind(tx, 3)
    twin = pkg.FIRFilter.per_channel_rates(np.array(H[1]), R3, Nphi).bind(tx, 3)
    f.set_channel_taps_device(_dev(torch, H))
    twin.set_channel_taps(H)
    got, want = _queries(f), _queries(twin)
    T = -(-hLen // Nphi)
    assert got[0].shape == (3, T, Nphi) and got[2].shape == (3, T)
    for g, w, name in zip(got, want, ("pfb", "dpfb") + tuple(f"tapsforphase({p})" for p in PHASES)):
        assert g.dtype == w.dtype == np.dtype(th)
        assert_bit_equal(g, w, f"{name}: device install against host install")
    for c in range(3):
        dh = np.append(np.diff(H[c]), np.zeros(1, dtype=th)).astype(th)      # [diff(h), 0]: one subtraction in the tap type
        assert dh.dtype == np.dtype(th)
        assert_bit_equal(got[0][c], pkg.host.taps2pfb(np.array(H[c]), Nphi), f"pfb of channel {c} against mrhip_taps2pfb")
        assert_bit_equal(got[1][c], pkg.host.taps2pfb(dh, Nphi), f"dpfb of channel {c} against mrhip_taps2pfb of [diff(h), 0]")
    f.close(), twin.close()


# ---- every channel is its one-channel filter --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("fused", [False, True], ids=["strict", "fused"])
@pytest.mark.parametrize("rates", [R4, R67], ids=["R4", "nch67"])
def test_every_channel_is_its_one_channel_filter(pkg, O, monkeypatch, torch_cuda, rates, fused, tiled):
    """a filter created with OTHER taps (row 0 for every channel) and OTHER rates (1.0), then given H and the rates from device memory
    before its first call: channel c is the oracle's FIRFilter(H[c], rates[c], Nphi) from the first sample on.  R67: more than one
    workgroup of rates_set_kernel and of the bank build kernel, and idle lanes."""
    torch = torch_cuda
    Nphi, hLen, th, tx = 32, 250, np.float32, np.float32
    nch = len(rates)
    for x_len in (257, 1500):
        seed = 1000 * Nphi + hLen + x_len
        H, x = _signal(seed, Nphi, hLen, x_len, th, tx, nch)
        xd = _dev(torch, x)
        for name, how in (("whole", None), ("prime", 97)):
            outs, states, hists = _reference(O, seed, rates, Nphi, hLen, x_len, th, tx, how, fused)
            _env(monkeypatch, tiled)
            f = pkg.FIRFilter.per_channel_rates(np.array(H[0]), [1.0] * nch, Nphi, numerics=_numerics(pkg, fused)).bind(tx, nch)
            f.set_channel_taps_device(_dev(torch, H))
            f.set_channel_rates_device(_dev(torch, np.array(rates, dtype=np.float64)), min(rates), max(rates))
            assert f.rate == max(rates)
            for i, (a, b) in enumerate(_chunks(x_len, how)):
                what = f"nch {nch} x_len {x_len} {name} piece {i} [{a}, {b})"
                y = torch.zeros((nch, f.outputlength_bound(b - a)), dtype=torch.float32, device="cuda")
                counts = f.filt_into(y, xd[:, a:b])
                want = [len(outs[c][i]) for c in range(nch)]
                assert list(counts) == want, (what, list(counts), want)
                yh = y.cpu().numpy()
                for c in range(nch):
                    assert_bit_equal(yh[c, :want[c]], outs[c][i], f"{what}: channel {c}")
                assert f.last_kernel_name() == (TILED if tiled else GENERIC), what
            _check_end(f, states, hists, f"{name} x_len {x_len}")
            assert [(s.rate, s.delta) for s in f.channel_states] == [(float(r), np.float64(Nphi) / np.float64(r)) for r in rates]
            f.close()


# ---- a loop that never meets the host ---------------------------------------------------------------------------------------------
LOOP_X_LEN, LOOP_PIECE, LOOP_LO, LOOP_HI = 1500, 97, 0.009, 12.0


def _loop_values(torch, base_rates_d, base_d, i):
    """the tracker's stand-in: piece i's rates and taps (or coefficients), computed by torch ON the device from the bases, in their
    dtypes.  Kept so that the host can learn them AFTER the loop."""
    rates = base_rates_d * (1.0 + 0.002 * i) + 1e-4 * torch.arange(base_rates_d.numel(), dtype=torch.float64, device="cuda") * (i % 3)
    values = base_d * (1.0 + 0.01 * i) + 0.003 * torch.roll(base_d, shifts=i + 1, dims=-1)
    return rates.contiguous(), values.contiguous()


def _rebuilt_per_piece_reference(make, x, pieces, states_of):
    """channel c: a NEW oracle filter for every piece, made by make(c, i) and given the previous one's (inputDeficit, phiAccumulator) and
    history -- as tests/test_gpu_rates_bank_arb.py rebuilds its filters where the taps change"""
    outs, states, hists = [], [], []
    for c in range(x.shape[0]):
        r, row = None, []
        for i, (a, b) in enumerate(pieces):
            new = make(c, i)
            if r is not None:
                st = r.state
                new.set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
                new.set_history(r.history)
            r = new
            row.append(r.filt(x[c, a:b]))
        outs.append(row), states.append(states_of(r.state)), hists.append(r.history)
    return outs, states, hists


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
@pytest.mark.parametrize("types", [(np.float32, np.float32), (np.float64, np.complex64)], ids=["f32-f32", "f64-c64"])
def test_a_loop_that_never_meets_the_host(pkg, O, monkeypatch, torch_cuda, types, tiled):
    torch = torch_cuda
    th, tx = types
    Nphi, hLen, nch = 32, 250, 4
    H0, x = _signal(5150, Nphi, hLen, LOOP_X_LEN, th, tx, nch)
    pieces = _chunks(LOOP_X_LEN, LOOP_PIECE)
    xd, base_H, base_r = _dev(torch, x), _dev(torch, H0), _dev(torch, np.array(R4, dtype=np.float64))
    _env(monkeypatch, tiled)
    f = pkg.FIRFilter.per_channel_rates(np.array(H0[0]), R4, Nphi).bind(tx, nch)
    out_dtype = _tt(torch, f.output_dtype)
    # piece 0's install is the first one: it allocates the banks and may wait once; from then on nothing reads back and nothing waits
    kept, ys, cnts = [], [], []
    for i, (a, b) in enumerate(pieces):
        rates_d, H_d = _loop_values(torch, base_r, base_H, i)
        assert H_d.dtype == _tt(torch, th) and rates_d.dtype == torch.float64
        f.set_channel_rates_device(rates_d, LOOP_LO, LOOP_HI)
        f.set_channel_taps_device(H_d)
        y = torch.zeros((nch, f.outputlength_bound(b - a)), dtype=out_dtype, device="cuda")
        cnt = torch.zeros(nch, dtype=torch.int64, device="cuda")
        f._filt_into_rates(y, xd[:, a:b], counts=cnt)                       # (returns without waiting; the counts stay on the device)
        kept.append((rates_d, H_d)), ys.append(y), cnts.append(cnt)
    assert f.last_kernel_name() == (TILED if tiled else GENERIC)
    # only now does the host learn anything
    values = [(r.cpu().numpy(), h.cpu().numpy()) for r, h in kept]
    got = [(y.cpu().numpy(), c.cpu().numpy()) for y, c in zip(ys, cnts)]
    assert all(LOOP_LO <= r.min() and r.max() <= LOOP_HI for r, _ in values) and len({h.tobytes() for _, h in values}) == len(pieces)
    # (a) the twin driven through the host calls with the same values
    twin = pkg.FIRFilter.per_channel_rates(np.array(H0[0]), R4, Nphi).bind(tx, nch)
    for i, (a, b) in enumerate(pieces):
        twin.set_channel_rates(values[i][0])
        twin.set_channel_taps(values[i][1])
        yt = torch.zeros((nch, twin.outputlength_bound(b - a)), dtype=out_dtype, device="cuda")
        counts = twin.filt_into(yt, xd[:, a:b])
        assert list(got[i][1]) == list(counts), (i, list(got[i][1]), list(counts))
        yth = yt.cpu().numpy()
        for c in range(nch):
            assert_bit_equal(got[i][0][c, :counts[c]], yth[c, :counts[c]], f"piece {i}, channel {c}: device calls against host calls")
    fs, ts = f.channel_states, twin.channel_states
    assert [_state5(s) + (s.rate, s.delta, s.last_count) for s in fs] == [_state5(s) + (s.rate, s.delta, s.last_count) for s in ts]
    assert [(s.rate, s.delta) for s in fs] == [(float(r), np.float64(Nphi) / np.float64(r)) for r in values[-1][0]]       # delta in every bit
    assert_bit_equal(f.history, twin.history, "history after the loop")
    for g, w in zip(_queries(f), _queries(twin)):
        assert_bit_equal(g, w, "taps after the loop")
    # (b) the oracle's one-channel filters, rebuilt per piece
    if (th, tx) == (np.float32, np.float32):
        make = lambda c, i: O.FIRFilter(values[i][1][c], float(values[i][0][c]), Nphi, tx=tx)
        outs, states, hists = _rebuilt_per_piece_reference(make, x, pieces, _state5)
        for i in range(len(pieces)):
            for c in range(nch):
                assert got[i][1][c] == len(outs[c][i]), (i, c)
                assert_bit_equal(got[i][0][c, :got[i][1][c]], outs[c][i], f"piece {i}, channel {c}: against the oracle")
        _check_end(f, states, hists, "after the loop, against the oracle")
    f.close(), twin.close()


@pytest.mark.parametrize("multi", [False, True], ids=["generic", "multi"])
def test_the_farrow_loop_that_never_meets_the_host(pkg, monkeypatch, torch_cuda, multi):
    """FIRFarrow, polyorder 4, Float32 taps: the coefficients are Float64 values that are NOT Float32-representable, so the rounding on
    the device is what is checked; against the twin driven through set_channel_rates / set_channel_pnfb with the same values"""
    torch = torch_cuda
    Nphi, hLen, P, nch, tx = 32, 250, 4, 4, np.float32
    H0, x = FB._signal(5160, Nphi, hLen, LOOP_X_LEN, np.float32, tx, nch)
    T = -(-hLen // Nphi)
    base = np.random.default_rng(5161).standard_normal((nch, T, P + 1)) / T * np.array([1.0, 0.1, 0.01, 0.001, 0.0001])
    pieces = _chunks(LOOP_X_LEN, LOOP_PIECE)
    xd, base_PN, base_r = _dev(torch, x), _dev(torch, base), _dev(torch, np.array(R4, dtype=np.float64))
    FB._env(monkeypatch, multi)
    f = pkg.FIRFilter.per_channel_rates_farrow(np.array(H0[0]), R4, Nphi, P).bind(tx, nch)
    kept, ys, cnts = [], [], []
    for i, (a, b) in enumerate(pieces):
        rates_d, PN_d = _loop_values(torch, base_r, base_PN, i)
        f.set_channel_rates_device(rates_d, LOOP_LO, LOOP_HI)
        f.set_channel_pnfb_device(PN_d)
        y = torch.zeros((nch, f.outputlength_bound(b - a)), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(nch, dtype=torch.int64, device="cuda")
        f._filt_into_rates(y, xd[:, a:b], counts=cnt)
        kept.append((rates_d, PN_d)), ys.append(y), cnts.append(cnt)
    assert f.last_kernel_name() == (FB.MULTI if multi else FB.GENERIC)
    values = [(r.cpu().numpy(), p.cpu().numpy()) for r, p in kept]
    got = [(y.cpu().numpy(), c.cpu().numpy()) for y, c in zip(ys, cnts)]
    for _, pn in values:
        assert pn.dtype == np.float64 and (pn.astype(np.float32).astype(np.float64) != pn).mean() > 0.9        # the rounding has work to do
    twin = pkg.FIRFilter.per_channel_rates_farrow(np.array(H0[0]), R4, Nphi, P).bind(tx, nch)
    for i, (a, b) in enumerate(pieces):
        twin.set_channel_rates(values[i][0])
        twin.set_channel_pnfb(values[i][1])
        yt = torch.zeros((nch, twin.outputlength_bound(b - a)), dtype=torch.float32, device="cuda")
        counts = twin.filt_into(yt, xd[:, a:b])
        assert list(got[i][1]) == list(counts), (i, list(got[i][1]), list(counts))
        yth = yt.cpu().numpy()
        for c in range(nch):
            assert_bit_equal(got[i][0][c, :counts[c]], yth[c, :counts[c]], f"piece {i}, channel {c}: device calls against host calls")
    fs, ts = f.channel_states, twin.channel_states
    assert [_state5(s) + (s.rate, s.delta, s.last_count) for s in fs] == [_state5(s) + (s.rate, s.delta, s.last_count) for s in ts]
    assert [(s.rate, s.delta) for s in fs] == [(float(r), np.float64(Nphi) / np.float64(r)) for r in values[-1][0]]
    assert_bit_equal(f.history, twin.history, "history after the loop")
    assert f.pnfb().shape == (nch, T, P + 1)
    assert_bit_equal(f.pnfb(), twin.pnfb(), "pnfb after the loop")
    assert_bit_equal(f.pnfb(), values[-1][1].astype(np.float32).astype(np.float64), "pnfb: rounded to Float32 and widened back")
    assert_bit_equal(f.tapsforphase(17.375), twin.tapsforphase(17.375), "tapsforphase after the loop")
    f.close(), twin.close()


# ---- refused values ---------------------------------------------------------------------------------------------------------------
R8 = [0.47, 1.0, 2.123, 0.8, 1.5, 0.3, 2.5, 1.25]


@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_refused_values_leave_their_channels_at_the_old_rate(pkg, O, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    lib = pkg.load_library()
    Nphi, hLen, n, lo, hi = 32, 250, 300, 0.25, 3.0
    h, x = _shared_signal(5170, Nphi, hLen, 3 * n, np.float32, np.float32, R8)
    new = [float("nan"), 0.0, -1.0, 2.0 ** -31, 4.5, 0.125, 2.75, 0.6]       # six refusals of eight; the last two are taken
    after = R8[:6] + new[6:]
    xd = _dev(torch, x)
    _env(monkeypatch, tiled)
    f = pkg.FIRFilter.per_channel_rates(h, R8, Nphi).bind(np.float32, 8)
    O.set_fused(False)
    refs = [O.FIRFilter(h, float(r), Nphi, tx=np.float32) for r in R8]

    def piece_equals_the_oracle(i):
        ys = f.filt(xd[:, i * n:(i + 1) * n])
        for c, r in enumerate(refs):
            assert_bit_equal(ys[c].cpu().numpy(), r.filt(x[c, i * n:(i + 1) * n]), f"piece {i}, channel {c}")

    piece_equals_the_oracle(0)
    f.set_channel_rates_device(_dev(torch, np.array(new)), lo, hi)           # nothing here faults: the kernel only declines to write
    for c in (6, 7):                                                         # the two that took the new rate: rebuilt, state and history carried over
        st, hist = refs[c].state, refs[c].history
        refs[c] = O.FIRFilter(h, after[c], Nphi, tx=np.float32)
        refs[c].set_state(int(math.floor(st.phiAccumulator)), int(st.inputDeficit), float(st.phiAccumulator))
        refs[c].set_history(hist)
    piece_equals_the_oracle(1)                                               # (the status is sticky, the outputs are exact all the same)
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.channel_states
    assert e.value.code == 1 and "rate was refused" in str(e.value) and "kept its rate" in str(e.value)
    raw = (pkg.ChannelState * 8)()
    assert lib.mrhip_get_channel_states(f._handle, C.cast(raw, C.c_void_p)) == 1              # (the states are filled in all the same)
    assert [s.rate for s in raw] == after and [s.delta for s in raw] == [np.float64(Nphi) / np.float64(r) for r in after]
    assert [_state5(s) for s in raw] == [_state5(r.state) for r in refs]
    f.set_channel_states([s.inputDeficit for s in raw], [s.phiAccumulator for s in raw])     # clears the refusal, moves nothing
    assert [_state5(s) + (s.rate,) for s in f.channel_states] == [_state5(r.state) + (a,) for r, a in zip(refs, after)]
    piece_equals_the_oracle(2)
    _check_end(f, [_state5(r.state) for r in refs], [r.history for r in refs], "after the refused rates")
    f.set_channel_rates_device(_dev(torch, np.array(new)), lo, hi)
    f.reset()                                                                # reset clears it too, and keeps the rates
    assert [(s.rate, s.phiAccumulator, s.inputDeficit) for s in f.channel_states] == [(a, 1.0, 1) for a in after]
    f.close()


# ---- host refusals change nothing -------------------------------------------------------------------------------------------------
def test_host_refusals_change_nothing(pkg, monkeypatch, torch_cuda):
    torch = torch_cuda
    lib = pkg.load_library()
    Nphi, hLen, P, n = 32, 250, 4, 300
    H, x = _signal(5180, Nphi, hLen, 2 * n, np.float32, np.float32, 3)
    xd, Hd, rd = _dev(torch, x), _dev(torch, H), _dev(torch, np.array(R3))
    T = -(-hLen // Nphi)
    PNd = torch.ones((3, T, P + 1), dtype=torch.float64, device="cuda")
    _env(monkeypatch, False), FB._env(monkeypatch, False)
    mk_arb = lambda: pkg.FIRFilter.per_channel_rates(np.array(H[0]), R3, Nphi).bind(np.float32, 3)
    mk_far = lambda: pkg.FIRFilter.per_channel_rates_farrow(np.array(H[0]), R3, Nphi, P).bind(np.float32, 3)
    arb, arb_twin, far, far_twin = mk_arb(), mk_arb(), mk_far(), mk_far()
    one = pkg.FIRFilter(np.array(H[0]), 2.123, Nphi).bind(np.float32, 3)
    firsts = [g.filt(xd[:, :n]) for g in (arb, arb_twin, far, far_twin)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def refused(rc, code, text):
        assert rc == code, (rc, code, text)
        msg = lib.mrhip_last_error().decode()
        assert text in msg, msg

    R, TP, PN = lib.mrhip_set_channel_rates_device, lib.mrhip_set_channel_taps_device, lib.mrhip_set_channel_pnfb_device
    for g in (arb, far):
        refused(R(None, p(rd), 0.4, 2.2, stream), 1, "mrhip_set_channel_rates_device: NULL filter")
        refused(R(g._handle, None, 0.4, 2.2, stream), 1, "rates is NULL")
        for lo, hi, code, text in ((0.0, 2.2, 1, "finite and greater than 0"), (-1.0, 2.2, 1, "finite"), (float("nan"), 2.2, 1, "finite"),
                                   (0.4, float("inf"), 1, "finite"), (2.2, 0.4, 1, "rate_hi < rate_lo"), (2.0 ** -31, 2.2, 5, "2^-30")):
            refused(R(g._handle, p(rd), lo, hi, stream), code, text)
    refused(R(one._handle, p(rd), 0.4, 2.2, stream), 1, "takes a filter of mrhip_create_arbitrary_rates")
    refused(TP(None, p(Hd), hLen, 0, stream), 1, "mrhip_set_channel_taps_device: NULL filter")
    refused(TP(arb._handle, None, hLen, 0, stream), 1, "h is NULL")
    refused(TP(arb._handle, p(Hd), hLen - 1, 0, stream), 1, "hLen")
    refused(TP(arb._handle, p(Hd), hLen, 1, stream), 1, "tap dtype")
    refused(TP(arb._handle, p(Hd), hLen, 2, stream), 5, "complex taps with per-channel rates are left out")
    refused(TP(arb._handle, p(Hd), hLen, 7, stream), 1, "tap dtype")
    refused(TP(far._handle, p(Hd), hLen, 0, stream), 5, "mrhip_set_channel_pnfb_device")
    refused(TP(one._handle, p(Hd), hLen, 0, stream), 1, "takes a filter of mrhip_create_arbitrary_rates")
    refused(PN(None, p(PNd), T, P, stream), 1, "mrhip_set_channel_pnfb_device: NULL filter")
    refused(PN(far._handle, None, T, P, stream), 1, "pnfb is NULL")
    refused(PN(far._handle, p(PNd), T + 1, P, stream), 1, "tapsPerPhi and polyorder")
    refused(PN(far._handle, p(PNd), T, P - 1, stream), 1, "tapsPerPhi and polyorder")
    refused(PN(arb._handle, p(PNd), T, P, stream), 1, "mrhip_set_channel_taps_device")
    refused(PN(one._handle, p(PNd), T, P, stream), 1, "takes a filter of mrhip_create_farrow_rates")
    # a capturing stream: status 5, nothing captured
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        scratch.add_(1.0)                                                   # (so that the graph is not empty)
        cs = C.c_void_p(s.cuda_stream)
        rcs = (R(arb._handle, p(rd), 0.4, 2.2, cs), lib.mrhip_last_error().decode(), TP(arb._handle, p(Hd), hLen, 0, cs), lib.mrhip_last_error().decode(),
               R(far._handle, p(rd), 0.4, 2.2, cs), lib.mrhip_last_error().decode(), PN(far._handle, p(PNd), T, P, cs), lib.mrhip_last_error().decode())
    torch.cuda.synchronize()
    assert rcs[0::2] == (5, 5, 5, 5) and all("captur" in m for m in rcs[1::2]), rcs
    assert [w in m for w, m in zip(("rates_device", "taps_device", "rates_device", "pnfb_device"), rcs[1::2])] == [True] * 4
    # the Python methods: wrong shape / dtype / device class / kind, code 1, no mirror moved
    bad = [lambda: arb.set_channel_rates_device(rd[:2], 0.4, 2.2), lambda: arb.set_channel_rates_device(rd.float(), 0.4, 2.2),
           lambda: arb.set_channel_rates_device(rd.cpu(), 0.4, 2.2), lambda: arb.set_channel_rates_device(rd.repeat(2)[::2], 0.4, 2.2),
           lambda: arb.set_channel_rates_device(np.array(R3), 0.4, 2.2), lambda: arb.set_channel_rates_device(rd, 2.2, 0.4),
           lambda: arb.set_channel_taps_device(Hd[:2]), lambda: arb.set_channel_taps_device(Hd[:, :-1]), lambda: arb.set_channel_taps_device(Hd.double()),
           lambda: arb.set_channel_taps_device(Hd.t().contiguous().t()), lambda: arb.set_channel_taps_device(np.array(H)), lambda: arb.set_channel_pnfb_device(PNd),
           lambda: far.set_channel_taps_device(Hd), lambda: far.set_channel_pnfb_device(PNd[:, :, :-1]), lambda: far.set_channel_pnfb_device(PNd.float()),
           lambda: far.set_channel_pnfb_device(PNd.cpu()), lambda: one.set_channel_rates_device(rd, 0.4, 2.2), lambda: one.set_channel_taps_device(Hd),
           lambda: one.set_channel_pnfb_device(PNd)]
    for i, call in enumerate(bad):
        with pytest.raises(pkg.MultirateHIPError) as e:
            call()
        assert e.value.code == 1, i
    assert arb._chan_taps is None and far._chan_farrow is None and arb.rate == max(R3) and np.array_equal(arb._rates, R3) and np.array_equal(far._rates, R3)
    # nothing moved: kernels, taps, states and the next call's outputs are the untouched twins'
    for g, twin, first, first_twin in ((arb, arb_twin, firsts[0], firsts[1]), (far, far_twin, firsts[2], firsts[3])):
        assert [_state5(s_) + (s_.rate, s_.delta, s_.last_count) for s_ in g.channel_states] == [_state5(s_) + (s_.rate, s_.delta, s_.last_count) for s_ in twin.channel_states]
        ya, yb = g.filt(xd[:, n:]), twin.filt(xd[:, n:])
        assert g.last_kernel_name() == twin.last_kernel_name() == (SHARED[False] if g is arb else FB.SHARED[False])
        for c in range(3):
            assert_bit_equal(first[c].cpu().numpy(), first_twin[c].cpu().numpy(), f"first call, channel {c}")
            assert_bit_equal(ya[c].cpu().numpy(), yb[c].cpu().numpy(), f"the call after the refusals, channel {c}")
        assert_bit_equal(g.history, twin.history, "history after the refusals")
        assert_bit_equal(g.tapsforphase(3.25), twin.tapsforphase(3.25), "taps after the refusals")
    assert arb.taps(0).shape == (T, Nphi) and far.pnfb().shape == (T, P + 1)                # still the shared layouts
    for g in (arb, arb_twin, far, far_twin, one):
        g.close()


# ---- only its own outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "A", "C"])
@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_each_row_receives_its_own_outputs_and_nothing_else(pkg, O, monkeypatch, torch_cuda, tiled, layout):
    """rates from device memory with a declared upper end well above every actual rate: the buffers are sized by hi, row c holds the
    oracle's outputs in [0, count_c) and every other byte of the poisoned backing store (tight; odd strides) is untouched"""
    torch = torch_cuda
    rates, Nphi, hLen, tx = R4, 32, 250, np.float32
    sizes = [257, 5, 300]
    x_len = sum(sizes)
    H, x = _signal(5190, Nphi, hLen, x_len, np.float32, tx, 4)
    O.set_fused(False)
    refs = [O.FIRFilter(H[c], float(r), Nphi, tx=tx) for c, r in enumerate(rates)]
    _env(monkeypatch, tiled)
    f = pkg.FIRFilter.per_channel_rates(np.array(H[0]), [1.0] * 4, Nphi).bind(tx, 4)
    f.set_channel_taps_device(_dev(torch, H))
    f.set_channel_rates_device(_dev(torch, np.array(rates)), 0.005, 40.0)
    oy, _, ox = LAYOUTS[layout]
    xback = torch.zeros((4, ox + x_len + 3), dtype=torch.float32, device="cuda")
    xback[:, ox:ox + x_len] = _dev(torch, x)
    pos = 0
    for i, size in enumerate(sizes):
        want = [r.filt(x[c, pos:pos + size]) for c, r in enumerate(refs)]
        cap = f.outputlength_bound(size)
        assert cap == math.ceil(size * 40.0) + 2 > 3 * max(len(w) for w in want)
        pad = row_pad(layout, oy, cap, 4)
        view, backing = make_buffer(torch, np.float32, 4, cap, oy, pad)
        counts = f.filt_into(view, xback[:, ox + pos:ox + pos + size])
        assert list(counts) == [len(w) for w in want]
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        _assert_rows_only_written(backing, 4, cap, oy, pad, counts, want, f"{layout} piece {i}")
        pos += size
    assert [_state5(s) for s in f.channel_states] == [_state5(r.state) for r in refs]
    f.close()


# ---- mixing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [False, True], ids=["generic", "tiled"])
def test_device_and_host_installs_mix_and_reset_keeps_what_the_device_installed(pkg, O, monkeypatch, torch_cuda, tiled):
    torch = torch_cuda
    Nphi, hLen, x_len, tx, nch = 32, 250, 1500, np.float32, 4
    seed = 1000 * Nphi + hLen + x_len
    H, x = _signal(seed, Nphi, hLen, x_len, np.float32, tx, nch)
    Hs = [H, _signal(5201, Nphi, hLen, 8, np.float32, tx, nch)[0], _signal(5202, Nphi, hLen, 8, np.float32, tx, nch)[0]]
    rs = [[1.37, 0.5, 2.123, 3.01], [0.9, 0.91, 0.92, 0.93], R4]
    how = ["device", "host", "device"]
    pieces = _chunks(900, 300)
    xd = _dev(torch, x)
    _env(monkeypatch, tiled)
    f = pkg.FIRFilter.per_channel_rates(np.array(H[0]), R3 + [1.0], Nphi).bind(tx, nch)
    untouched = pkg.FIRFilter.per_channel_rates(np.array(H[0]), R3 + [1.0], Nphi).bind(tx, nch)
    O.set_fused(False)
    make = lambda c, i: O.FIRFilter(Hs[i][c], float(rs[i][c]), Nphi, tx=tx)
    outs, states, hists = _rebuilt_per_piece_reference(make, x, pieces, _state5)
    for i, (a, b) in enumerate(pieces):
        if how[i] == "device":
            f.set_channel_taps_device(_dev(torch, Hs[i]))
            f.set_channel_rates_device(_dev(torch, np.array(rs[i])), min(rs[i]), max(rs[i]))
            assert f.rate == max(rs[i])
        else:
            f.set_channel_taps(Hs[i])
            f.set_channel_rates(rs[i])
            assert np.array_equal(f._chan_taps, Hs[i]) and np.array_equal(f._rates, rs[i])      # the mirrors are current again
        ys = f.filt(xd[:, a:b])
        for c in range(nch):
            assert_bit_equal(ys[c].cpu().numpy(), outs[c][i], f"piece {i} ({how[i]} install), channel {c}")
        assert f.last_kernel_name() == (TILED if tiled else GENERIC)
        for c in range(nch):
            assert_bit_equal(f.taps(0)[c], pkg.host.taps2pfb(np.array(Hs[i][c]), Nphi), f"pfb after the {how[i]} install {i}, channel {c}")
    _check_end(f, states, hists, "after the three installs")
    # reset(): the constructor state and a history of zeros; the taps and the rates the DEVICE installed stay
    f.reset()
    assert [_state5(s) + (s.last_count, s.rate) for s in f.channel_states] == [(1, 1.0, 1, 0.0, 1, 0, r) for r in R4]
    assert not f.history.any()
    outs, states, hists = _reference(O, seed, R4, Nphi, hLen, x_len, np.float32, tx, None, False)        # (Hs[2] is another matrix: install H)
    f.set_channel_taps_device(_dev(torch, H))
    f.reset()
    ys = f.filt(xd)
    for c in range(nch):
        assert_bit_equal(ys[c].cpu().numpy(), outs[c][0], f"after reset: channel {c}")
    _check_end(f, states, hists, "after reset")
    # a closed filter whose values lived on the device does not bind again; one on which no new call was made is what it always was
    f.close()
    with pytest.raises(pkg.MultirateHIPError) as e:
        f.bind(tx, nch)
    assert e.value.code == 1 and "set_channel_rates_device" in str(e.value)
    untouched.filt(xd[:, :300])
    assert untouched.last_kernel_name() == SHARED[tiled] and untouched.taps(0).shape == (8, Nphi) and untouched.tapsforphase(2.5).shape == (8,)
    assert_bit_equal(untouched.taps(0), pkg.host.taps2pfb(np.array(H[0]), Nphi), "the shared pfb")
    untouched.close()
