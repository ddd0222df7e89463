"""Pins tests/complex_taps_farrow_restatement.py (the model the GPU tests of kernels_ctaps_farrow.hip compare with) to the
untouched C oracle wherever the two overlap -- the oracle refuses complex taps, so the overlap is by components:

* real samples: the Horner evaluation, the rounding to the tap type, the products, the sums and the start-from-zero seam are all
  per component, so re(y) / im(y) are, BIT FOR BIT, the oracle's FIRFarrow outputs with the polynomial banks real(pnfb) /
  imag(pnfb) (counts, 𝜙Accumulator, inputDeficit and history too);
* complex samples: the taps of every output are, bit for bit, the oracle's currentTaps for real(pnfb) and imag(pnfb) at that
  output's phase; the dot behind them is the rational family's, pinned by tests/test_complex_taps_cpu.py.

No GPU: everything here is the restatement, the oracle and the library's host-only parts.
"""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_farrow_restatement import ComplexTapsFarrowRestated, fit_pnfb
from conftest import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [0.47, 1.0, 2.123, 32.0 / 3]
BANKS = [(4, 4, 2), (4, 30, 0), (4, 30, 3), (32, 250, 4)]      # (Nphi, hLen, polyorder): T = 1 (no history), 8, 8, 8
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
X_LEN = 300


def _chunks(n, how):
    if how is None:
        return [(0, n)]
    if isinstance(how, int):
        return [(a, min(a + how, n)) for a in range(0, n, how)]
    out, pos = [], 0
    for c in how:
        out.append((pos, pos + c))
        pos += c
    out.append((pos, n))
    return out


def _bank(pkg, seed, Nphi, hLen, polyorder, th):
    """complex taps and their per-component fit (mrhip_polyfit: host only)"""
    rng = np.random.default_rng(seed)
    h = ((rng.standard_normal(hLen) + 1j * rng.standard_normal(hLen)) / hLen).astype(th)
    return h, fit_pnfb(h, Nphi, polyorder, pkg.polyfit)


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.float64)])
@pytest.mark.parametrize("Nphi,hLen,polyorder", BANKS)
@pytest.mark.parametrize("rate", RATES)
def test_real_samples_are_two_real_tap_oracle_runs(O, pkg, rate, Nphi, hLen, polyorder, th, tx, chunking):
    h, pnfb = _bank(pkg, hLen + polyorder, Nphi, hLen, polyorder, th)
    x = (np.random.default_rng(1).random(X_LEN) - 0.5).astype(tx)
    f = ComplexTapsFarrowRestated(hLen, th, rate, Nphi, polyorder, pnfb, tx=tx)
    rt = np.float32 if th == np.complex64 else np.float64
    hr = np.zeros(hLen, dtype=rt)                         # (the oracle takes only length and type from h when pnfb is given)
    ore = O.FIRFilter(hr, rate, Nphi, tx=tx, polyorder=polyorder, pnfb=np.ascontiguousarray(f.pnfb.real))
    oim = O.FIRFilter(hr, rate, Nphi, tx=tx, polyorder=polyorder, pnfb=np.ascontiguousarray(f.pnfb.imag))
    assert (f.T, f.historyLen) == (ore.state.tapsPerPhi, ore.state.historyLen)
    for a, b in _chunks(X_LEN, CHUNKINGS[chunking]):
        y = f.filt(x[a:b])
        yr, yi = ore.filt(x[a:b]), oim.filt(x[a:b])
        assert y.dtype == (np.complex64 if tx == np.float32 else np.complex128)
        assert len(y) == len(yr) == len(yi), (a, b)
        assert_bit_equal(np.ascontiguousarray(y.real), yr, f"re(y), chunk [{a}, {b})")
        assert_bit_equal(np.ascontiguousarray(y.imag), yi, f"im(y), chunk [{a}, {b})")
        so = ore.state
        assert (f.inputDeficit, f.phiAccumulator) == (so.inputDeficit, so.phiAccumulator), (a, b)
    assert_bit_equal(f.history_array(), ore.history, "history")


@pytest.mark.parametrize("th,tx", [(np.complex64, np.complex64), (np.complex64, np.complex128), (np.complex128, np.complex64)])
@pytest.mark.parametrize("Nphi,hLen,polyorder", BANKS)
@pytest.mark.parametrize("rate", RATES)
def test_complex_samples_taps_of_every_output_are_the_oracles_by_components(O, pkg, rate, Nphi, hLen, polyorder, th, tx):
    h, pnfb = _bank(pkg, 100 + hLen + polyorder, Nphi, hLen, polyorder, th)
    f = ComplexTapsFarrowRestated(hLen, th, rate, Nphi, polyorder, pnfb, tx=tx)
    rt = np.float32 if th == np.complex64 else np.float64
    hr = np.zeros(hLen, dtype=rt)
    xt = np.float32 if tx == np.complex64 else np.float64
    ore = O.FIRFilter(hr, rate, Nphi, tx=xt, polyorder=polyorder, pnfb=np.ascontiguousarray(f.pnfb.real))
    oim = O.FIRFilter(hr, rate, Nphi, tx=xt, polyorder=polyorder, pnfb=np.ascontiguousarray(f.pnfb.imag))
    # the oracle's own schedule, then its currentTaps at the phase of every output (set_state evaluates tapsforphase!)
    sched = f.schedule(120)
    assert len(sched) >= 50
    o_sched = ore.filt(np.zeros(120, dtype=xt), return_schedule=True)[1]
    assert len(o_sched) == len(sched)
    phases = [s[1] for s in sched]
    tr, ti = f._tap_arrays(phases)
    for k, (n, phase) in enumerate(sched):
        assert (n, phase) == (o_sched["xIdx"][k], o_sched["phiIdx"][k] + o_sched["alpha"][k])
        ore.set_state(1, 1, phase)
        oim.set_state(1, 1, phase)
        t = f.tapsforphase(phase)
        assert t.dtype == th
        assert_bit_equal(np.ascontiguousarray(t.real), ore.current_taps(), f"re(taps) of output {k}")
        assert_bit_equal(np.ascontiguousarray(t.imag), oim.current_taps(), f"im(taps) of output {k}")
        assert_bit_equal(tr[k].astype(rt), ore.current_taps(), f"array evaluation, re(taps) of output {k}")
        assert_bit_equal(ti[k].astype(rt), oim.current_taps(), f"array evaluation, im(taps) of output {k}")


def test_short_input_branch_and_empty_input(O, pkg):
    """src/Filters.jl:805-809: a call shorter than inputDeficit only shifts the history and reduces the deficit (rate 0.1:
    nine samples in ten produce nothing)"""
    h, pnfb = _bank(pkg, 3, 4, 12, 2, np.complex64)
    x = (np.random.default_rng(3).random(60) - 0.5).astype(np.float32)
    f = ComplexTapsFarrowRestated(12, np.complex64, 0.1, 4, 2, pnfb, tx=np.float32)
    o = O.FIRFilter(np.zeros(12, np.float32), 0.1, 4, tx=np.float32, polyorder=2, pnfb=np.ascontiguousarray(f.pnfb.real))
    short = 0
    for a, b in _chunks(60, [1, 3, 0, 2, 1, 4, 3]):
        short += f.inputDeficit > b - a
        y, yo = f.filt(x[a:b]), o.filt(x[a:b])
        assert_bit_equal(np.ascontiguousarray(y.real), yo, f"chunk [{a}, {b})")
        assert (f.inputDeficit, f.phiAccumulator) == (o.state.inputDeficit, o.state.phiAccumulator)
        assert_bit_equal(f.history_array(), o.history, f"history after [{a}, {b})")
    assert short >= 4


def test_both_mod_forms_follow_the_oracle(O, pkg):
    """update()'s mod() (src/Filters.jl:785) in both forms (mrhip_set_mod_form); N𝜙 = 5 is no power of two, so they differ"""
    h, pnfb = _bank(pkg, 4, 5, 18, 2, np.complex128)
    x = np.random.default_rng(4).random(3000) - 0.5
    accs = []
    for form in (0, 1):
        f = ComplexTapsFarrowRestated(18, np.complex128, math.pi / 3, 5, 2, pnfb, tx=np.float64, mod_form=form)
        O.set_mod_form(bool(form))
        try:
            o = O.FIRFilter(np.zeros(18), math.pi / 3, 5, tx=np.float64, polyorder=2, pnfb=np.ascontiguousarray(f.pnfb.imag))
            y, yo = f.filt(x, scalar=False), o.filt(x)
            st = o.state
        finally:
            O.set_mod_form(False)
        assert_bit_equal(np.ascontiguousarray(y.imag), yo, f"mod form {form}")
        assert (f.inputDeficit, f.phiAccumulator) == (st.inputDeficit, st.phiAccumulator)
        accs.append(f.phiAccumulator)
    assert accs[0] != accs[1]


def test_the_seam_starts_from_zero_per_component_and_a_continuation_piece_does_not(pkg):
    """x and the history all -0.0, positive taps: every product is -0.0; 0 + (-0.0) = +0.0 on the seam (xIdx < tapsPer𝜙), -0.0
    behind it -- and everywhere in a piece that continues a call"""
    Nphi, T = 4, 3
    pnfb = np.full((T, 1), 1 + 2j)
    x = np.full(8, -0.0, dtype=np.float32)

    def run(continuation):
        f = ComplexTapsFarrowRestated(Nphi * T, np.complex64, 1.0, Nphi, 0, pnfb)
        f.history = [(np.float32(-0.0),)] * f.historyLen
        ys = f.filt(x, continuation=continuation), f.filt(x, scalar=False, continuation=continuation)
        assert_bit_equal(ys[0], ys[1], "array evaluation")
        return ys[0]

    y = run(False)
    assert len(y) == 8
    for part in (y.real, y.imag):
        assert not part.any() and list(np.signbit(part)) == [False] * (T - 1) + [True] * (8 - T + 1)
    y = run(True)
    assert np.signbit(y.real).all() and np.signbit(y.imag).all()


@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex64, np.complex64), (np.complex64, np.float64),
                                   (np.complex128, np.float32), (np.complex64, np.complex128), (np.complex128, np.complex64)])
def test_array_evaluation_of_the_restatement_is_its_scalar_evaluation(pkg, th, tx):
    """the GPU tests evaluate the restatement with array operations (filt(x, scalar=False)): the same bits, state and history"""
    h, pnfb = _bank(pkg, 6, 32, 94, 4, th)
    rng = np.random.default_rng(6)
    x = rng.random(300) - 0.5
    if np.dtype(tx).kind == "c":
        x = x + 1j * (rng.random(300) - 0.5)
    x = x.astype(tx)
    for rate in (0.47, 2.123):
        fs = ComplexTapsFarrowRestated(94, th, rate, 32, 4, pnfb, tx=tx)
        fa = ComplexTapsFarrowRestated(94, th, rate, 32, 4, pnfb, tx=tx)
        for a, b in _chunks(300, [1, 0, 7, 2]):
            assert_bit_equal(fa.filt(x[a:b], scalar=False), fs.filt(x[a:b]), f"rate {rate} chunk [{a}, {b})")
        assert (fa.inputDeficit, fa.phiAccumulator) == (fs.inputDeficit, fs.phiAccumulator)
        assert_bit_equal(fa.history_array(), fs.history_array(), "history")


# ---- the library's host side (no GPU is touched) ----------------------------------------------------------------------------
def test_library_exports_both_new_symbols_and_the_binding_table_has_them(pkg):
    from multirate_jl_amd import host
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    for name, plain in (("mrhip_create_farrow_ctaps", "mrhip_create_farrow"), ("mrhip_create_farrow_pnfb_ctaps", "mrhip_create_farrow_pnfb")):
        assert hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(const (void|double) \*\w+, int64_t hLen, int tap_dtype", hdr)
        entry = [e for e in host.ABI if e[0] == name]
        real = [e for e in host.ABI if e[0] == plain]
        assert len(entry) == 1 and entry[0][1:] == real[0][1:]                  # same signature as the real-tap constructor
        assert f"ccall((:{name}, libmr), Cint," in jl
    assert re.search(r"function FIRFilter\(h::Vector\{Th\}, rate::AbstractFloat, Nphi::Integer, polyorder::Integer; device::Integer = 0\) "
                     r"where \{Th<:Union\{ComplexF32,ComplexF64\}\}", jl)


def test_complex_taps_farrow_constructor_without_a_gpu(pkg):
    f = pkg.FIRFilter.complex_taps_farrow(np.ones(70, dtype=np.complex64), 1.5, 32, 4)
    assert f.kernel_name == "FIRFarrow" and f.h.dtype == np.complex64 and f.polyorder == 4
    assert (f.tapsPerPhi, f.historyLen, f.Nphi) == (3, 2, 32)
    f = pkg.FIRFilter.complex_taps_farrow(np.ones(30, dtype=np.float64), 0.47, 4, 2)          # real h is promoted
    assert f.h.dtype == np.complex128 and (f.tapsPerPhi, f.historyLen, f.Nphi) == (8, 7, 4)
    st = f.state
    assert (st.phiIdx, st.inputDeficit, st.phiAccumulator, st.rate) == (1, 1, 1.0, 0.47)
    f = pkg.FIRFilter.complex_taps_farrow(np.ones(8, dtype=np.complex64), 2.0, 4, 1, pnfb=np.ones((2, 2)))
    assert f._pnfb_in.dtype == np.complex128 and f._pnfb_in.shape == (2, 2)
    for bad, kw in (((np.ones(4, dtype=np.complex64), Fraction(3, 2), 4, 2), {}),             # a Rational ratio
                    ((np.ones(4, dtype=np.complex64), 3, 4, 2), {}),
                    ((np.ones(4, dtype=np.complex64), 1.5, 4, None), {}),                     # no polyorder
                    ((np.ones(4, dtype=np.complex64), -1.0, 4, 2), {}),                       # "rate must be greater than 0"
                    ((np.ones(8, dtype=np.complex64), 2.0, 4, 1), {"pnfb": np.ones((3, 2))})):  # a bank of another shape
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.complex_taps_farrow(*bad, **kw)
        assert e.value.code == 1
    with pytest.raises(TypeError):
        pkg.FIRFilter.complex_taps_farrow(np.ones(4, dtype=np.complex64), 1.5, 4)             # polyorder is not optional


def test_the_existing_constructors_keep_refusing(pkg):
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.complex_taps(np.ones(4, dtype=np.complex64), 1.5)
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError, match="complex_taps") as e:
        pkg.FIRFilter(np.ones(4, dtype=np.complex64), 1.5, 4, 2)
    assert e.value.code == 5


def test_real_tap_dtype_is_an_invalid_argument_before_any_device_is_looked_for(pkg):
    lib = pkg.load_library()
    h = np.ones(8, dtype=np.float64)
    out = C.c_void_p()
    for th in (0, 1):
        assert lib.mrhip_create_farrow_ctaps(h.ctypes.data_as(C.c_void_p), 8, th, 1.5, 4, 2, 0, 1, 0, C.byref(out)) == 1
        assert not out.value and "mrhip_create_farrow" in lib.mrhip_last_error().decode()
        assert lib.mrhip_create_farrow_pnfb_ctaps(h.ctypes.data_as(C.c_void_p), 8, th, 1.5, 4, 1, 0, 1, 0, C.byref(out)) == 1
        assert not out.value and "mrhip_create_farrow_pnfb" in lib.mrhip_last_error().decode()
