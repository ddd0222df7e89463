"""Pins tests/complex_taps_arb_restatement.py (the model the GPU tests of kernels_ctaps_arb.hip compare with) to the untouched
C oracle wherever the two overlap -- the oracle refuses complex taps, so the overlap is by components:

* real samples: diff, both dot products and the combine yLower + yUpper * α are all per component, so re(y) / im(y) are, BIT
  FOR BIT, the oracle's FIRArbitrary outputs with the taps real(h) / imag(h) (counts, 𝜙Accumulator, inputDeficit and history too);
* complex samples, imag(h) = 0 or real(h) = 0: half of every product is an exact zero, and adding a zero never changes a
  non-zero sum, so the restatement equals the real-tap oracle BY VALUE (==: the sign of a zero may differ).

No GPU: everything here is the restatement, the oracle and the library's host-only parts.
"""
import math
import os
import re

import numpy as np
import pytest

from complex_taps_arb_restatement import ComplexTapsArbitraryRestated
from conftest import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [0.47, 1.0, 2 * math.pi / 3]                 # one < 1, the identity, one > 1 and irrational
NPHIS = [4, 32]
TAPS_PER_PHI = [1, 3, 8]                             # T = 1: no history
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
X_LEN = 400


def _hlen(Nphi, T):
    return Nphi * T - (2 if T > 1 else 0)            # not a multiple of Nphi: the bank's last row is zero padded


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


def _taps(rng, hLen, dt):
    return ((rng.standard_normal(hLen) + 1j * rng.standard_normal(hLen)) / hLen).astype(dt)


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.float64)])
@pytest.mark.parametrize("T", TAPS_PER_PHI)
@pytest.mark.parametrize("Nphi", NPHIS)
@pytest.mark.parametrize("rate", RATES)
def test_real_samples_are_two_real_tap_oracle_runs(O, rate, Nphi, T, th, tx, chunking):
    hLen = _hlen(Nphi, T)
    rng = np.random.default_rng(hLen)
    h = _taps(rng, hLen, th)
    x = (rng.random(X_LEN) - 0.5).astype(tx)
    f = ComplexTapsArbitraryRestated(h, rate, Nphi, tx=tx)
    assert (f.T, f.historyLen) == (T, T - 1)
    ore = O.FIRFilter(np.ascontiguousarray(h.real), rate, Nphi, tx=tx)
    oim = O.FIRFilter(np.ascontiguousarray(h.imag), rate, Nphi, tx=tx)
    for a, b in _chunks(X_LEN, CHUNKINGS[chunking]):
        y = f.filt(x[a:b])
        yr, yi = ore.filt(x[a:b]), oim.filt(x[a:b])
        assert y.dtype == (np.complex64 if tx == np.float32 else np.complex128)
        assert len(y) == len(yr) == len(yi), (a, b)
        assert_bit_equal(np.ascontiguousarray(y.real), yr, f"re(y), chunk [{a}, {b})")
        assert_bit_equal(np.ascontiguousarray(y.imag), yi, f"im(y), chunk [{a}, {b})")
        so = ore.state
        assert f.inputDeficit == so.inputDeficit, (a, b)
        assert f.phiAccumulator == so.phiAccumulator, (a, b)
    assert_bit_equal(f.history_array(), ore.history, "history")


@pytest.mark.parametrize("th,tx", [(np.complex64, np.complex64), (np.complex64, np.complex128)])
@pytest.mark.parametrize("T", TAPS_PER_PHI)
@pytest.mark.parametrize("Nphi", NPHIS)
@pytest.mark.parametrize("rate", RATES)
def test_complex_samples_purely_real_taps_equal_the_real_tap_oracle(O, rate, Nphi, T, th, tx):
    hLen = _hlen(Nphi, T)
    rng = np.random.default_rng(100 + hLen)
    hr = (rng.standard_normal(hLen) / hLen).astype(np.float32)
    x = (rng.random(X_LEN) + 1j * rng.random(X_LEN)).astype(tx)            # samples in [0, 1)
    f = ComplexTapsArbitraryRestated(hr.astype(th), rate, Nphi, tx=tx)
    o = O.FIRFilter(hr, rate, Nphi, tx=tx)
    for a, b in _chunks(X_LEN, 97):
        y, yo = f.filt(x[a:b]), o.filt(x[a:b])
        assert y.dtype == yo.dtype and y.shape == yo.shape
        assert np.all(y == yo), f"chunk [{a}, {b})"
    assert f.phiAccumulator == o.state.phiAccumulator and f.inputDeficit == o.state.inputDeficit


@pytest.mark.parametrize("th,tx", [(np.complex64, np.complex64), (np.complex64, np.complex128)])
@pytest.mark.parametrize("T", TAPS_PER_PHI)
@pytest.mark.parametrize("Nphi", NPHIS)
@pytest.mark.parametrize("rate", RATES)
def test_complex_samples_purely_imaginary_taps_equal_the_real_tap_oracle(O, rate, Nphi, T, th, tx):
    hLen = _hlen(Nphi, T)
    rng = np.random.default_rng(200 + hLen)
    hi = (rng.standard_normal(hLen) / hLen).astype(np.float32)
    x = (rng.random(X_LEN) + 1j * rng.random(X_LEN)).astype(tx)            # samples in [0, 1)
    xt = np.float32 if tx == np.complex64 else np.float64
    f = ComplexTapsArbitraryRestated((1j * hi).astype(th), rate, Nphi, tx=tx)
    o_im = O.FIRFilter(hi, rate, Nphi, tx=xt)     # over imag(x): -re(y)
    o_re = O.FIRFilter(hi, rate, Nphi, tx=xt)     # over real(x):  im(y)
    for a, b in _chunks(X_LEN, 97):
        y = f.filt(x[a:b])
        y_from_im = o_im.filt(np.ascontiguousarray(x[a:b].imag))
        y_from_re = o_re.filt(np.ascontiguousarray(x[a:b].real))
        assert y.shape == y_from_im.shape == y_from_re.shape
        assert y.real.dtype == y_from_im.dtype
        assert np.all(y.real == -y_from_im), f"re(y), chunk [{a}, {b})"
        assert np.all(y.imag == y_from_re), f"im(y), chunk [{a}, {b})"


def test_short_input_branch_and_empty_input(O):
    """src/Filters.jl:705-709: a call shorter than inputDeficit only shifts the history and reduces the deficit (rate 0.1:
    nine samples in ten produce nothing)"""
    rng = np.random.default_rng(3)
    h = _taps(rng, 12, np.complex64)
    x = (rng.random(60) - 0.5).astype(np.float32)
    f = ComplexTapsArbitraryRestated(h, 0.1, 4, tx=np.float32)
    o = O.FIRFilter(np.ascontiguousarray(h.real), 0.1, 4, tx=np.float32)
    short = 0
    for a, b in _chunks(60, [1, 3, 0, 2, 1, 4, 3]):
        short += f.inputDeficit > b - a
        y, yo = f.filt(x[a:b]), o.filt(x[a:b])
        assert_bit_equal(np.ascontiguousarray(y.real), yo, f"chunk [{a}, {b})")
        assert (f.inputDeficit, f.phiAccumulator) == (o.state.inputDeficit, o.state.phiAccumulator)
        assert_bit_equal(f.history_array(), o.history, f"history after [{a}, {b})")
    assert short >= 4


def test_both_mod_forms_follow_the_oracle(O):
    """update()'s mod() (src/Filters.jl:668) in both forms (mrhip_set_mod_form); N𝜙 = 5 is no power of two, so they differ"""
    rng = np.random.default_rng(4)
    h = _taps(rng, 18, np.complex128)
    x = (rng.random(3000) - 0.5)
    accs = []
    for form in (0, 1):
        f = ComplexTapsArbitraryRestated(h, math.pi / 3, 5, tx=np.float64, mod_form=form)
        O.set_mod_form(bool(form))
        try:
            o = O.FIRFilter(np.ascontiguousarray(h.imag), math.pi / 3, 5, tx=np.float64)
            y, yo = f.filt(x), o.filt(x)
            st = o.state
        finally:
            O.set_mod_form(False)
        assert_bit_equal(np.ascontiguousarray(y.imag), yo, f"mod form {form}")
        assert (f.inputDeficit, f.phiAccumulator) == (st.inputDeficit, st.phiAccumulator)
        accs.append(f.phiAccumulator)
    assert accs[0] != accs[1]


@pytest.mark.parametrize("th", [np.complex64, np.complex128])
def test_banks_and_tapsforphase_are_the_oracles_by_components(O, pkg, th):
    rng = np.random.default_rng(5)
    h = _taps(rng, 30, th)
    f = ComplexTapsArbitraryRestated(h, 1.5, 4)
    ore = O.FIRFilter(np.ascontiguousarray(h.real), 1.5, 4)
    oim = O.FIRFilter(np.ascontiguousarray(h.imag), 1.5, 4)
    for which, bank in ((0, f.pfb), (1, f.dpfb)):
        assert_bit_equal(np.ascontiguousarray(bank.real), ore.taps(which), f"re(bank {which})")
        assert_bit_equal(np.ascontiguousarray(bank.imag), oim.taps(which), f"im(bank {which})")
    # tapsforphase against a direct Float64 evaluation (exact for Complex128 taps up to the stated roundings)
    for phase in (1.0, 1.25, 4.5):
        t = f.tapsforphase(phase)
        a, col = math.modf(phase)
        want = (f.pfb[:, int(col) - 1].astype(np.complex128) + a * f.dpfb[:, int(col) - 1].astype(np.complex128)).astype(th)
        assert t.dtype == th
        assert_bit_equal(t, want, f"tapsforphase({phase})")


@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex64, np.complex64), (np.complex64, np.float64),
                                   (np.complex128, np.float32), (np.complex64, np.complex128), (np.complex128, np.complex64)])
def test_array_evaluation_of_the_restatement_is_its_scalar_evaluation(th, tx):
    """the GPU tests evaluate the restatement with array operations (filt(x, scalar=False)): the same bits, state and history"""
    rng = np.random.default_rng(6)
    h = _taps(rng, 94, th)
    x = rng.random(300) - 0.5
    if np.dtype(tx).kind == "c":
        x = x + 1j * (rng.random(300) - 0.5)
    x = x.astype(tx)
    for rate in (0.47, 2.123):
        fs, fa = ComplexTapsArbitraryRestated(h, rate, 32, tx=tx), ComplexTapsArbitraryRestated(h, rate, 32, tx=tx)
        for a, b in _chunks(300, [1, 0, 7, 2]):
            assert_bit_equal(fa.filt(x[a:b], scalar=False), fs.filt(x[a:b]), f"rate {rate} chunk [{a}, {b})")
        assert (fa.inputDeficit, fa.phiAccumulator) == (fs.inputDeficit, fs.phiAccumulator)
        assert_bit_equal(fa.history_array(), fs.history_array(), "history")


# ---- the library's host side (no GPU is touched) ----------------------------------------------------------------------------
def test_complex_taps_arbitrary_constructor_without_a_gpu(pkg):
    f = pkg.FIRFilter.complex_taps_arbitrary(np.ones(70, dtype=np.complex64), 1.5)
    assert f.kernel_name == "FIRArbitrary" and f.h.dtype == np.complex64
    assert (f.tapsPerPhi, f.historyLen, f.Nphi) == (3, 2, 32)
    f = pkg.FIRFilter.complex_taps_arbitrary(np.ones(30, dtype=np.float64), 0.47, 4)      # real h is promoted
    assert f.h.dtype == np.complex128 and (f.tapsPerPhi, f.historyLen, f.Nphi) == (8, 7, 4)
    assert pkg.FIRFilter.complex_taps_arbitrary(np.ones(4, dtype=np.float32), 2.0, 4).h.dtype == np.complex64
    st = f.state
    assert (st.phiIdx, st.inputDeficit, st.phiAccumulator, st.rate) == (1, 1, 1.0, 0.47)
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.complex_taps_arbitrary(np.ones(4, dtype=np.complex64), -1.0)         # "rate must be greater than 0"
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.complex_taps_arbitrary(np.ones(4, dtype=np.complex64), 2)            # a ratio: complex_taps
    assert e.value.code == 1


def test_the_existing_constructors_keep_refusing(pkg):
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.complex_taps(np.ones(4, dtype=np.complex64), 1.5)
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError, match="complex_taps") as e:
        pkg.FIRFilter(np.ones(4, dtype=np.complex64), 1.5)
    assert e.value.code == 5


def test_real_tap_dtype_is_an_invalid_argument_before_any_device_is_looked_for(pkg):
    import ctypes as C
    lib = pkg.load_library()
    h = np.ones(8, dtype=np.float64)
    out = C.c_void_p()
    for th in (0, 1):
        assert lib.mrhip_create_arbitrary_ctaps(h.ctypes.data_as(C.c_void_p), 8, th, 1.5, 4, 0, 1, 0, C.byref(out)) == 1
        assert not out.value and "mrhip_create_arbitrary" in lib.mrhip_last_error().decode()


def test_new_symbol_is_in_the_header_the_binding_table_and_the_shim(pkg):
    from multirate_jl_amd import host
    name = "mrhip_create_arbitrary_ctaps"
    hdr = open(os.path.join(ROOT, "include", "multirate_hip.h")).read()
    assert re.search(r"\bint " + name + r"\(const void \*h, int64_t hLen, int tap_dtype", hdr)
    entry = [e for e in host.ABI if e[0] == name]
    plain = [e for e in host.ABI if e[0] == "mrhip_create_arbitrary"]
    assert len(entry) == 1 and entry[0][1:] == plain[0][1:]                 # same signature as the real-tap constructor
    assert hasattr(pkg.load_library(), name)
    jl = open(os.path.join(ROOT, "multirate.jl_amd", "julia", "MultirateHIP.jl")).read()
    assert f"ccall((:{name}, libmr), Cint," in jl
    assert re.search(r"function FIRFilter\(h::Vector\{Th\}, rate::AbstractFloat, Nphi::Integer = 32; device::Integer = 0\) "
                     r"where \{Th<:Union\{ComplexF32,ComplexF64\}\}", jl)
