"""Pins tests/complex_taps_restatement.py (the model the GPU tests of the complex-tap kernels compare with) to the untouched
C oracle wherever the two overlap -- the oracle refuses complex taps, so the overlap is by components:

* real samples: Complex*Real is two independent real chains, so re(y) / im(y) are, BIT FOR BIT, the oracle's outputs with the
  taps real(h) / imag(h) (counts, state and history too);
* complex samples, imag(h) = 0 or real(h) = 0: half of every product is an exact zero, and adding a zero never changes a
  non-zero sum, so the restatement equals the real-tap oracle BY VALUE (==: the sign of a zero may differ).

No GPU: everything here is the restatement, the oracle and the library's host-only helpers.
"""
from fractions import Fraction

import numpy as np
import pytest

from complex_taps_restatement import ComplexTapsRestated, taps2pfb
from conftest import assert_bit_equal

# (L, M, hLen): FIRStandard, FIRDecimator, FIRInterpolator, FIRRational
SHAPES = [(1, 1, 17), (1, 3, 33), (4, 1, 30), (3, 2, 50)]
CHUNKINGS = {"whole": None, "ragged": [1, 0, 7, 2], "prime": 97}
X_LEN = 400


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
    h = (rng.standard_normal(hLen) + 1j * rng.standard_normal(hLen)) / hLen
    return h.astype(dt)


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("th,tx", [(np.complex64, np.float32), (np.complex128, np.float64)])
@pytest.mark.parametrize("L,M,hLen", SHAPES)
def test_real_samples_are_two_real_tap_oracle_runs(O, L, M, hLen, th, tx, chunking):
    rng = np.random.default_rng(hLen)
    h = _taps(rng, hLen, th)
    x = (rng.random(X_LEN) - 0.5).astype(tx)
    ratio = Fraction(L, M)
    f = ComplexTapsRestated(h, ratio, tx=tx)
    ore = O.FIRFilter(np.ascontiguousarray(h.real), ratio, tx=tx)
    oim = O.FIRFilter(np.ascontiguousarray(h.imag), ratio, tx=tx)
    for a, b in _chunks(X_LEN, CHUNKINGS[chunking]):
        y = f.filt(x[a:b])
        yr, yi = ore.filt(x[a:b]), oim.filt(x[a:b])
        assert y.dtype == (np.complex64 if tx == np.float32 else np.complex128)
        assert len(y) == len(yr) == len(yi), (a, b)
        assert_bit_equal(np.ascontiguousarray(y.real), yr, f"re(y), chunk [{a}, {b})")
        assert_bit_equal(np.ascontiguousarray(y.imag), yi, f"im(y), chunk [{a}, {b})")
        so = ore.state
        if f.kind in ("decimator", "rational"):
            assert f.inputDeficit == so.inputDeficit
        if f.kind == "rational":
            assert f.phiIdx == so.phiIdx
    assert_bit_equal(f.history_array(), ore.history, "history")


@pytest.mark.parametrize("th,tx", [(np.complex64, np.complex64), (np.complex128, np.complex128), (np.complex64, np.complex128)])
@pytest.mark.parametrize("L,M,hLen", SHAPES)
def test_complex_samples_purely_real_taps_equal_the_real_tap_oracle(O, L, M, hLen, th, tx):
    rng = np.random.default_rng(100 + hLen)
    hr = (rng.standard_normal(hLen) / hLen).astype(np.float32 if th == np.complex64 else np.float64)
    x = (rng.random(X_LEN) + 1j * rng.random(X_LEN)).astype(tx)            # samples in [0, 1)
    ratio = Fraction(L, M)
    f = ComplexTapsRestated(hr.astype(th), ratio, tx=tx)
    o = O.FIRFilter(hr, ratio, tx=tx)
    for a, b in _chunks(X_LEN, 97):
        y, yo = f.filt(x[a:b]), o.filt(x[a:b])
        assert y.dtype == yo.dtype and y.shape == yo.shape
        assert np.all(y == yo), f"chunk [{a}, {b})"


@pytest.mark.parametrize("th,tx", [(np.complex64, np.complex64), (np.complex128, np.complex128), (np.complex64, np.complex128)])
@pytest.mark.parametrize("L,M,hLen", SHAPES)
def test_complex_samples_purely_imaginary_taps_equal_the_real_tap_oracle(O, L, M, hLen, th, tx):
    rng = np.random.default_rng(200 + hLen)
    rt = np.float32 if th == np.complex64 else np.float64
    hi = (rng.standard_normal(hLen) / hLen).astype(rt)
    x = (rng.random(X_LEN) + 1j * rng.random(X_LEN)).astype(tx)            # samples in [0, 1)
    xt = np.float32 if tx == np.complex64 else np.float64
    ratio = Fraction(L, M)
    f = ComplexTapsRestated((1j * hi).astype(th), ratio, tx=tx)
    o_im = O.FIRFilter(hi, ratio, tx=xt)     # over imag(x): -re(y)
    o_re = O.FIRFilter(hi, ratio, tx=xt)     # over real(x):  im(y)
    for a, b in _chunks(X_LEN, 97):
        y = f.filt(x[a:b])
        y_from_im = o_im.filt(np.ascontiguousarray(x[a:b].imag))
        y_from_re = o_re.filt(np.ascontiguousarray(x[a:b].real))
        assert y.shape == y_from_im.shape == y_from_re.shape
        assert y.real.dtype == y_from_im.dtype
        assert np.all(y.real == -y_from_im), f"re(y), chunk [{a}, {b})"
        assert np.all(y.imag == y_from_re), f"im(y), chunk [{a}, {b})"


def test_restated_taps2pfb_is_the_oracles_by_components(O):
    h = (np.arange(1, 11) + 1j * np.arange(11, 21)).astype(np.complex128)
    pfb = taps2pfb(h, 4)
    assert np.array_equal(pfb.real, O.taps2pfb(np.ascontiguousarray(h.real), 4))
    assert np.array_equal(pfb.imag, O.taps2pfb(np.ascontiguousarray(h.imag), 4))


# ---- the library's host logic (no GPU is touched) ---------------------------------------------------------------------------
def test_output_dtype_with_complex_taps(pkg):
    lib = pkg.load_library()
    F32, F64, C64, C128 = 0, 1, 2, 3
    for tx in (F32, F64, C64, C128):
        assert lib.mrhip_output_dtype(C64, tx) == (C128 if tx in (F64, C128) else C64)
        assert lib.mrhip_output_dtype(C128, tx) == C128
    # real taps: unchanged
    assert [lib.mrhip_output_dtype(F32, tx) for tx in (F32, F64, C64, C128)] == [F32, F64, C64, C128]
    assert [lib.mrhip_output_dtype(F64, tx) for tx in (F32, F64, C64, C128)] == [F64, F64, C128, C128]


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_taps2pfb_of_the_doc_example_with_complex_entries(pkg, dt):
    """taps2pfb([1:10], 4) (src/Filters.jl:271-282) with h[k] = k + (10 + k)im: the matrix of the example in both parts"""
    h = (np.arange(1, 11) + 1j * np.arange(11, 21)).astype(dt)
    pfb = pkg.taps2pfb(h, 4)
    want_re = np.array([[9, 10, 0, 0], [5, 6, 7, 8], [1, 2, 3, 4]], dtype=float)
    want_im = np.where(want_re > 0, want_re + 10, 0)
    assert pfb.dtype == dt and pfb.shape == (3, 4)
    assert np.array_equal(pfb.real, want_re) and np.array_equal(pfb.imag, want_im)
    assert np.array_equal(pfb, taps2pfb(h, 4))


def test_plain_constructor_still_refuses_complex_taps_and_names_the_new_one(pkg):
    with pytest.raises(pkg.MultirateHIPError, match="complex_taps") as e:
        pkg.FIRFilter(np.ones(4, dtype=np.complex64))
    assert e.value.code == 5


def test_complex_taps_constructor_without_a_gpu(pkg):
    f = pkg.FIRFilter.complex_taps(np.ones(7, dtype=np.complex64), Fraction(3, 2))
    assert f.kernel_name == "FIRRational" and f.h.dtype == np.complex64
    assert (f.tapsPerPhi, f.historyLen, f.Nphi) == (3, 2, 3)
    assert pkg.FIRFilter.complex_taps(np.ones(4, dtype=np.float64)).h.dtype == np.complex128     # real h is promoted
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.complex_taps(np.ones(4, dtype=np.complex64), 1.5)                          # float rate: FIRArbitrary
    assert e.value.code == 5
