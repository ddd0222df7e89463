"""Restatement of the rational family with COMPLEX taps -- test infrastructure, pure NumPy scalar arithmetic.

The reference is generic over the tap type (FIRFilter(h::Vector, ratio), src/Filters.jl:158-180; the unsafedot methods,
src/support.jl:5-55, only multiply and add), but the C oracle under oracle/ refuses complex taps, so the tests of the
complex-tap kernels carry this model of the contract in include/multirate_hip.h ("Complex taps"):

    R = Float64 if either side is 64-bit, else Float32; every multiply, add and subtract is ONE scalar operation in R
    the window [history ; x] is visited oldest sample first; the first product initialises the accumulator
    FIRStandard / FIRDecimator outputs on the seam start from zero: 0 + p per component (support.jl:46)
    real sample x, tap (hr, hi):      p = (hr*x, hi*x)                           Julia's Complex*Real
    complex sample (xr, xi):          p = (hr*xr - hi*xi, hr*xi + hi*xr)         Julia's Complex*Complex
    acc = acc + p, component-wise

The state machine (counts, phase, deficit, history) is the loop of src/Filters.jl:536-575 written once for the four kinds:
L == 1 and / or M == 1 make it the FIRStandard, FIRDecimator and FIRInterpolator loops.  tests/test_complex_taps_cpu.py
pins this file to the untouched oracle wherever the two overlap.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def real_type(th, tx):
    f64 = np.dtype(th) == np.complex128 or np.dtype(tx) in (np.dtype(np.float64), np.dtype(np.complex128))
    return np.float64 if f64 else np.float32


def taps2pfb(h, Nphi):
    """src/Filters.jl:284-298: tapsPerPhi x Nphi, rows filled from the last one up, zero past the end"""
    hLen = len(h)
    T = -(-hLen // Nphi)
    pfb = np.zeros((T, Nphi), dtype=h.dtype)
    hIdx = 0
    for row in range(T - 1, -1, -1):
        for col in range(Nphi):
            if hIdx < hLen:
                pfb[row, col] = h[hIdx]
            hIdx += 1
    return pfb


class ComplexTapsRestated:
    """FIRFilter(h::Vector{Complex}, ratio) and filt(self, x), one channel."""

    def __init__(self, h, ratio=Fraction(1, 1), tx=np.float32):
        h = np.ascontiguousarray(h)
        assert h.dtype in (np.complex64, np.complex128)
        self.th, self.tx = h.dtype, np.dtype(tx)
        self.cplx_x = self.tx.kind == "c"
        R = self.R = real_type(self.th, self.tx)
        self.out_dtype = np.dtype(np.complex128 if R is np.float64 else np.complex64)
        r = Fraction(ratio)
        self.L, self.M, self.hLen = r.numerator, r.denominator, len(h)
        self.kind = ("standard" if r == 1 else "decimator" if self.L == 1 else "interpolator" if self.M == 1 else "rational")
        pfb = taps2pfb(h, self.L)              # L == 1: one column, h reversed (flipud, Filters.jl:21, :53)
        self.T = pfb.shape[0]
        # taps widened exactly to R, as (re, im) scalars: cols[phi][i]
        self.cols = [[(R(pfb[i, c].real), R(pfb[i, c].imag)) for i in range(self.T)] for c in range(self.L)]
        self.historyLen = self.T - 1
        self.history = [self._widen(self.tx.type(0))] * self.historyLen
        self.phiIdx, self.inputDeficit = 1, 1

    def _widen(self, v):
        R = self.R
        return (R(v.real), R(v.imag)) if self.cplx_x else (R(v),)

    @staticmethod
    def _product(t, x):
        hr, hi = t
        if len(x) == 1:
            return (hr * x[0], hi * x[0])
        xr, xi = x
        return (hr * xr - hi * xi, hr * xi + hi * xr)

    def _dot(self, col, ext, n, zero_start):
        """output whose newest sample is x[n] (1-based): window ext[n - 1 .. n - 1 + T) of ext = [history ; x]"""
        acc = self._product(col[0], ext[n - 1])
        if zero_start:
            acc = (self.R(0) + acc[0], self.R(0) + acc[1])
        for i in range(1, self.T):
            p = self._product(col[i], ext[n - 1 + i])
            acc = (acc[0] + p[0], acc[1] + p[1])
        return acc

    def filt(self, x):
        x = np.ascontiguousarray(x, dtype=self.tx)
        xs = [self._widen(v) for v in x]
        xLen = len(xs)
        out = []
        if xLen < self.inputDeficit:                    # Filters.jl:543-547 (and nothing at all for an empty x)
            self.inputDeficit -= xLen
        else:
            ext = self.history + xs
            seam_below = self.hLen + 1 if self.kind == "standard" else self.hLen if self.kind == "decimator" else 0
            inputIdx, phi = self.inputDeficit, self.phiIdx
            while inputIdx <= xLen:
                out.append(self._dot(self.cols[phi - 1], ext, inputIdx, inputIdx < seam_below))
                inputIdx += (phi + self.M - 1) // self.L
                phi += self.M % self.L                  # nextphase, Filters.jl:433-439
                if phi > self.L:
                    phi -= self.L
            self.inputDeficit = inputIdx - xLen
            self.phiIdx = phi
        if self.historyLen:                             # shiftin!, support.jl:61-80
            self.history = (self.history + xs)[-self.historyLen:]
        if not out:
            return np.zeros(0, self.out_dtype)
        y = np.empty(len(out), dtype=self.out_dtype)
        y.real = [o[0] for o in out]
        y.imag = [o[1] for o in out]
        return y

    def history_array(self):
        if self.cplx_x:
            return np.array([complex(float(v[0]), float(v[1])) for v in self.history], dtype=np.complex128).astype(self.tx)
        return np.array([v[0] for v in self.history], dtype=self.tx)
