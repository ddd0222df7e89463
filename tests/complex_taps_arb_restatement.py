"""Restatement of FIRArbitrary with COMPLEX taps -- test infrastructure, pure NumPy scalar arithmetic, one channel.

The reference is generic over the tap type (FIRArbitrary(h::Vector, rate, N𝜙), src/Filters.jl:105-117; update, tapsforphase!
and filt!, :663-742, only take differences, multiply and add), but the C oracle under oracle/ refuses complex taps, so the
tests of kernels_ctaps_arb.hip carry this model of the contract in include/multirate_hip.h ("Complex taps", FIRArbitrary):

    dh = [diff(h), 0] per component in the tap type; pfb, dpfb = taps2pfb(h, N𝜙), taps2pfb(dh, N𝜙)
    R = Float64 if either side is 64-bit, else Float32; the taps are widened exactly to R
    yLower, yUpper: two dot products over ONE window with pfb[:, 𝜙Idx] and dpfb[:, 𝜙Idx], each exactly as the rational
        family's (complex_taps_restatement.py): oldest sample first, the first product initialises the accumulator (no
        start-from-zero seam: FIRArbitrary's seam method is the Matrix one, support.jl:16-31), every operation one scalar
        operation in R
    buffer[k] = yLower + yUpper * α, α::Float64: per component  y_c = R(Float64(lo_c) + Float64(up_c) * α)
    update() in Float64 (:663-673), with either form of mod() (mrhip_set_mod_form)
    tapsforphase: per component  Th(Float64(pfb_c) + α * Float64(dpfb_c))    (:677-688)

tests/test_complex_taps_arb_cpu.py pins this file to the untouched oracle wherever the two overlap.
"""
from __future__ import annotations

import math

import numpy as np

from complex_taps_restatement import ComplexTapsRestated, real_type, taps2pfb


class ComplexTapsArbitraryRestated:
    """FIRFilter(h::Vector{Complex}, rate::Float64, N𝜙) and filt(self, x), one channel."""

    def __init__(self, h, rate, Nphi=32, tx=np.float32, mod_form=0):
        h = np.ascontiguousarray(h)
        assert h.dtype in (np.complex64, np.complex128)
        assert rate > 0.0                                   # "rate must be greater than 0", Filters.jl:184
        self.th, self.tx = h.dtype, np.dtype(tx)
        self.cplx_x = self.tx.kind == "c"
        R = self.R = real_type(self.th, self.tx)
        self.out_dtype = np.dtype(np.complex128 if R is np.float64 else np.complex64)
        # dh = [diff(h), 0] (Filters.jl:106): numpy's complex subtraction is one subtraction per component in the tap type
        dh = np.zeros_like(h)
        dh[:-1] = h[1:] - h[:-1]
        self.Nphi, self.hLen = int(Nphi), len(h)
        self.pfb, self.dpfb = taps2pfb(h, self.Nphi), taps2pfb(dh, self.Nphi)
        self.T = self.pfb.shape[0]
        widen = lambda m: [[(R(m[i, c].real), R(m[i, c].imag)) for i in range(self.T)] for c in range(self.Nphi)]
        self.cols, self.dcols = widen(self.pfb), widen(self.dpfb)
        self.historyLen = self.T - 1
        self.history = [self._widen(self.tx.type(0))] * self.historyLen
        self.rate = float(rate)
        self.delta = float(self.Nphi) / self.rate           # Δ = N𝜙/rate, Filters.jl:113
        self.mod_form = mod_form
        self.reset_state()

    def reset_state(self):
        self.phiAccumulator, self.phiIdx, self.alpha = 1.0, 1, 0.0          # Filters.jl:110-115
        self.xIdx, self.inputDeficit = 1, 1

    def reset(self):
        self.reset_state()
        self.history = [self._widen(self.tx.type(0))] * self.historyLen

    def _widen(self, v):
        R = self.R
        return (R(v.real), R(v.imag)) if self.cplx_x else (R(v),)

    def _mod(self, x, y):
        r = math.fmod(x, y)                                 # exact remainder (operands are positive here): Julia >= 0.4
        return r if not self.mod_form else math.fmod(y + r, y)   # rem(y + rem(x, y), y): Julia Base before 0.4

    def update(self):
        """src/Filters.jl:663-673, Float64 throughout"""
        N = float(self.Nphi)
        self.phiAccumulator += self.delta
        if self.phiAccumulator > N:
            self.xIdx += int(math.floor((self.phiAccumulator - 1.0) / N))
            self.phiAccumulator = self._mod(self.phiAccumulator - 1.0, N) + 1.0
        self.phiIdx = int(math.floor(self.phiAccumulator))
        self.alpha = self.phiAccumulator - self.phiIdx

    def _dot(self, col, ext, n):
        """window ext[n - 1 .. n - 1 + T) of ext = [history ; x] for the output whose newest sample is x[n] (1-based)"""
        product = ComplexTapsRestated._product
        acc = product(col[0], ext[n - 1])
        for i in range(1, self.T):
            p = product(col[i], ext[n - 1 + i])
            acc = (acc[0] + p[0], acc[1] + p[1])
        return acc

    def filt(self, x, scalar=True):
        """src/Filters.jl:693-742.  scalar=True: every output by scalar operations, as the loop states them.  scalar=False: the
        same operations in the same order as NumPy array operations over all outputs of the call at once (each array operation
        rounds every element once in its dtype, so the results are the same bits: tests/test_complex_taps_arb_cpu.py checks) --
        for the GPU tests, whose calls have up to 16 000 outputs of 32 taps."""
        x = np.ascontiguousarray(x, dtype=self.tx)
        xs = [self._widen(v) for v in x]
        xLen = len(xs)
        sched = []                                          # (xIdx, 𝜙Idx, α) per output
        if xLen < self.inputDeficit:                        # :705-709 (and nothing at all for an empty x)
            self.inputDeficit -= xLen
        else:
            self.xIdx = self.inputDeficit                   # :715
            while self.xIdx <= xLen:
                sched.append((self.xIdx, self.phiIdx, self.alpha))
                self.update()
            self.inputDeficit = self.xIdx - xLen            # :734
        ext = self.history + xs
        out = self._outputs_scalar(ext, sched) if scalar else self._outputs_arrays(ext, sched)
        if self.historyLen:                                 # shiftin!, support.jl:61-80
            self.history = ext[-self.historyLen:]
        return out

    def _outputs_scalar(self, ext, sched):
        R = self.R
        y = np.empty(len(sched), dtype=self.out_dtype)
        for k, (n, phi, alpha) in enumerate(sched):
            lo = self._dot(self.cols[phi - 1], ext, n)
            up = self._dot(self.dcols[phi - 1], ext, n)
            a = np.float64(alpha)
            re = R(np.float64(lo[0]) + np.float64(up[0]) * a)                   # :730
            im = R(np.float64(lo[1]) + np.float64(up[1]) * a)
            y[k] = complex(re, im)
        return y

    def _outputs_arrays(self, ext, sched):
        R = self.R
        y = np.empty(len(sched), dtype=self.out_dtype)
        if not sched:
            return y
        n = np.array([s[0] for s in sched], dtype=np.int64)
        phi = np.array([s[1] for s in sched], dtype=np.int64) - 1
        alpha = np.array([s[2] for s in sched], dtype=np.float64)
        e = [np.array([v[c] for v in ext], dtype=R) for c in range(2 if self.cplx_x else 1)]
        banks = []
        for m in (self.pfb, self.dpfb):                     # [phi, i] -> R, exactly widened
            banks.append((np.ascontiguousarray(m.real.T).astype(R), np.ascontiguousarray(m.imag.T).astype(R)))

        def product(hr, hi, idx):
            if not self.cplx_x:
                xr = e[0][idx]
                return hr * xr, hi * xr
            xr, xi = e[0][idx], e[1][idx]
            return hr * xr - hi * xi, hr * xi + hi * xr

        dots = []
        for br, bi in banks:
            acc = product(br[phi, 0], bi[phi, 0], n - 1)
            for i in range(1, self.T):
                p = product(br[phi, i], bi[phi, i], n - 1 + i)
                acc = (acc[0] + p[0], acc[1] + p[1])
            assert acc[0].dtype == R and acc[1].dtype == R
            dots.append(acc)
        (lo_r, lo_i), (up_r, up_i) = dots
        y.real = (lo_r.astype(np.float64) + up_r.astype(np.float64) * alpha).astype(R)
        y.imag = (lo_i.astype(np.float64) + up_i.astype(np.float64) * alpha).astype(R)
        return y

    def tapsforphase(self, phase):
        """src/Filters.jl:677-688: pfb[i, 𝜙Idx] + α * dpfb[i, 𝜙Idx] in Float64 per component, stored in the tap type"""
        assert 0 <= phase <= self.Nphi + 1
        alpha, idx = math.modf(float(phase))
        col = int(idx) - 1
        rt = np.float32 if self.th == np.complex64 else np.float64
        out = np.empty(self.T, dtype=self.th)
        a = np.float64(alpha)
        for i in range(self.T):
            p, d = self.pfb[i, col], self.dpfb[i, col]
            re = rt(np.float64(p.real) + a * np.float64(d.real))
            im = rt(np.float64(p.imag) + a * np.float64(d.imag))
            out[i] = complex(re, im)
        return out

    def history_array(self):
        if self.cplx_x:
            return np.array([complex(float(v[0]), float(v[1])) for v in self.history], dtype=np.complex128).astype(self.tx)
        return np.array([v[0] for v in self.history], dtype=self.tx)
