"""Restatement of FIRFarrow with COMPLEX taps -- test infrastructure, pure NumPy scalar arithmetic, one channel.

The reference is generic over the tap type (FIRFarrow(h::Vector, rate, N𝜙, polyorder), src/Filters.jl:138-147; pfb2pnfb,
:311-321; tapsforphase!, update and filt!, :764-839), but the C oracle under oracle/ refuses complex taps, so the tests of
kernels_ctaps_farrow.hip carry this model of the contract in include/multirate_hip.h ("Complex taps", FIRFarrow):

    pnfb: one polynomial per ROW of taps2pfb(h, N𝜙), (tapsPer𝜙, polyorder+1) complex coefficients in ascending powers, fitted
        per component and stored in the tap type per component (Complex64 taps: each component rounded to Float32)
    taps of an output with the Float64 phase 𝜙, tap i, component c: Horner in Float64 from the highest power,
        t = 𝜙*v; v = coef + t  (product and sum each rounded once), the result rounded once to the tap's real scalar
        -- polyval(Poly{Complex{T}}, ::Float64) stored into currentTaps::Vector{Complex{T}}
    R = Float64 if either side is 64-bit, else Float32; the taps are widened exactly to R
    y = ONE dot product over the window exactly as the rational family's (complex_taps_restatement.py): oldest sample first, the
        first product initialises the accumulator, every operation one scalar operation in R; outputs with xIdx < tapsPer𝜙 start
        from zero per component (0 + p, support.jl:46)
    update() in Float64 (:780-788), with either form of mod() (mrhip_set_mod_form); the phase is 𝜙Accumulator itself

tests/test_complex_taps_farrow_cpu.py pins this file to the untouched oracle wherever the two overlap.
"""
from __future__ import annotations

import math

import numpy as np

from complex_taps_restatement import ComplexTapsRestated, real_type, taps2pfb


def fit_pnfb(h, Nphi, polyorder, polyfit):
    """pfb2pnfb (src/Filters.jl:311-321) per component: ``polyfit(row, polyorder)`` -> ascending Float64 coefficients, applied to
    the real parts and to the imaginary parts of every row of taps2pfb(h, N𝜙).  (tapsPer𝜙, polyorder+1) complex128."""
    pfb = taps2pfb(np.ascontiguousarray(h), Nphi)
    out = np.empty((pfb.shape[0], polyorder + 1), dtype=np.complex128)
    for i in range(pfb.shape[0]):
        out[i].real = polyfit(np.ascontiguousarray(pfb[i].real).astype(np.float64), polyorder)
        out[i].imag = polyfit(np.ascontiguousarray(pfb[i].imag).astype(np.float64), polyorder)
    return out


class ComplexTapsFarrowRestated:
    """FIRFilter(h::Vector{Complex}, rate::Float64, N𝜙, polyorder) and filt(self, x), one channel.  The polynomial bank is the
    caller's (``pnfb``: the reference pins no bits of the fit); only length and type of ``h`` are used."""

    def __init__(self, hLen, th, rate, Nphi, polyorder, pnfb, tx=np.float32, mod_form=0):
        self.th, self.tx = np.dtype(th), np.dtype(tx)
        assert self.th in (np.complex64, np.complex128)
        assert rate > 0.0                                   # "rate must be greater than 0", Filters.jl:193
        self.cplx_x = self.tx.kind == "c"
        self.R = real_type(self.th, self.tx)
        self.rt = np.float32 if self.th == np.complex64 else np.float64        # the tap's real scalar
        self.out_dtype = np.dtype(np.complex128 if self.R is np.float64 else np.complex64)
        self.Nphi, self.hLen, self.polyorder = int(Nphi), int(hLen), int(polyorder)
        self.T = -(-self.hLen // self.Nphi)
        pnfb = np.asarray(pnfb, dtype=np.complex128)
        assert pnfb.shape == (self.T, self.polyorder + 1), pnfb.shape
        # Poly{Complex{T}} storage: each component in the tap type, held as Float64
        self.pnfb = np.empty_like(pnfb)
        self.pnfb.real = pnfb.real.astype(self.rt).astype(np.float64)
        self.pnfb.imag = pnfb.imag.astype(self.rt).astype(np.float64)
        self.historyLen = self.T - 1
        self.history = [self._widen(self.tx.type(0))] * self.historyLen
        self.rate = float(rate)
        self.delta = float(self.Nphi) / self.rate           # Δ = N𝜙/rate, Filters.jl:143
        self.mod_form = mod_form
        self.reset_state()

    def reset_state(self):
        self.phiAccumulator = 1.0                           # 𝜙Idx = 1.0, a Float64 for this kernel (Filters.jl:142)
        self.xIdx, self.inputDeficit = 1, 1

    def reset(self):
        self.reset_state()
        self.history = [self._widen(self.tx.type(0))] * self.historyLen

    # bookkeeping the state snapshots carry
    @property
    def phiIdx(self):
        return int(math.floor(self.phiAccumulator))

    @property
    def alpha(self):
        return self.phiAccumulator - self.phiIdx

    def _widen(self, v):
        R = self.R
        return (R(v.real), R(v.imag)) if self.cplx_x else (R(v),)

    def _mod(self, x, y):
        r = math.fmod(x, y)                                 # exact remainder (operands are positive here): Julia >= 0.4
        return r if not self.mod_form else math.fmod(y + r, y)   # rem(y + rem(x, y), y): Julia Base before 0.4

    def update(self):
        """src/Filters.jl:780-788, Float64 throughout (tapsforphase! is evaluated where the taps are used)"""
        N = float(self.Nphi)
        self.phiAccumulator += self.delta
        if self.phiAccumulator > N:
            self.xIdx += int(math.floor((self.phiAccumulator - 1.0) / N))
            self.phiAccumulator = self._mod(self.phiAccumulator - 1.0, N) + 1.0

    def tapsforphase(self, phase):
        """src/Filters.jl:764-773: per component, Horner in Float64 (each product and each sum one np.float64 operation),
        rounded once to the tap's real scalar.  tapsPer𝜙 taps of the tap type."""
        assert 0 <= phase <= self.Nphi + 1
        x = np.float64(phase)
        out = np.empty(self.T, dtype=self.th)
        P = self.polyorder
        for i in range(self.T):
            comp = []
            for part in (self.pnfb[i].real, self.pnfb[i].imag):
                v = np.float64(part[P])
                for j in range(P - 1, -1, -1):
                    t = x * v
                    v = np.float64(part[j]) + t
                comp.append(self.rt(v))
            out[i] = complex(comp[0], comp[1])
        return out

    def _tap_arrays(self, phases):
        """the same statement over all outputs of a call at once: (re, im), each [output, tap] in R"""
        P = self.polyorder
        x = np.asarray(phases, dtype=np.float64)[:, None]
        comp = []
        for part in (self.pnfb.real, self.pnfb.imag):
            v = np.broadcast_to(part[None, :, P], (len(phases), self.T)).astype(np.float64)
            for j in range(P - 1, -1, -1):
                t = x * v
                v = part[None, :, j] + t
            comp.append(v.astype(self.rt).astype(self.R))
        return comp

    def schedule(self, xLen):
        """the (xIdx, 𝜙) pairs of a call of xLen samples; advances the state (src/Filters.jl:805-828)"""
        sched = []
        if xLen < self.inputDeficit:                        # :805-809 (and nothing at all for an empty x)
            self.inputDeficit -= xLen
        else:
            self.xIdx = self.inputDeficit                   # :812
            while self.xIdx <= xLen:
                sched.append((self.xIdx, self.phiAccumulator))
                self.update()
            self.inputDeficit = self.xIdx - xLen            # :828
        return sched

    def filt(self, x, scalar=True, continuation=False):
        """src/Filters.jl:795-839.  scalar=True: every output by scalar operations, as the loop states them.  scalar=False: the
        same operations in the same order as NumPy array operations over all outputs of the call at once (each array operation
        rounds every element once in its dtype: the same bits, tests/test_complex_taps_farrow_cpu.py checks) -- for the GPU
        tests.  continuation: the call continues another one (no seam), as the pieces of a split call do."""
        x = np.ascontiguousarray(x, dtype=self.tx)
        xs = [self._widen(v) for v in x]
        sched = self.schedule(len(xs))
        ext = self.history + xs
        seam_below = 0 if continuation else self.T          # kernel.xIdx < kernel.tapsPer𝜙, :818
        out = self._outputs_scalar(ext, sched, seam_below) if scalar else self._outputs_arrays(ext, sched, seam_below)
        if self.historyLen:                                 # shiftin!, support.jl:61-80
            self.history = ext[-self.historyLen:]
        return out

    def _outputs_scalar(self, ext, sched, seam_below):
        R = self.R
        product = ComplexTapsRestated._product
        y = np.empty(len(sched), dtype=self.out_dtype)
        for k, (n, phase) in enumerate(sched):
            taps = self.tapsforphase(phase)
            col = [(R(t.real), R(t.imag)) for t in taps]
            acc = product(col[0], ext[n - 1])
            if n < seam_below:
                acc = (R(0) + acc[0], R(0) + acc[1])        # support.jl:46
            for i in range(1, self.T):
                p = product(col[i], ext[n - 1 + i])
                acc = (acc[0] + p[0], acc[1] + p[1])
            y[k] = complex(acc[0], acc[1])
        return y

    def _outputs_arrays(self, ext, sched, seam_below):
        R = self.R
        y = np.empty(len(sched), dtype=self.out_dtype)
        if not sched:
            return y
        n = np.array([s[0] for s in sched], dtype=np.int64)
        tr, ti = self._tap_arrays([s[1] for s in sched])
        e = [np.array([v[c] for v in ext], dtype=R) for c in range(2 if self.cplx_x else 1)]

        def product(hr, hi, idx):
            if not self.cplx_x:
                xr = e[0][idx]
                return hr * xr, hi * xr
            xr, xi = e[0][idx], e[1][idx]
            return hr * xr - hi * xi, hr * xi + hi * xr

        acc = product(tr[:, 0], ti[:, 0], n - 1)
        seam = n < seam_below
        acc = (np.where(seam, R(0) + acc[0], acc[0]), np.where(seam, R(0) + acc[1], acc[1]))
        for i in range(1, self.T):
            p = product(tr[:, i], ti[:, i], n - 1 + i)
            acc = (acc[0] + p[0], acc[1] + p[1])
        assert acc[0].dtype == R and acc[1].dtype == R
        y.real, y.imag = acc
        return y

    def history_array(self):
        if self.cplx_x:
            return np.array([complex(float(v[0]), float(v[1])) for v in self.history], dtype=np.complex128).astype(self.tx)
        return np.array([v[0] for v in self.history], dtype=self.tx)
