// rates_farrow_device.h -- what the two FIRFarrow units with per-channel rates share, stated ONCE: kernels_rates_farrow.hip (one
// polynomial bank behind all channels) and kernels_rates_bank_farrow.hip (a bank per channel, mrhip_set_channel_taps_farrow /
// mrhip_set_channel_pnfb).  The rounding of an evaluated tap, the OPL Horner chains of one polynomial and the OPL dots of one lane: the
// units differ only in where a channel's coefficients start.  The including units are compiled with -ffp-contract=off.
#pragma once

#include "rates_arb.h"
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {

// the evaluated tap, stored into currentTaps::Vector{Th} (one rounding to the tap type), widened exactly to R
template <typename R>
__device__ __forceinline__ R farrow_rates_round(const double v, const bool tap_f32)
{
    return tap_f32 ? static_cast<R>(static_cast<float>(v)) : static_cast<R>(v);
}

// OPL Horner chains of ONE polynomial side by side, each at its own phase: the P+1 coefficients are loaded once as scalars and feed all
// the chains, which are independent, so they interleave and cover each other's Float64 latency.  Per chain the statement of
// farrow_bank_horner (variant_device.h): t = 𝜙*v; v = coef + t, the product and the sum each rounded once, never fused.  PP >= 0: the
// polyorder at compile time, the loads issued together and waited for once; PP < 0: any polyorder, one load per Horner step.
template <int PP, int OPL>
__device__ __forceinline__ void farrow_rates_horner(farrow_coef_t c, const int P, const double (&phase)[OPL], double (&v)[OPL])
{
    if constexpr (PP >= 0) {
        double cj[PP + 1];
#pragma unroll
        for (int e = 0; e <= PP; ++e) cj[e] = c[e];
#pragma unroll
        for (int q = 0; q < OPL; ++q) v[q] = cj[PP];
#pragma unroll
        for (int j = PP - 1; j >= 0; --j) {
#pragma unroll
            for (int q = 0; q < OPL; ++q) {
                const double t = phase[q] * v[q];
                v[q] = cj[j] + t;
            }
        }
    } else {
        const double top = c[P];
#pragma unroll
        for (int q = 0; q < OPL; ++q) v[q] = top;
        for (int j = P - 1; j >= 0; --j) {
            const double cj = c[j];
#pragma unroll
            for (int q = 0; q < OPL; ++q) {
                const double t = phase[q] * v[q];
                v[q] = cj + t;
            }
        }
    }
}

// The OPL dots of one lane: per tap ONE evaluation of the coefficients' scalar loads, OPL Horner chains, OPL multiply-adds; sample xi of
// a window comes from x (xi >= 0) or from the end of the history (he[xi], xi < 0).  The first `live` slots are stored.  pc: the first
// coefficient of the polynomial bank the lane's channel reads, [T][P+1].
template <typename A, int PP, int OPL>
__device__ __forceinline__ void farrow_rates_dots(farrow_coef_t pc, const int P, const int T, const bool tap_f32, const double (&phase)[OPL],
                                                  const long long (&base)[OPL], const bool (&seam)[OPL],
                                                  const typename A::Sample *__restrict__ xc, const typename A::Sample *__restrict__ he,
                                                  typename A::Out *__restrict__ yc, const long long k_first, const int live)
{
    using R = typename A::Tap;
    typename A::Sum acc[OPL];
    double v[OPL];
    farrow_rates_horner<PP, OPL>(pc, P, phase, v);
#pragma unroll
    for (int j = 0; j < OPL; ++j) {
        const long long xi = base[j];
        acc[j] = A::first(farrow_rates_round<R>(v[j], tap_f32), xi >= 0 ? xc[xi] : he[xi]);
        if (seam[j]) acc[j] = A::zero_start(acc[j]);
    }
    for (int i = 1; i < T; ++i) {
        farrow_rates_horner<PP, OPL>(pc + i * (P + 1), P, phase, v);
#pragma unroll
        for (int j = 0; j < OPL; ++j) {
            const long long xi = base[j] + i;
            acc[j] = A::step(acc[j], farrow_rates_round<R>(v[j], tap_f32), xi >= 0 ? xc[xi] : he[xi]);
        }
    }
#pragma unroll
    for (int j = 0; j < OPL; ++j)
        if (j < live) A::store(yc, k_first + j * kVariantThreads, acc[j]);
}

}  // namespace mrhip
