// ctaps_device.h -- the arithmetic of the complex-tap kernels (kernels_ctaps.hip, kernels_bank_ctaps.hip: the rational family;
// kernels_ctaps_arb.hip: FIRArbitrary; kernels_ctaps_farrow.hip: FIRFarrow), stated ONCE, and the sample struct of every variant
// kernel (variant_device.h wraps the arithmetic as the complex tap algebra).  Contract: include/multirate_hip.h, "Complex taps".  R = the promoted real scalar; every multiply,
// add and subtract below is rounded separately in R: the including translation units are compiled with -ffp-contract=off.
#pragma once

#include "mrhip_internal.h"

#pragma clang fp contract(off)

namespace mrhip {

template <typename R> struct alignas(2 * sizeof(R)) CPair { R re, im; };
template <typename TX, int NCX> struct alignas(sizeof(TX) * NCX) CSample { TX c[NCX]; };

// the ONE set of arithmetic statements every complex-tap kernel executes
template <typename TX, typename R, int NCX>
__device__ __forceinline__ CPair<R> ctap_product(const CPair<R> h, const CSample<TX, NCX> v)
{
    CPair<R> p;
    if constexpr (NCX == 1) {
        const R x = static_cast<R>(v.c[0]);
        p.re = h.re * x;
        p.im = h.im * x;
    } else {
        const R xr = static_cast<R>(v.c[0]), xi = static_cast<R>(v.c[1]);
        const R rr = h.re * xr;
        const R ii = h.im * xi;
        p.re = rr - ii;
        const R ri = h.re * xi;
        const R ir = h.im * xr;
        p.im = ri + ir;
    }
    return p;
}
template <typename R>
__device__ __forceinline__ CPair<R> ctap_zero_start(const CPair<R> p)      // support.jl:46
{
    CPair<R> a;
    a.re = static_cast<R>(0) + p.re;
    a.im = static_cast<R>(0) + p.im;
    return a;
}
template <typename R>
__device__ __forceinline__ CPair<R> ctap_add(const CPair<R> acc, const CPair<R> p)
{
    CPair<R> a;
    a.re = acc.re + p.re;
    a.im = acc.im + p.im;
    return a;
}
// FIRArbitrary: buffer[k] = yLower + yUpper * α with α::Float64 (src/Filters.jl:724-730): both sides promote to
// Complex{Float64}, the store rounds to Complex{R}.  Per component: one Float64 product, one Float64 sum, one rounding to R.
template <typename R>
__device__ __forceinline__ CPair<R> ctap_arb_combine(const CPair<R> lo, const CPair<R> up, const double alpha)
{
    CPair<R> y;
    const double pr = static_cast<double>(up.re) * alpha;
    const double sr = static_cast<double>(lo.re) + pr;
    y.re = static_cast<R>(sr);
    const double pi = static_cast<double>(up.im) * alpha;
    const double si = static_cast<double>(lo.im) + pi;
    y.im = static_cast<R>(si);
    return y;
}

}  // namespace mrhip
