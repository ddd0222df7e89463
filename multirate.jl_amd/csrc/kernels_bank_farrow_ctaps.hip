// kernels_bank_farrow_ctaps.hip -- FIRFarrow (src/Filters.jl:123-147, 764-839) with PER-CHANNEL COMPLEX taps.
//
// The reference is generic over the tap type: N channels are N FIRFilter(h_c::Vector{Complex{T}}, rate, N𝜙, polyorder) objects and every
// h_c may differ (a prototype rotated to each channel's centre frequency, a per-antenna complex equaliser, in front of a common,
// continuously variable rate change).  The phase schedule (update(), :780-792; arb_schedule.hip evaluates it) depends neither on the taps
// nor on their type, so mrhip_create_farrow_bank_ctaps builds ONE filter whose channels share rate, N𝜙, polyorder, state and call length
// -- everything but the polynomial bank: channel c reads bank c of a.pnfb, [nch][T][polyorder+1] (re, im) pairs of Float64, ascending
// powers, values representable in the tap type.  This kernel is the only one such a filter ever reaches (api.hip: launch_range tests
// TypeKey::bank && TypeKey::complex_h first).  Per output k the schedule supplies the input index n_k and the Float64 phase 𝜙_k:
//
//     taps_c[i] = Complex{T}(polyval(pnfb_c[i], 𝜙_k))           i = 1 .. tapsPer𝜙
//     y_c,k     = sum_i taps_c[i] * ext_c[n_k - T + i]           ext = [history ; x]
//
// Arithmetic (include/multirate_hip.h, "Per-channel complex taps for FIRFarrow"): the statements of farrow_ctap
// (kernels_ctaps_farrow.hip) on bank c -- Horner in Float64 from the highest power PER COMPONENT (t = 𝜙*v; v = coef + t, the product and
// the sum each rounded once, never fused), one rounding to the tap's real scalar, widened exactly to R; the dot is the ComplexTaps
// algebra (variant_device.h, ctaps_device.h): oldest sample first, the first product initialises the sum, Complex*Real / Complex*Complex
// written out, every operation rounded separately in R; outputs on the seam (n < seam_below) start from +0 per component
// (support.jl:46).  STRICT only: there is no FUSED form.  So channel c is bit for bit mrhip_create_farrow_ctaps(h_c, ..., nch = 1) fed
// x_c.  This file is compiled with -ffp-contract=off.
//
// One kernel, the body farrow_variant_bank_generic_body<ComplexTaps> of variant_device.h: one lane per output, blockIdx.y strides the
// channels, no dynamic LDS; a tap belongs to one (channel, output) and feeds one product, so it is evaluated in the inner loop from
// wave-uniform coefficients read through the constant address space (scalar loads; at polyorder 4 the ten Float64 of a tap arrive as
// one 16-dword and one 4-dword load and reach the Float64 adds as scalar operands: DESIGN.md 5.16).  The count comes from the call
// record when a.dyn is set; the ShiftFold epilogue (shiftin! by the workgroup that leaves last) has no early return in front of it.
// No tiled kernel, on purpose: staging samples in LDS won nowhere behind ONE Float64 Horner chain per sample read (DESIGN.md 9 item
// 13), and this kernel runs two.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void farrow_bank_ctaps_generic_kernel(FarrowArgs a)
{
    farrow_variant_bank_generic_body<ComplexTaps<TX, R, NCX>>(a, static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x);
}

}  // namespace

hipError_t launch_farrow_bank_ctaps_generic(const TypeKey &tk, const FarrowArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || !tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "farrow_bank_ctaps_generic_kernel", kname,
                                  [&]<typename TX, typename R, int NCX>() { return farrow_bank_ctaps_generic_kernel<TX, R, NCX>; });
}

}  // namespace mrhip
