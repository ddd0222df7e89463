// kernels_bank_ctaps.hip -- the rational family (FIRStandard / FIRDecimator / FIRInterpolator / FIRRational) with PER-CHANNEL COMPLEX
// taps: the conjunction of kernels_bank.hip (one bank per channel) and kernels_ctaps.hip (complex taps).
//
// In the reference N channels are N FIRFilter(h_c::Vector{Complex}, ratio) objects: one low-pass prototype rotated to every channel's
// own centre frequency in front of a common resampler, per-channel Hilbert filters, per-antenna complex equalisers.
// mrhip_create_rational_bank_ctaps builds ONE filter whose channels share ratio, state and call length -- everything but the taps:
// channel c reads bank c of a.taps, [nch][Nphi][T] (re, im) pairs of R.  These kernels are the only ones such a filter ever reaches
// (api.hip: launch_poly / launch_poly_dyn branch on TypeKey::bank && TypeKey::complex_h first).
//
//     y_c,k = sum_{i=0}^{T-1} pfb_c[i, phi_k] * ext_c[n_k - T + i],   u = u0 + k*M, phi_k = u mod L, n_k = d0 + u div L
//
// Arithmetic (include/multirate_hip.h, "Per-channel complex taps"): the statements of ctaps_device.h on bank c -- oldest sample first, the
// first product initialises the accumulator, the start-from-zero seam of support.jl:46 as 0 + p per component, every multiply, add and
// subtract rounded separately in R -- so channel c is bit for bit mrhip_create_rational(h_c complex, ..., nch = 1) fed x_c.  There is no
// FUSED form.  This file is compiled with -ffp-contract=off.
// Shared with the other variant units: variant_device.h (bodies, staging, tile hand-out, launch shapes); the tiled plan: host_logic.cpp.
#include "ctaps_device.h"
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// poly_variant_generic_body with complex taps, the tap pointer offset by ch * L * T pairs
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void poly_bank_ctaps_generic_kernel(PolyArgs a)
{
    poly_variant_generic_body<ComplexTaps<TX, R, NCX>, true>(a);
}

// poly_variant_bank_tiled_body with complex taps: the bank in LDS as (re, im) pairs
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void poly_bank_ctaps_tiled_kernel(PolyArgs a, ArbTileArgs ta)
{
    poly_variant_bank_tiled_body<ComplexTaps<TX, R, NCX>>(a, ta);
}

}  // namespace

hipError_t launch_poly_bank_ctaps_generic(const TypeKey &tk, const PolyArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || !tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "poly_bank_ctaps_generic_kernel", kname,
                                  [&]<typename TX, typename R, int NCX>() { return poly_bank_ctaps_generic_kernel<TX, R, NCX>; });
}

bool plan_bank_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_bank_ctaps_tiled(tk, a, num_cus, MRHIP_ENV_INT("MRHIP_BANK_CTAPS_TILED", -1), out, lds);
}

hipError_t launch_poly_bank_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                        const char **kname, int num_cus)
{
    if (!tk.bank || !tk.complex_h || a.dyn) return hipErrorInvalidValue;
    *kname = "poly_bank_ctaps_tiled_kernel";
    const int grid_cap = MRHIP_ENV_INT("MRHIP_BANK_CTAPS_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return launch_persistent(poly_bank_ctaps_tiled_kernel<TX, R, NCX>, a, ta, lds, s, num_cus, GridOverride::cap, grid_cap);
    });
}

}  // namespace mrhip
