// kernels_bank.hip -- the rational family (FIRStandard / FIRDecimator / FIRInterpolator / FIRRational) with PER-CHANNEL taps.
//
// In the reference N channels are N FIRFilter(h_c, ratio) objects and every h_c may differ (per-antenna equalisers, matched-filter
// banks, per-receiver calibration filters in front of a common resampler).  mrhip_create_rational_bank builds ONE filter whose
// channels share ratio, state and call length -- everything but the taps: channel c reads bank c of a.taps, [nch][Nphi][T] in R.
// These kernels are the only ones such a filter ever reaches (api.hip: launch_poly / launch_poly_dyn branch on TypeKey::bank first).
//
//     y_c,k = sum_{i=0}^{T-1} pfb_c[i, phi_k] * ext_c[n_k - T + i],   u = u0 + k*M, phi_k = u mod L, n_k = d0 + u div L
//
// Arithmetic (include/multirate_hip.h, "per-channel taps"): that of poly_generic_kernel / poly_tiled_kernel on bank c -- oldest
// sample first, the first product initialises the accumulator, the start-from-zero seam of support.jl:46, STRICT: every multiply
// and add rounded separately in R, FUSED: one fma per tap -- so channel c is bit for bit mrhip_create_rational(h_c, ..., nch = 1)
// fed x_c.  This file is compiled with -ffp-contract=off; FUSED calls fma explicitly (RealTaps, variant_device.h: mac of pipe_stage.h).
// Shared with the other variant units: variant_device.h (bodies, staging, tile hand-out, launch shapes); the tiled plan: host_logic.cpp.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// poly_variant_generic_body with real taps, taps + ch * L * T
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void poly_bank_generic_kernel(PolyArgs a)
{
    poly_variant_generic_body<RealTaps<TX, R, NCX, FUSED>, true>(a);
}

// poly_variant_bank_tiled_body with real taps
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void poly_bank_tiled_kernel(PolyArgs a, ArbTileArgs ta)
{
    poly_variant_bank_tiled_body<RealTaps<TX, R, NCX, FUSED>>(a, ta);
}

}  // namespace

hipError_t launch_poly_bank_generic(const TypeKey &tk, bool fused, const PolyArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "poly_bank_generic_kernel", kname, [&]<typename TX, typename R, int NCX>() {
        return fused ? poly_bank_generic_kernel<TX, R, NCX, true> : poly_bank_generic_kernel<TX, R, NCX, false>;
    });
}

bool plan_bank_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_bank_tiled(tk, a, num_cus, MRHIP_ENV_INT("MRHIP_BANK_TILED", -1), out, lds);
}

hipError_t launch_poly_bank_tiled(const TypeKey &tk, bool fused, const PolyArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                  const char **kname, int num_cus)
{
    if (!tk.bank || tk.complex_h || a.dyn) return hipErrorInvalidValue;
    *kname = "poly_bank_tiled_kernel";
    const int grid_cap = MRHIP_ENV_INT("MRHIP_BANK_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return launch_persistent(fused ? poly_bank_tiled_kernel<TX, R, NCX, true> : poly_bank_tiled_kernel<TX, R, NCX, false>, a, ta, lds, s,
                                 num_cus, GridOverride::cap, grid_cap);
    });
}

}  // namespace mrhip
