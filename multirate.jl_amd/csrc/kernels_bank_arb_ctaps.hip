// kernels_bank_arb_ctaps.hip -- FIRArbitrary (src/Filters.jl:91-117, 663-742) with PER-CHANNEL COMPLEX taps.
//
// The reference is generic over the tap type, and in it N channels are N FIRFilter(h_c, rate, N𝜙) objects whose h_c may differ and may
// be complex (a prototype rotated to every channel's own centre frequency in front of a common clock-trim or arbitrary-rate change,
// per-antenna complex equalisers folded into the resampler's prototype, per-channel Hilbert or single-sideband filters).  The phase
// schedule (update(), :663-673; arb_schedule.hip evaluates it) depends neither on the taps nor on their type, so
// mrhip_create_arbitrary_bank_ctaps builds ONE filter whose channels share rate, N𝜙, state and call length -- everything but the two
// filter banks: channel c reads bank c of a.taps (pfb) and of a.dtaps (dpfb), both [nch][Nphi][T] (re, im) pairs of R.  These kernels
// are the only ones such a filter ever reaches (api.hip: launch_range branches on TypeKey::bank && TypeKey::complex_h first).
//
//     yLower_c = sum_i pfb_c[i, 𝜙Idx] * ext_c[n_k - T + i],   yUpper_c = sum_i dpfb_c[i, 𝜙Idx] * ext_c[n_k - T + i],   ext = [history ; x]
//     y_c,k    = yLower_c + yUpper_c * α
//
// Arithmetic (include/multirate_hip.h, "Per-channel complex taps for FIRArbitrary"): that of kernels_ctaps_arb.hip on bank c -- both
// dots over one window, oldest sample first, the first product initialises the accumulator, no start-from-zero seam (FIRArbitrary's
// seam method is the Matrix one, support.jl:16-31), Complex*Real / Complex*Complex written out, every operation rounded separately
// in R (the statements of ctaps_device.h through ComplexTaps<TX, R, NCX>, variant_device.h), the combine per component
// R(double(lo) + double(up) * α) -- so channel c is bit for bit mrhip_create_arbitrary_ctaps(h_c, ..., nch = 1) fed x_c.  There is no
// FUSED form.  This file is compiled with -ffp-contract=off.
// Shared with the other variant units: variant_device.h (bodies, staging, tile hand-out, launch shapes); the tiled plan: host_logic.cpp.
//
// Both kernels take the count from the call record when a.dyn is set and the ShiftFold epilogue (shiftin! by the workgroup that
// leaves last), exactly as arb_bank_generic_kernel and arb_bank_tiled_kernel do.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// arb_variant_generic_body with complex taps, taps + ch*Nphi*T and dtaps + ch*Nphi*T pairs: the universal kernel
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void arb_bank_ctaps_generic_kernel(ArbArgs a)
{
    arb_variant_generic_body<ComplexTaps<TX, R, NCX>, true>(a, static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x);
}

// arb_variant_bank_tiled_body with complex taps: arb_bank_tiled_kernel's shape, one channel's pfb and dpfb in LDS as (re, im) pairs
// at the plan's column pitch (a pair is aligned to its size: a Float32 pair is one 8-byte LDS read, a Float64 pair one 16-byte read)
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void arb_bank_ctaps_tiled_kernel(ArbArgs a, ArbTileArgs ta)
{
    arb_variant_bank_tiled_body<ComplexTaps<TX, R, NCX>>(a, ta);
}

}  // namespace

hipError_t launch_arb_bank_ctaps_generic(const TypeKey &tk, const ArbArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || !tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "arb_bank_ctaps_generic_kernel", kname,
                                  [&]<typename TX, typename R, int NCX>() { return arb_bank_ctaps_generic_kernel<TX, R, NCX>; });
}

bool plan_arb_bank_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_arb_bank_ctaps_tiled(tk, a, rate, num_cus, MRHIP_ENV_INT("MRHIP_ARB_BANK_CTAPS_TILED", -1), out, lds);
}

hipError_t launch_arb_bank_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                       const char **kname, int num_cus)
{
    if (!tk.bank || !tk.complex_h) return hipErrorInvalidValue;
    *kname = "arb_bank_ctaps_tiled_kernel";
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_ARB_BANK_CTAPS_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return launch_persistent(arb_bank_ctaps_tiled_kernel<TX, R, NCX>, a, ta, lds, s, num_cus, GridOverride::replace, grid_fixed);
    });
}

}  // namespace mrhip
