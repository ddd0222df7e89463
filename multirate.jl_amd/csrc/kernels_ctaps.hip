// kernels_ctaps.hip -- the rational family (FIRStandard / FIRDecimator / FIRInterpolator / FIRRational) with COMPLEX taps.
//
// The reference is generic over the tap type: FIRFilter(h::Vector, ratio) (src/Filters.jl:158-180) and the four unsafedot
// methods (src/support.jl:5-55) only multiply and add, and every filt wrapper allocates promote_type(Th, Tx) -- a
// Vector{Complex64} of taps (a rotated low-pass, a Hilbert filter) works there.  With complex taps the two components of a
// sample are no longer two independent real dot products (the assumption behind NC in every other kernel of the library),
// and a real sample has a two-component output: these kernels are the only ones a complex-tap filter ever reaches
// (api.hip: launch_poly branches on TypeKey::complex_h first).
//
//     y_k = sum_{i=0}^{T-1} pfb[i, phi_k] * ext[n_k - T + i],   u = u0 + k*M, phi_k = u mod L, n_k = d0 + u div L
//
// Arithmetic contract (include/multirate_hip.h, "complex taps"): R = the promoted real scalar; the window is visited oldest
// sample first, the first product initialises the accumulator, the start-from-zero seam of support.jl:46 applies as 0 + p
// per component, and every multiply, add and subtract is rounded separately in R:
//     real sample x,  tap (hr, hi):     p = (hr*x, hi*x)                              Julia's Complex*Real
//     complex sample (xr, xi):          p = (hr*xr - hi*xi, hr*xi + hi*xr)            Julia's Complex*Complex
//     acc = acc + p, component-wise
// There is no FUSED form.  This file is compiled with -ffp-contract=off.
//
// The taps are R-typed (re, im) pairs on the device, [Nphi][T] pairs, oldest-sample tap first (a narrower tap type is
// widened exactly at upload); the history is Tx (real for real samples: shiftin_kernel is reused as is); the output is
// (re, im) pairs of R.
// Shared with the other variant units: variant_device.h (bodies, staging, tile hand-out, launch shapes); the tiled plan: host_logic.cpp.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// poly_variant_generic_body with complex taps and the one shared bank
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void poly_ctaps_generic_kernel(PolyArgs a)
{
    poly_variant_generic_body<ComplexTaps<TX, R, NCX>, false>(a);
}

// Persistent workgroups, as poly_tiled_kernel: the complex bank sits in LDS once per workgroup as (re, im) pairs with a column pitch of
// T + 1 pairs (lanes of different phases read different banks; a pair of Float32 is one 8-byte LDS read), the [history ; x] run of a tile
// is staged for CPL channels, one lane owns one output index of CPL channels.  Host-planned calls only (the tiling follows the count).
template <typename TX, typename R, int NCX, int CPL>
__global__ __launch_bounds__(kVariantThreads) void poly_ctaps_tiled_kernel(PolyArgs a, ArbTileArgs ta)
{
    using A = ComplexTaps<TX, R, NCX>;
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctaps_smem[];
    CPair<R> *const lpfb = reinterpret_cast<CPair<R> *>(ctaps_smem);
    Sample *const lx = reinterpret_cast<Sample *>(ctaps_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    if (a.rec && tid == 0 && blockIdx.x == 0) file_end_state(a);
    bank_to_lds(lpfb, static_cast<const CPair<R> *>(a.taps), a.L * T, T, TP, tid);       // the tap bank -> LDS once per workgroup

    for (long long tile = blockIdx.x; tile < ta.total_tiles; tile += gridDim.x) {
        const BankTile t = bank_tile(tile, ta, a.n_out);                                // (t.ch: the channel group)
        const int ch0 = t.ch * CPL;
        const int nchl = a.nch - ch0 < CPL ? a.nch - ch0 : CPL;
        const long long k0 = t.k0, klast = t.klast;
        int phi_unused;
        const long long n_lo = newest_of(a, k0, &phi_unused), n_hi = newest_of(a, klast, &phi_unused);
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (may be < 0)
        const int span = static_cast<int>(n_hi - n_lo) + T;                             // <= ta.max_span (plan_variant_poly_tiled: span_of)

        __syncthreads();   // previous tile's reads are done (and, first time, the tap bank is written)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            if (cc < nchl)
                stage_window(lx + static_cast<size_t>(cc) * ta.max_span, static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride,
                             static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H, o, span, a.x_len, a.H, tid);
        }
        __syncthreads();

        for (long long k = k0 + tid; k <= klast; k += kVariantThreads) {
            int phi;
            const long long n = newest_of(a, k, &phi);
            const CPair<R> *tp = lpfb + phi * TP;
            const Sample *wp = lx + (n - n_lo);             // oldest sample of this output's window (channel 0 of the group)
            CPair<R> acc[CPL];
            {
                const CPair<R> t = tp[0];
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) acc[cc] = A::first(t, wp[static_cast<size_t>(cc) * ta.max_span]);
            }
            if (n < a.zero_start_below) {
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) acc[cc] = A::zero_start(acc[cc]);
            }
#pragma unroll 4
            for (int i = 1; i < T; ++i) {
                const CPair<R> t = tp[i];
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) acc[cc] = A::step(acc[cc], t, wp[static_cast<size_t>(cc) * ta.max_span + i]);
            }
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                if (cc < nchl) A::store(A::channel_out(a.y, ch0 + cc, a.y_stride), k, acc[cc]);
            }
        }
    }
}

}  // namespace

hipError_t launch_poly_ctaps_generic(const TypeKey &tk, const PolyArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "poly_ctaps_generic_kernel", kname,
                                  [&]<typename TX, typename R, int NCX>() { return poly_ctaps_generic_kernel<TX, R, NCX>; });
}

bool plan_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_ctaps_tiled(tk, a, num_cus, MRHIP_ENV_INT("MRHIP_CTAPS_TILED", -1), out, lds);
}

hipError_t launch_poly_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                   const char **kname, int num_cus)
{
    if (!tk.complex_h || a.dyn) return hipErrorInvalidValue;
    *kname = "poly_ctaps_tiled_kernel";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        switch (ta.cpl) {
        case 4: return launch_persistent(poly_ctaps_tiled_kernel<TX, R, NCX, 4>, a, ta, lds, s, num_cus);
        case 2: return launch_persistent(poly_ctaps_tiled_kernel<TX, R, NCX, 2>, a, ta, lds, s, num_cus);
        default: return launch_persistent(poly_ctaps_tiled_kernel<TX, R, NCX, 1>, a, ta, lds, s, num_cus);
        }
    });
}

}  // namespace mrhip
