// kernels_ctaps_arb.hip -- FIRArbitrary (src/Filters.jl:91-117, 663-742) with COMPLEX taps.
//
// The reference is generic over the tap type: FIRArbitrary(h::Vector, rate, N𝜙) takes dh = [diff(h), 0] in the tap type and
// filt! only multiplies and adds.  Per output k the phase schedule (update(), :663-673; arb_schedule.hip evaluates it, the tap
// type plays no part in it) supplies the input index n_k and the accumulator acc_k; 𝜙Idx = floor(acc), α = acc - 𝜙Idx:
//
//     yLower = sum_i pfb[i, 𝜙Idx] * ext[n_k - T + i],   yUpper = sum_i dpfb[i, 𝜙Idx] * ext[n_k - T + i],   ext = [history ; x]
//     y_k    = yLower + yUpper * α
//
// Arithmetic contract (include/multirate_hip.h, "Complex taps"): both dots exactly as the rational family's -- oldest sample
// first, the first product initialises the accumulator (FIRArbitrary's seam method is the Matrix one, support.jl:16-31: no
// start from zero), Complex*Real / Complex*Complex written out, every operation rounded separately in R (ctaps_device.h) --
// and the combine per component in Float64, rounded once to R (α is a Float64 in the reference).  There is no FUSED form.
// This file is compiled with -ffp-contract=off.
//
// Both banks are R-typed (re, im) pairs on the device, [Nphi][T] pairs, oldest-sample tap first; the history is Tx (real for
// real samples); the output is (re, im) pairs of R.  Both kernels take the ShiftFold epilogue (shiftin! by the workgroup that
// leaves last) exactly as arb_generic_kernel does.
// Shared with the other variant units: variant_device.h (bodies, staging, tile hand-out, launch shapes); the tiled plan: host_logic.cpp.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// arb_variant_generic_body with complex taps and the one shared pair of banks
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void arb_ctaps_generic_kernel(ArbArgs a)
{
    arb_variant_generic_body<ComplexTaps<TX, R, NCX>, false>(a, static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x);
}

// Persistent workgroups, as poly_ctaps_tiled_kernel: BOTH complex banks sit in LDS once per workgroup as (re, im)
// pairs with a column pitch of T + 1 pairs (lanes of different phases read different banks; a pair of Float32 is one 8-byte
// LDS read).  Per tile of 256 consecutive outputs and group of CPL channels the tile's run of samples is staged (tile_span); one
// lane owns one output index of CPL channels, holds lo and up for each and reads one pair of each bank per tap for all of them.
// Device-planned calls (a.dyn): the count comes from the call record and the tiling follows it.
template <typename TX, typename R, int NCX, int CPL>
__global__ __launch_bounds__(kVariantThreads) void arb_ctaps_tiled_kernel(ArbArgs a, ArbTileArgs ta)
{
    using A = ComplexTaps<TX, R, NCX>;
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctaps_arb_smem[];
    CPair<R> *const lpfb = reinterpret_cast<CPair<R> *>(ctaps_arb_smem);
    CPair<R> *const ldpfb = lpfb + ta.bank_elems;
    Sample *const lx = reinterpret_cast<Sample *>(ctaps_arb_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    {   // both tap banks -> LDS once per workgroup: pair (phi, i) at phi*TP + i
        const CPair<R> *__restrict__ g0 = static_cast<const CPair<R> *>(a.taps);
        const CPair<R> *__restrict__ g1 = static_cast<const CPair<R> *>(a.dtaps);
        const int total = a.Nphi * T;
        for (int e = tid; e < total; e += kVariantThreads) {
            const int phi = e / T, i = e - phi * T;
            lpfb[phi * TP + i] = g0[e];
            ldpfb[phi * TP + i] = g1[e];
        }
    }
    long long ngroups;
    tiles_take_dyn(a.n_out, ta, ngroups, a.dyn);                    // (a device-planned call: the count from the call record)

    for (long long tile = blockIdx.x; tile < ta.total_tiles; tile += gridDim.x) {
        // time-major: the workgroups that run together work on the same stretch of the (shared) schedule for different channel groups
        const long long tau = tile / ngroups;
        const int cg = static_cast<int>(tile - tau * ngroups);
        const int ch0 = cg * CPL;
        const int nchl = a.nch - ch0 < CPL ? a.nch - ch0 : CPL;
        const long long k0 = tau * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        const TileSpan w = tile_span(a.n_idx, k0, klast, T, ta.max_span);

        __syncthreads();   // previous tile's reads are done (and, first time, the tap banks are written)
        if (w.staged) {
#pragma unroll 1
            for (int cc = 0; cc < nchl; ++cc)
                stage_window(lx + static_cast<size_t>(cc) * ta.max_span, static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride,
                             static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H, w.o, static_cast<int>(w.span), a.x_len, a.H, tid);
        }
        __syncthreads();

        for (long long k = k0 + tid; k <= klast; k += kVariantThreads) {
            const long long n = a.n_idx[k];
            double alpha;
            const int phi = arb_phase(a.acc[k], &alpha);
            const CPair<R> *tp = lpfb + phi * TP;
            const CPair<R> *dp = ldpfb + phi * TP;
            CPair<R> lo[CPL], up[CPL];
            if (w.staged) {
                const Sample *wp = lx + (n - w.n_lo);         // oldest sample of this output's window (channel 0 of the group)
                {
                    const CPair<R> t = tp[0], d = dp[0];
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) {
                        const Sample v = wp[static_cast<size_t>(cc) * ta.max_span];
                        lo[cc] = A::first(t, v);
                        up[cc] = A::first(d, v);
                    }
                }
#pragma unroll 2
                for (int i = 1; i < T; ++i) {
                    const CPair<R> t = tp[i], d = dp[i];
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) {
                        const Sample v = wp[static_cast<size_t>(cc) * ta.max_span + i];
                        lo[cc] = A::step(lo[cc], t, v);
                        up[cc] = A::step(up[cc], d, v);
                    }
                }
            } else {
                // the windows from global memory, a channel at a time (the taps are read from LDS once per channel here)
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    if (cc < nchl)
                        arb_dots_global<A>(tp, dp, static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride,
                                           static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H + a.H, n - T, T, lo[cc], up[cc]);
                }
            }
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                if (cc < nchl) A::store(A::channel_out(a.y, ch0 + cc, a.y_stride), k, A::arb_combine(lo[cc], up[cc], alpha));
            }
        }
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

}  // namespace

hipError_t launch_arb_ctaps_generic(const TypeKey &tk, const ArbArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "arb_ctaps_generic_kernel", kname,
                                  [&]<typename TX, typename R, int NCX>() { return arb_ctaps_generic_kernel<TX, R, NCX>; });
}

// (MRHIP_CTAPS_ARB_TILED_MIN: the threshold of the default rule, outputs x channels)
bool plan_ctaps_arb_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_ctaps_arb_tiled(tk, a, rate, num_cus, MRHIP_ENV_INT("MRHIP_CTAPS_TILED", -1),
                                MRHIP_ENV_INT("MRHIP_CTAPS_ARB_TILED_MIN", kCtapsArbTiledMinDefault), out, lds);
}

hipError_t launch_arb_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                  const char **kname, int num_cus)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    *kname = "arb_ctaps_tiled_kernel";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return ta.cpl == 2 ? launch_persistent(arb_ctaps_tiled_kernel<TX, R, NCX, 2>, a, ta, lds, s, num_cus)
                           : launch_persistent(arb_ctaps_tiled_kernel<TX, R, NCX, 1>, a, ta, lds, s, num_cus);
    });
}

}  // namespace mrhip
