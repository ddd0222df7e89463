// kernels_bank_arb.hip -- FIRArbitrary (src/Filters.jl:91-117, 663-742) with PER-CHANNEL taps.
//
// In the reference N channels are N FIRFilter(h_c, rate, N𝜙) objects and every h_c may differ (per-antenna equalisers folded into the
// prototype of a clock-trim resampler, per-channel matched pulse shapes, per-sensor calibration filters).  The phase schedule
// (update(), :663-673; arb_schedule.hip evaluates it) does not depend on the taps, so mrhip_create_arbitrary_bank builds ONE filter
// whose channels share rate, N𝜙, state and call length -- everything but the two filter banks: channel c reads bank c of a.taps (pfb)
// and of a.dtaps (dpfb), both [nch][Nphi][T] in R.  These kernels are the only ones such a filter ever reaches (api.hip: launch_range
// branches on TypeKey::bank first).  Per output k the schedule supplies the input index n_k and the accumulator acc_k;
// 𝜙Idx = floor(acc), α = acc - 𝜙Idx:
//
//     yLower_c = sum_i pfb_c[i, 𝜙Idx] * ext_c[n_k - T + i],   yUpper_c = sum_i dpfb_c[i, 𝜙Idx] * ext_c[n_k - T + i],   ext = [history ; x]
//     y_c,k    = yLower_c + yUpper_c * α
//
// Arithmetic (include/multirate_hip.h, "Per-channel taps for FIRArbitrary"): that of arb_generic_kernel (kernels_generic.hip) on bank
// c -- both dots over one window, oldest sample first, the first product initialises the accumulator, no start-from-zero seam
// (FIRArbitrary's seam method is the Matrix one, support.jl:16-31); STRICT: every multiply and add rounded separately in R, FUSED: one
// fma per tap; the combine in Float64, product and sum each rounded once, then rounded to R -- so channel c is bit for bit
// mrhip_create_arbitrary(h_c, ..., nch = 1) fed x_c.  This file is compiled with -ffp-contract=off; FUSED calls fma explicitly (RealTaps,
// variant_device.h: mac of pipe_stage.h).
// Shared with the other variant units: variant_device.h (bodies, staging, tile hand-out, launch shapes); the tiled plan: host_logic.cpp.
//
// Both kernels take the count from the call record when a.dyn is set (the synchronous path of a FIRArbitrary call is device-planned
// too) and the ShiftFold epilogue (shiftin! by the workgroup that leaves last), exactly as arb_generic_kernel does.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// arb_variant_generic_body with real taps, taps + ch*Nphi*T and dtaps + ch*Nphi*T
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void arb_bank_generic_kernel(ArbArgs a)
{
    arb_variant_generic_body<RealTaps<TX, R, NCX, FUSED>, true>(a, static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x);
}

// Persistent workgroups in the channel-major tile order (tile_run, variant_device.h), the rest arb_ctaps_tiled_kernel's.  A tile is
// (channel, run of tile_out = 256 outputs); the workgroup holds one channel's pfb and dpfb in LDS (column pitch T + 1: lanes of
// different phases read different LDS banks) and reloads them only when its run crosses into the next channel.  The tile's run of
// samples is staged through LDS (tile_span).  The count and the tiling follow the call record when a.dyn is set (tiles_take_dyn with
// nch groups), so every workgroup's run is computed from the device-side count.  No workgroup communicates with or waits for another.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void arb_bank_tiled_kernel(ArbArgs a, ArbTileArgs ta)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_arb_smem[];
    R *const lpfb = reinterpret_cast<R *>(bank_arb_smem);
    R *const ldpfb = lpfb + ta.bank_elems;
    Sample *const lx = reinterpret_cast<Sample *>(bank_arb_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    long long ngroups;                                              // (== nch: a tile covers one channel)
    tiles_take_dyn(a.n_out, ta, ngroups, a.dyn);                    // (a device-planned call: the count from the call record)
    const TileRun run = tile_run(ta.total_tiles);
    const int bank_elems = a.Nphi * T;
    int ch_in_lds = -1;

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile(tile, ta, a.n_out);
        const int ch = t.ch;
        const TileSpan w = tile_span(a.n_idx, t.k0, t.klast, T, ta.max_span);
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;

        __syncthreads();   // the previous tile's reads of banks and window are done
        if (ch != ch_in_lds) {   // (uniform over the workgroup) channel ch's banks -> LDS: element (phi, i) at phi*TP + i
            const R *__restrict__ g0 = static_cast<const R *>(a.taps) + static_cast<long long>(ch) * bank_elems;
            const R *__restrict__ g1 = static_cast<const R *>(a.dtaps) + static_cast<long long>(ch) * bank_elems;
            for (int e = tid; e < bank_elems; e += kVariantThreads) {
                const int phi = e / T, i = e - phi * T;
                lpfb[phi * TP + i] = g0[e];
                ldpfb[phi * TP + i] = g1[e];
            }
            ch_in_lds = ch;
        }
        if (w.staged) stage_window(lx, xc, hc, w.o, static_cast<int>(w.span), a.x_len, a.H, tid);
        __syncthreads();

        R *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        for (long long k = t.k0 + tid; k <= t.klast; k += kVariantThreads) {
            const long long n = a.n_idx[k];
            double alpha;
            const int phi = arb_phase(a.acc[k], &alpha);
            const R *tp = lpfb + phi * TP;
            const R *dp = ldpfb + phi * TP;
            typename A::Sum lo, up;
            if (w.staged) {
                const Sample *wp = lx + (n - w.n_lo);             // oldest sample of this output's window
                const R t0 = tp[0], d0 = dp[0];
                const Sample v0 = wp[0];
                lo = A::first(t0, v0);
                up = A::first(d0, v0);
#pragma unroll 4
                for (int i = 1; i < T; ++i) {
                    const R ti = tp[i], di = dp[i];
                    const Sample v = wp[i];
                    lo = A::step(lo, ti, v);
                    up = A::step(up, di, v);
                }
            } else arb_dots_global<A>(tp, dp, xc, hc + a.H, n - T, T, lo, up);
            A::store(yc, k, A::arb_combine(lo, up, alpha));
        }
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

}  // namespace

hipError_t launch_arb_bank_generic(const TypeKey &tk, bool fused, const ArbArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "arb_bank_generic_kernel", kname, [&]<typename TX, typename R, int NCX>() {
        return fused ? arb_bank_generic_kernel<TX, R, NCX, true> : arb_bank_generic_kernel<TX, R, NCX, false>;
    });
}

bool plan_arb_bank_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_arb_bank_tiled(tk, a, rate, num_cus, MRHIP_ENV_INT("MRHIP_ARB_BANK_TILED", -1), out, lds);
}

hipError_t launch_arb_bank_tiled(const TypeKey &tk, bool fused, const ArbArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                 const char **kname, int num_cus)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    *kname = "arb_bank_tiled_kernel";
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_ARB_BANK_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return launch_persistent(fused ? arb_bank_tiled_kernel<TX, R, NCX, true> : arb_bank_tiled_kernel<TX, R, NCX, false>, a, ta, lds, s,
                                 num_cus, GridOverride::replace, grid_fixed);
    });
}

}  // namespace mrhip
