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
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "ctaps_device.h"
#include "mrhip_internal.h"
#include "pair_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kCtapsArbThreads = 256;
// outputs x channels from which plan_ctaps_arb_tiled takes a call by default; negative: only when MRHIP_CTAPS_TILED=1 asks for it
constexpr int kCtapsArbTiledMinDefault = -1;

// One thread per output, any (Nphi, T, hLen, rate): arb_generic_kernel with complex taps.  Serves small calls and the calls
// whose count only the device knows (a.dyn: asynchronous, device-planned and graph-captured calls).
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kCtapsArbThreads) void arb_ctaps_generic_kernel(ArbArgs a)
{
    using Sample = CSample<TX, NCX>;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a.dyn) a.n_out = a.dyn->n_out;              // a device-planned call: the count the schedule's FINISH kernel left
    if (k < a.n_out) {                               // (no early return: every thread takes part in the history epilogue below)
        const long long n = a.n_idx[k];
        const double pacc = a.acc[k];
        const double phif = __builtin_floor(pacc);
        const double alpha = pacc - phif;           // src/Filters.jl:671-672
        const int phi = static_cast<int>(phif) - 1; // 0-based column
        const CPair<R> *__restrict__ tp = static_cast<const CPair<R> *>(a.taps) + static_cast<long long>(phi) * a.T;
        const CPair<R> *__restrict__ dp = static_cast<const CPair<R> *>(a.dtaps) + static_cast<long long>(phi) * a.T;
        const long long base = n - a.T;             // 0-based index of the oldest sample (>= -H: n >= 1)
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            CPair<R> *__restrict__ yc = static_cast<CPair<R> *>(a.y) + static_cast<long long>(ch) * a.y_stride;
            auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
            Sample v = sample(base);
            CPair<R> lo = ctap_product<TX, R, NCX>(tp[0], v);
            CPair<R> up = ctap_product<TX, R, NCX>(dp[0], v);
            for (int i = 1; i < a.T; ++i) {
                v = sample(base + i);
                lo = ctap_add<R>(lo, ctap_product<TX, R, NCX>(tp[i], v));
                up = ctap_add<R>(up, ctap_product<TX, R, NCX>(dp[i], v));
            }
            yc[k] = ctap_arb_combine<R>(lo, up, alpha);
        }
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// Persistent workgroups, modelled on poly_ctaps_tiled_kernel: BOTH complex banks sit in LDS once per workgroup as (re, im)
// pairs with a column pitch of T + 1 pairs (lanes of different phases read different banks; a pair of Float32 is one 8-byte
// LDS read).  Per tile of 256 consecutive outputs and group of CPL channels the contiguous [history ; x] run between the
// tile's first and last n_idx (the schedule is non-decreasing in k: x[n_idx[k0] - T ... n_idx[klast])) is staged; one lane owns
// one output index of CPL channels, holds lo and up for each and reads one pair of each bank per tap for all of them.
// The span of a tile is read from the schedule HERE, so the kernel serves device-planned calls too (a.dyn: the count comes
// from the call record and the tiling follows it); a tile whose run is longer than the planned span (ta.max_span: the plan
// goes by the rate and by what LDS holds -- a heavily decimating rate, rate << 1) reads its windows from global memory.
template <typename TX, typename R, int NCX, int CPL>
__global__ __launch_bounds__(kCtapsArbThreads) void arb_ctaps_tiled_kernel(ArbArgs a, ArbTileArgs ta)
{
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
        for (int e = tid; e < total; e += kCtapsArbThreads) {
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
        const long long n_lo = a.n_idx[k0], n_hi = a.n_idx[klast];
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (>= -H)
        const long long span = n_hi - n_lo + T;
        const bool staged = span <= ta.max_span;                                        // (uniform over the workgroup)

        __syncthreads();   // previous tile's reads are done (and, first time, the tap banks are written)
        if (staged) {
#pragma unroll 1
            for (int cc = 0; cc < nchl; ++cc) {
                {
                    const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride;
                    const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H;
                    Sample *const lxc = lx + static_cast<size_t>(cc) * ta.max_span;
                    for (int s = tid; s < static_cast<int>(span); s += kCtapsArbThreads) {
                        const long long gi = o + s;
                        Sample v;
#pragma unroll
                        for (int c = 0; c < NCX; ++c) v.c[c] = static_cast<TX>(0);
                        if (gi >= 0) { if (gi < a.x_len) v = xc[gi]; }
                        else if (gi >= -static_cast<long long>(a.H)) v = hc[a.H + gi];
                        lxc[s] = v;
                    }
                }
            }
        }
        __syncthreads();

        for (long long k = k0 + tid; k <= klast; k += kCtapsArbThreads) {
            const long long n = a.n_idx[k];
            const double pacc = a.acc[k];
            const double phif = __builtin_floor(pacc);
            const double alpha = pacc - phif;
            const int phi = static_cast<int>(phif) - 1;
            const CPair<R> *tp = lpfb + phi * TP;
            const CPair<R> *dp = ldpfb + phi * TP;
            CPair<R> lo[CPL], up[CPL];
            if (staged) {
                const Sample *wp = lx + (n - n_lo);         // oldest sample of this output's window (channel 0 of the group)
                {
                    const CPair<R> t = tp[0], d = dp[0];
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) {
                        const Sample v = wp[static_cast<size_t>(cc) * ta.max_span];
                        lo[cc] = ctap_product<TX, R, NCX>(t, v);
                        up[cc] = ctap_product<TX, R, NCX>(d, v);
                    }
                }
#pragma unroll 2
                for (int i = 1; i < T; ++i) {
                    const CPair<R> t = tp[i], d = dp[i];
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) {
                        const Sample v = wp[static_cast<size_t>(cc) * ta.max_span + i];
                        lo[cc] = ctap_add<R>(lo[cc], ctap_product<TX, R, NCX>(t, v));
                        up[cc] = ctap_add<R>(up[cc], ctap_product<TX, R, NCX>(d, v));
                    }
                }
            } else {
                // the windows from global memory, a channel at a time (the taps are read from LDS once per channel here)
                const long long base = n - T;
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    if (cc < nchl) {
                        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride;
                        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H + a.H;
                        Sample v = base >= 0 ? xc[base] : hc[base];
                        CPair<R> l = ctap_product<TX, R, NCX>(tp[0], v);
                        CPair<R> u = ctap_product<TX, R, NCX>(dp[0], v);
                        for (int i = 1; i < T; ++i) {
                            const long long xi = base + i;
                            v = xi >= 0 ? xc[xi] : hc[xi];
                            l = ctap_add<R>(l, ctap_product<TX, R, NCX>(tp[i], v));
                            u = ctap_add<R>(u, ctap_product<TX, R, NCX>(dp[i], v));
                        }
                        lo[cc] = l;
                        up[cc] = u;
                    }
                }
            }
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                if (cc < nchl) {
                    CPair<R> *__restrict__ yc = static_cast<CPair<R> *>(a.y) + static_cast<long long>(ch0 + cc) * a.y_stride;
                    yc[k] = ctap_arb_combine<R>(lo[cc], up[cc], alpha);
                }
            }
        }
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

}  // namespace

hipError_t launch_arb_ctaps_generic(const TypeKey &tk, const ArbArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    const long long bx = a.n_out > 0 ? (a.n_out + kCtapsArbThreads - 1) / kCtapsArbThreads : 1;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "arb_ctaps_generic_kernel";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(arb_ctaps_generic_kernel<TX, R, NCX>, grid, dim3(kCtapsArbThreads), 0, s, a);
        return hipGetLastError();
    });
}

// Eligibility of arb_ctaps_tiled_kernel (beside plan_ctaps_tiled, kernels_ctaps.hip): both banks of pairs plus a tile of samples
// fit LDS, and the call gives every CU a tile.  A tile is 256 outputs (a lane each) of CPL channels; its planned span follows
// from the rate -- consecutive outputs are 1/rate samples apart -- and is cut to the 40 KiB the samples may take (two workgroups
// a CU beside banks of up to 40 KiB): tiles with a longer run read global memory, so a rate that makes EVERY full tile such a
// tile is left to the universal kernel unless the kernel is forced.
// MRHIP_CTAPS_TILED=0: never; =1: whenever LDS allows (tests, measurements); unset: the measured rule at the end.
bool plan_ctaps_arb_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, ArbTileArgs *out, size_t *lds)
{
    const int mode = MRHIP_ENV_INT("MRHIP_CTAPS_TILED", -1);
    if (mode == 0 || !tk.complex_h || a.n_out < 1 || a.T < 1 || !(rate > 0.0)) return false;
    const size_t ps = (tk.r_f64 ? 8 : 4) * 2;                                           // one tap pair
    const size_t sb = (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1);                      // one sample
    const int TP = a.T + 1;
    const size_t bank_pairs = static_cast<size_t>(a.Nphi) * TP;
    const size_t banks_bytes = (2 * bank_pairs * ps + 15) / 16 * 16;
    if (banks_bytes > 96 * 1024) return false;
    constexpr size_t kSampleBytes = 40 * 1024;
    const long long tile_out = kCtapsArbThreads;
    // samples the run of a tile can hold: n advances by at most ceil(1/rate) + 1 per output (update(), Filters.jl:663-673)
    const double per_tile = std::ceil(static_cast<double>(tile_out - 1) / rate) + static_cast<double>(a.T) + 2.0;
    // (CPL = 1 or 2: with four channels a lane -- lo and up of four complex sums beside both banks' pairs -- the compiler spills
    //  to scratch in every type combination)
    int cpl = a.nch >= 8 ? 2 : 1;
    while (cpl > 1 && per_tile * static_cast<double>(sb * cpl) > static_cast<double>(kSampleBytes)) cpl /= 2;
    long long max_span = static_cast<long long>(kSampleBytes / (sb * cpl));
    const bool cut = per_tile > static_cast<double>(max_span);
    if (!cut) max_span = static_cast<long long>(per_tile);
    if (max_span < a.T + 1) return false;                                               // not even one window
    if (cut && mode != 1) return false;
    const long long groups = (a.nch + cpl - 1) / cpl;
    ArbTileArgs ta{};
    ta.cpl = cpl;
    ta.tap_pitch = TP;
    ta.bank_elems = static_cast<int>(bank_pairs);
    ta.x_offset_bytes = static_cast<int>(banks_bytes);
    ta.max_span = static_cast<int>(max_span);
    ta.tile_out = tile_out;
    ta.tiles_per_channel = (a.n_out + tile_out - 1) / tile_out;
    ta.total_tiles = ta.tiles_per_channel * groups;
    if (mode != 1) {
        // The default rule.  MRHIP_CTAPS_ARB_TILED_MIN: outputs x channels from which the tiled kernel takes the call
        // (profiles/r07/ctaps_arb.txt has the measurements the default comes from); and a tile per CU at least.
        if (ta.total_tiles < static_cast<long long>(num_cus)) return false;
        const long long min_work = MRHIP_ENV_INT("MRHIP_CTAPS_ARB_TILED_MIN", kCtapsArbTiledMinDefault);
        if (min_work < 0 || a.n_out * static_cast<long long>(a.nch) < min_work) return false;
    }
    *out = ta;
    *lds = banks_bytes + static_cast<size_t>(max_span) * sb * cpl;
    return true;
}

hipError_t launch_arb_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                  const char **kname, int num_cus)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    *kname = "arb_ctaps_tiled_kernel";
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto go = [&](auto kfn) -> hipError_t {
            const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kCtapsArbThreads, lds, num_cus, ta.total_tiles);
            if (pg.err != hipSuccess) return pg.err;
            launch_kernel(kfn, dim3(static_cast<unsigned>(pg.grid)), dim3(kCtapsArbThreads), lds, s, a, ta);
            return hipGetLastError();
        };
        return ta.cpl == 2 ? go(arb_ctaps_tiled_kernel<TX, R, NCX, 2>) : go(arb_ctaps_tiled_kernel<TX, R, NCX, 1>);
    });
}

}  // namespace mrhip
