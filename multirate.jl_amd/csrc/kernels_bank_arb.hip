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
// mrhip_create_arbitrary(h_c, ..., nch = 1) fed x_c.  This file is compiled with -ffp-contract=off; FUSED calls fma explicitly.
//
// Both kernels take the count from the call record when a.dyn is set (the synchronous path of a FIRArbitrary call is device-planned
// too) and the ShiftFold epilogue (shiftin! by the workgroup that leaves last), exactly as arb_generic_kernel does.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "mrhip_internal.h"
#include "pair_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kArbBankThreads = 256;

template <typename R, bool FUSED>
__device__ __forceinline__ R mac(R t, R x, R acc)
{
    if constexpr (FUSED) {
        if constexpr (sizeof(R) == 4) return __builtin_fmaf(t, x, acc);
        else return __builtin_fma(t, x, acc);
    } else {
        R p = t * x;
        return acc + p;
    }
}

template <typename TX, int NCX>
struct alignas(sizeof(TX) * NCX) BankSample { TX c[NCX]; };

// yLower + yUpper * α: both sides promote to Float64 (α is a Float64 in the reference), the store rounds to R
template <typename R>
__device__ __forceinline__ R arb_combine(R lo, R up, double alpha)
{
    const double prod = static_cast<double>(up) * alpha;
    const double sum = static_cast<double>(lo) + prod;
    return static_cast<R>(sum);
}

// One thread per output, any (Nphi, T, hLen, rate): arb_generic_kernel with taps + ch*Nphi*T and dtaps + ch*Nphi*T.  Serves every
// path: device-planned calls (a.dyn: the synchronous path, asynchronous, chained and graph-captured calls), host-scheduled calls and
// the pieces of a split call.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kArbBankThreads) void arb_bank_generic_kernel(ArbArgs a)
{
    using Sample = BankSample<TX, NCX>;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a.dyn) a.n_out = a.dyn->n_out;              // a device-planned call: the count the schedule's FINISH kernel left
    if (k < a.n_out) {                               // (no early return: every thread takes part in the history epilogue below)
        const long long n = a.n_idx[k];
        const double pacc = a.acc[k];
        const double phif = __builtin_floor(pacc);
        const double alpha = pacc - phif;           // src/Filters.jl:671-672
        const int phi = static_cast<int>(phif) - 1; // 0-based column
        const long long bank = static_cast<long long>(a.Nphi) * a.T;
        const long long col = static_cast<long long>(phi) * a.T;
        const long long base = n - a.T;             // 0-based index of the oldest sample (>= -H: n >= 1)
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            const R *__restrict__ tp = static_cast<const R *>(a.taps) + static_cast<long long>(ch) * bank + col;
            const R *__restrict__ dp = static_cast<const R *>(a.dtaps) + static_cast<long long>(ch) * bank + col;
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            R *__restrict__ yc = static_cast<R *>(a.y) + static_cast<long long>(ch) * a.y_stride * NCX;
            auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
            R lo[NCX], up[NCX];
            {
                const Sample v = sample(base);
                const R t = tp[0], d = dp[0];
#pragma unroll
                for (int c = 0; c < NCX; ++c) {
                    lo[c] = t * static_cast<R>(v.c[c]);
                    up[c] = d * static_cast<R>(v.c[c]);
                }
            }
            for (int i = 1; i < a.T; ++i) {
                const Sample v = sample(base + i);
                const R t = tp[i], d = dp[i];
#pragma unroll
                for (int c = 0; c < NCX; ++c) {
                    lo[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), lo[c]);
                    up[c] = mac<R, FUSED>(d, static_cast<R>(v.c[c]), up[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < NCX; ++c) yc[k * NCX + c] = arb_combine<R>(lo[c], up[c], alpha);
        }
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// Persistent workgroups: the ownership of tiles is poly_bank_tiled_kernel's, the rest arb_ctaps_tiled_kernel's.  A tile is (channel,
// run of tile_out = 256 outputs); the tiles are ordered channel-major and workgroup b owns ONE contiguous run of that order, so it
// holds one channel's pfb and dpfb in LDS (column pitch T + 1: lanes of different phases read different LDS banks) and reloads them
// only when its run crosses into the next channel.  The contiguous [history ; x] run between the tile's first and last n_idx (the
// schedule is non-decreasing in k: x[n_idx[k0] - T ... n_idx[klast])) is read from the schedule HERE and staged through LDS; a tile
// whose run is longer than the planned span (ta.max_span: the plan goes by the rate and by what LDS holds -- a heavily decimating
// rate) reads its windows from global memory.  The count and the tiling follow the call record when a.dyn is set (tiles_take_dyn with
// nch groups), so every workgroup's run is computed from the device-side count.  No workgroup communicates with or waits for another.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kArbBankThreads) void arb_bank_tiled_kernel(ArbArgs a, ArbTileArgs ta)
{
    using Sample = BankSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_arb_smem[];
    R *const lpfb = reinterpret_cast<R *>(bank_arb_smem);
    R *const ldpfb = lpfb + ta.bank_elems;
    Sample *const lx = reinterpret_cast<Sample *>(bank_arb_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    long long ngroups;                                              // (== nch: a tile covers one channel)
    tiles_take_dyn(a.n_out, ta, ngroups, a.dyn);                    // (a device-planned call: the count from the call record)

    // this workgroup's run of the channel-major tile order: [t_begin, t_end)
    const long long per = ta.total_tiles / gridDim.x, extra = ta.total_tiles - per * gridDim.x;
    const long long b = blockIdx.x;
    const long long t_begin = b * per + (b < extra ? b : extra);
    const long long t_end = t_begin + per + (b < extra ? 1 : 0);
    const int bank_elems = a.Nphi * T;
    int ch_in_lds = -1;

    for (long long tile = t_begin; tile < t_end; ++tile) {
        const int ch = static_cast<int>(tile / ta.tiles_per_channel);
        const long long tau = tile - static_cast<long long>(ch) * ta.tiles_per_channel;
        const long long k0 = tau * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        const long long n_lo = a.n_idx[k0], n_hi = a.n_idx[klast];
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (>= -H)
        const long long span = n_hi - n_lo + T;
        const bool staged = span <= ta.max_span;                                        // (uniform over the workgroup)
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;

        __syncthreads();   // the previous tile's reads of banks and window are done
        if (ch != ch_in_lds) {   // (uniform over the workgroup) channel ch's banks -> LDS: element (phi, i) at phi*TP + i
            const R *__restrict__ g0 = static_cast<const R *>(a.taps) + static_cast<long long>(ch) * bank_elems;
            const R *__restrict__ g1 = static_cast<const R *>(a.dtaps) + static_cast<long long>(ch) * bank_elems;
            for (int e = tid; e < bank_elems; e += kArbBankThreads) {
                const int phi = e / T, i = e - phi * T;
                lpfb[phi * TP + i] = g0[e];
                ldpfb[phi * TP + i] = g1[e];
            }
            ch_in_lds = ch;
        }
        if (staged) {
            for (int s = tid; s < static_cast<int>(span); s += kArbBankThreads) {
                const long long gi = o + s;
                Sample v;
#pragma unroll
                for (int c = 0; c < NCX; ++c) v.c[c] = static_cast<TX>(0);
                if (gi >= 0) { if (gi < a.x_len) v = xc[gi]; }
                else if (gi >= -static_cast<long long>(a.H)) v = hc[a.H + gi];
                lx[s] = v;
            }
        }
        __syncthreads();

        R *__restrict__ yc = static_cast<R *>(a.y) + static_cast<long long>(ch) * a.y_stride * NCX;
        for (long long k = k0 + tid; k <= klast; k += kArbBankThreads) {
            const long long n = a.n_idx[k];
            const double pacc = a.acc[k];
            const double phif = __builtin_floor(pacc);
            const double alpha = pacc - phif;
            const int phi = static_cast<int>(phif) - 1;
            const R *tp = lpfb + phi * TP;
            const R *dp = ldpfb + phi * TP;
            R lo[NCX], up[NCX];
            if (staged) {
                const Sample *wp = lx + (n - n_lo);             // oldest sample of this output's window
                {
                    const R t = tp[0], d = dp[0];
                    const Sample v = wp[0];
#pragma unroll
                    for (int c = 0; c < NCX; ++c) {
                        lo[c] = t * static_cast<R>(v.c[c]);
                        up[c] = d * static_cast<R>(v.c[c]);
                    }
                }
#pragma unroll 4
                for (int i = 1; i < T; ++i) {
                    const R t = tp[i], d = dp[i];
                    const Sample v = wp[i];
#pragma unroll
                    for (int c = 0; c < NCX; ++c) {
                        lo[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), lo[c]);
                        up[c] = mac<R, FUSED>(d, static_cast<R>(v.c[c]), up[c]);
                    }
                }
            } else {
                // the window from global memory (the taps still come from LDS)
                const long long base = n - T;
                const Sample *__restrict__ he = hc + a.H;
                {
                    const R t = tp[0], d = dp[0];
                    const Sample v = base >= 0 ? xc[base] : he[base];
#pragma unroll
                    for (int c = 0; c < NCX; ++c) {
                        lo[c] = t * static_cast<R>(v.c[c]);
                        up[c] = d * static_cast<R>(v.c[c]);
                    }
                }
                for (int i = 1; i < T; ++i) {
                    const long long xi = base + i;
                    const R t = tp[i], d = dp[i];
                    const Sample v = xi >= 0 ? xc[xi] : he[xi];
#pragma unroll
                    for (int c = 0; c < NCX; ++c) {
                        lo[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), lo[c]);
                        up[c] = mac<R, FUSED>(d, static_cast<R>(v.c[c]), up[c]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NCX; ++c) yc[k * NCX + c] = arb_combine<R>(lo[c], up[c], alpha);
        }
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// (Tx scalar, R) combinations that promote_type can produce: (f32,f32) (f32,f64) (f64,f64), real and complex samples
template <typename F>
hipError_t dispatch_arb_bank(const TypeKey &tk, F &&f)
{
    if (!tk.x_f64 && !tk.r_f64) return tk.complex_x ? f.template operator()<float, float, 2>() : f.template operator()<float, float, 1>();
    if (!tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<float, double, 2>() : f.template operator()<float, double, 1>();
    if (tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<double, double, 2>() : f.template operator()<double, double, 1>();
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_arb_bank_generic(const TypeKey &tk, bool fused, const ArbArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    const long long bx = a.n_out > 0 ? (a.n_out + kArbBankThreads - 1) / kArbBankThreads : 1;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "arb_bank_generic_kernel";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_arb_bank(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        if (fused) launch_kernel(arb_bank_generic_kernel<TX, R, NCX, true>, grid, dim3(kArbBankThreads), 0, s, a);
        else launch_kernel(arb_bank_generic_kernel<TX, R, NCX, false>, grid, dim3(kArbBankThreads), 0, s, a);
        return hipGetLastError();
    });
}

// The default rule of plan_arb_bank_tiled (MRHIP_ARB_BANK_TILED unset): the tiled kernel was faster than the universal one by far more
// than the spread of the repeats in every measured call of 5312 tiles or more (1.4 ... 10 times: DESIGN.md 9 item 12,
// profiles/r07/arb_bank.txt) and was not at 664 and 166 tiles (calls bound by their launches).  So: from kArbBankTiledTilesPerCu tiles
// per CU (5120 tiles on 256 CUs; 5312 is the smallest measured call it won); everything smaller stays on the universal kernel.
constexpr long long kArbBankTiledTilesPerCu = 20;
static bool arb_bank_tiled_measured_faster(long long total_tiles, int num_cus)
{
    return total_tiles >= kArbBankTiledTilesPerCu * static_cast<long long>(num_cus);
}

// Eligibility of arb_bank_tiled_kernel: both banks of ONE channel plus the sample tile fit LDS at two workgroups a CU (160 KiB a CU:
// 78 KiB a workgroup, which leaves room for the epilogue's own word).  A tile is 256 outputs (a lane each) of one channel; its planned
// span follows from the rate -- consecutive outputs are 1/rate samples apart -- and is cut to what the samples may take (40 KiB, or
// what the banks leave): tiles with a longer run read global memory, so a rate that makes EVERY full tile such a tile is left to
// the universal kernel unless the kernel is forced.
// MRHIP_ARB_BANK_TILED=0: never; =1: wherever LDS allows (tests, measurements); unset: the measured rule above.
bool plan_arb_bank_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, ArbTileArgs *out, size_t *lds)
{
    const int mode = MRHIP_ENV_INT("MRHIP_ARB_BANK_TILED", -1);
    if (mode == 0 || !tk.bank || tk.complex_h || a.n_out < 1 || a.T < 1 || a.Nphi < 1 || !(rate > 0.0)) return false;
    const size_t rs = tk.r_f64 ? 8 : 4;                                                 // one tap
    const size_t sb = (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1);                      // one sample
    const int TP = a.T + 1;
    const size_t bank_elems = static_cast<size_t>(a.Nphi) * TP;
    const size_t banks_bytes = (2 * bank_elems * rs + 15) / 16 * 16;
    constexpr size_t kWorkgroupBytes = 78 * 1024, kSampleBytesMax = 40 * 1024;
    if (banks_bytes + static_cast<size_t>(TP) * sb > kWorkgroupBytes) return false;     // not even one window beside the banks
    const size_t sample_bytes = std::min(kSampleBytesMax, kWorkgroupBytes - banks_bytes);
    const long long tile_out = kArbBankThreads;
    // samples the run of a tile can hold: n advances by at most ceil(1/rate) + 1 per output (update(), Filters.jl:663-673)
    const double per_tile = std::ceil(static_cast<double>(tile_out - 1) / rate) + static_cast<double>(a.T) + 2.0;
    long long max_span = static_cast<long long>(sample_bytes / sb);
    const bool cut = per_tile > static_cast<double>(max_span);
    if (!cut) max_span = static_cast<long long>(per_tile);
    if (max_span < a.T + 1) return false;                                               // not even one window
    if (cut && mode != 1) return false;
    ArbTileArgs ta{};
    ta.cpl = 1;
    ta.tap_pitch = TP;
    ta.bank_elems = static_cast<int>(bank_elems);
    ta.x_offset_bytes = static_cast<int>(banks_bytes);
    ta.max_span = static_cast<int>(max_span);
    ta.tile_out = tile_out;
    ta.tiles_per_channel = (a.n_out + tile_out - 1) / tile_out;
    ta.total_tiles = ta.tiles_per_channel * a.nch;
    if (mode != 1 && !arb_bank_tiled_measured_faster(ta.total_tiles, num_cus)) return false;
    *out = ta;
    *lds = banks_bytes + static_cast<size_t>(max_span) * sb;
    return true;
}

hipError_t launch_arb_bank_tiled(const TypeKey &tk, bool fused, const ArbArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                 const char **kname, int num_cus)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    *kname = "arb_bank_tiled_kernel";
    // MRHIP_ARB_BANK_GRID: the number of workgroups of the launch (tests: one workgroup that walks every channel, runs that cross a
    // channel in mid-run, more workgroups than tiles)
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_ARB_BANK_GRID", 0);
    return dispatch_arb_bank(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto go = [&](auto kfn) -> hipError_t {
            const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kArbBankThreads, lds, num_cus, ta.total_tiles);
            if (pg.err != hipSuccess) return pg.err;
            long long g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
            if (grid_fixed > 0) g = std::min<long long>(grid_fixed, 65535);
            launch_kernel(kfn, dim3(static_cast<unsigned>(g)), dim3(kArbBankThreads), lds, s, a, ta);
            return hipGetLastError();
        };
        return fused ? go(arb_bank_tiled_kernel<TX, R, NCX, true>) : go(arb_bank_tiled_kernel<TX, R, NCX, false>);
    });
}

}  // namespace mrhip
