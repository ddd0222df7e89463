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
// fed x_c.  This file is compiled with -ffp-contract=off; FUSED calls fma explicitly.
#include <algorithm>
#include <cstdlib>

#include "mrhip_internal.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kBankThreads = 256;

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

// One thread per output, any (L, M, T, hLen): poly_generic_kernel with taps + ch * L * T.  Serves host-planned calls (one lane files
// the end state in the record) and device-planned ones (a.dyn: mrhip_filt_device_async, calls under HIP-graph capture, the chunked
// entry, cascade stages, a ring's stream-ordered launches).
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kBankThreads) void poly_bank_generic_kernel(PolyArgs a)
{
    using Sample = BankSample<TX, NCX>;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a.dyn) { a.n_out = a.dyn->n_out; a.u0 = a.dyn->u0; a.d0 = a.dyn->d0; }
    else if (a.rec && k == 0 && blockIdx.y == 0) {
        a.rec->phiIdx = a.phi_end; a.rec->inputDeficit = a.d_end; a.rec->n_written = a.n_out; a.rec->calls += 1;
    }
    if (k >= a.n_out) return;
    const long long u = a.u0 + k * a.M;
    const long long q = u / a.L;
    const int phi = static_cast<int>(u - q * a.L);
    const long long n = a.d0 + q;              // 1-based newest-sample index
    const long long base = n - a.T;            // 0-based index of the oldest sample
    const long long bank = static_cast<long long>(a.L) * a.T;
    for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
        const R *__restrict__ tp = static_cast<const R *>(a.taps) + static_cast<long long>(ch) * bank + static_cast<long long>(phi) * a.T;
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
        R *__restrict__ yc = static_cast<R *>(a.y) + static_cast<long long>(ch) * a.y_stride * NCX;
        auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
        R acc[NCX];
        {
            const Sample v = sample(base);
            const R t0 = tp[0];
#pragma unroll
            for (int c = 0; c < NCX; ++c) acc[c] = t0 * static_cast<R>(v.c[c]);
        }
        if (n < a.zero_start_below) {          // support.jl:46 (see poly_generic_kernel)
#pragma unroll
            for (int c = 0; c < NCX; ++c) acc[c] = static_cast<R>(0) + acc[c];
        }
        for (int i = 1; i < a.T; ++i) {
            const Sample v = sample(base + i);
            const R t = tp[i];
#pragma unroll
            for (int c = 0; c < NCX; ++c) acc[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), acc[c]);
        }
#pragma unroll
        for (int c = 0; c < NCX; ++c) yc[k * NCX + c] = acc[c];
    }
}

// Persistent workgroups, modelled on poly_tiled_kernel.  A tile is (channel, run of tile_out outputs); the tiles are ordered
// channel-major and workgroup b owns ONE contiguous run of that order, so it holds one channel's bank in LDS (column pitch T + 1:
// lanes of different phases read different LDS banks) and reloads it only when its run crosses into the next channel.  The
// [history ; x] window of a tile is staged through LDS.  No workgroup communicates with or waits for another one.  Host-planned calls
// only (the tiling follows the call's own count).
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kBankThreads) void poly_bank_tiled_kernel(PolyArgs a, ArbTileArgs ta)
{
    using Sample = BankSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_smem[];
    R *const lpfb = reinterpret_cast<R *>(bank_smem);
    Sample *const lx = reinterpret_cast<Sample *>(bank_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    if (a.rec && tid == 0 && blockIdx.x == 0) {                     // the host planned the call: file its end state
        a.rec->phiIdx = a.phi_end; a.rec->inputDeficit = a.d_end; a.rec->n_written = a.n_out; a.rec->calls += 1;
    }
    auto newest_of = [&](long long k, int *phi) -> long long {     // 1-based index of the newest sample of output k
        const long long u = a.u0 + k * a.M;
        const long long q = u / a.L;
        *phi = static_cast<int>(u - q * a.L);
        return a.d0 + q;
    };
    // this workgroup's run of the channel-major tile order: [t_begin, t_end)
    const long long per = ta.total_tiles / gridDim.x, extra = ta.total_tiles - per * gridDim.x;
    const long long b = blockIdx.x;
    const long long t_begin = b * per + (b < extra ? b : extra);
    const long long t_end = t_begin + per + (b < extra ? 1 : 0);
    const int bank_elems = a.L * T;
    int ch_in_lds = -1;

    for (long long tile = t_begin; tile < t_end; ++tile) {
        const int ch = static_cast<int>(tile / ta.tiles_per_channel);
        const long long tau = tile - static_cast<long long>(ch) * ta.tiles_per_channel;
        const long long k0 = tau * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        int phi_unused;
        const long long n_lo = newest_of(k0, &phi_unused), n_hi = newest_of(klast, &phi_unused);
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (may be < 0)
        const int span = static_cast<int>(n_hi - n_lo) + T;                             // <= ta.max_span (plan_bank_tiled: span_of)

        __syncthreads();   // the previous tile's reads of bank and window are done
        if (ch != ch_in_lds) {   // (uniform over the workgroup) channel ch's bank -> LDS: element (phi, i) at phi*TP + i
            const R *__restrict__ g0 = static_cast<const R *>(a.taps) + static_cast<long long>(ch) * bank_elems;
            for (int e = tid; e < bank_elems; e += kBankThreads) {
                const int phi = e / T, i = e - phi * T;
                lpfb[phi * TP + i] = g0[e];
            }
            ch_in_lds = ch;
        }
        {
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            for (int s = tid; s < span; s += kBankThreads) {
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
        for (long long k = k0 + tid; k <= klast; k += kBankThreads) {
            int phi;
            const long long n = newest_of(k, &phi);
            const R *tp = lpfb + phi * TP;
            const Sample *wp = lx + (n - n_lo);             // oldest sample of this output's window
            R acc[NCX];
            {
                const R t = tp[0];
                const Sample v = wp[0];
#pragma unroll
                for (int c = 0; c < NCX; ++c) acc[c] = t * static_cast<R>(v.c[c]);
            }
            if (n < a.zero_start_below) {                   // support.jl:46 (see poly_generic_kernel)
#pragma unroll
                for (int c = 0; c < NCX; ++c) acc[c] = static_cast<R>(0) + acc[c];
            }
#pragma unroll 4
            for (int i = 1; i < T; ++i) {
                const R t = tp[i];
                const Sample v = wp[i];
#pragma unroll
                for (int c = 0; c < NCX; ++c) acc[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), acc[c]);
            }
#pragma unroll
            for (int c = 0; c < NCX; ++c) yc[k * NCX + c] = acc[c];
        }
    }
}

// (Tx scalar, R) combinations that promote_type can produce: (f32,f32) (f32,f64) (f64,f64), real and complex samples
template <typename F>
hipError_t dispatch_bank(const TypeKey &tk, F &&f)
{
    if (!tk.x_f64 && !tk.r_f64) return tk.complex_x ? f.template operator()<float, float, 2>() : f.template operator()<float, float, 1>();
    if (!tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<float, double, 2>() : f.template operator()<float, double, 1>();
    if (tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<double, double, 2>() : f.template operator()<double, double, 1>();
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_poly_bank_generic(const TypeKey &tk, bool fused, const PolyArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    const long long bx = a.n_out > 0 ? (a.n_out + kBankThreads - 1) / kBankThreads : 1;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "poly_bank_generic_kernel";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_bank(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        if (fused) launch_kernel(poly_bank_generic_kernel<TX, R, NCX, true>, grid, dim3(kBankThreads), 0, s, a);
        else launch_kernel(poly_bank_generic_kernel<TX, R, NCX, false>, grid, dim3(kBankThreads), 0, s, a);
        return hipGetLastError();
    });
}

// Eligibility of poly_bank_tiled_kernel: ONE channel's bank plus the window of a tile fit the LDS budget (otherwise the call runs on
// the universal kernel).  MRHIP_BANK_TILED: 0 never, 1 wherever the LDS plan fits (tests, measurements), -1 (default) the measured
// plan: calls with at least one tile per CU, where the tiled kernel was 1.12 ... 3.6 times faster in every row measured (DESIGN.md 9
// item 10, profiles/r07/bank.txt); smaller calls are unmeasured and stay on the universal kernel.
bool plan_bank_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, ArbTileArgs *out, size_t *lds)
{
    const int mode = MRHIP_ENV_INT("MRHIP_BANK_TILED", -1);
    if (mode == 0 || !tk.bank || tk.complex_h || a.dyn || a.n_out < 1 || a.T < 1) return false;
    const size_t rs = tk.r_f64 ? 8 : 4;
    const size_t sb = (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1);
    const int TP = a.T + 1;
    const size_t bank_elems = static_cast<size_t>(a.L) * TP;
    const size_t bank_bytes = (bank_elems * rs + 15) / 16 * 16;
    if (bank_bytes > 96 * 1024) return false;
    long long tile_out = kBankThreads;
    // samples a tile of `t` outputs can touch: floor((u_first + (t-1)*M)/L) - floor(u_first/L) + T  (as plan_ctaps_tiled)
    auto span_of = [&](long long t) { return ((t - 1) * a.M + a.L - 1) / a.L + a.T + 1; };
    const size_t budget = std::max<size_t>(64 * 1024, std::min<size_t>(bank_bytes + 40 * 1024, 150 * 1024));
    for (;;) {
        const long long max_span = span_of(tile_out);
        const size_t total = bank_bytes + static_cast<size_t>(max_span) * sb;
        if (total <= budget || tile_out == 64) {
            if (total > 150 * 1024 || max_span > (1 << 30)) return false;
            ArbTileArgs ta{};
            ta.cpl = 1;
            ta.tap_pitch = TP;
            ta.bank_elems = static_cast<int>(bank_elems);
            ta.x_offset_bytes = static_cast<int>(bank_bytes);
            ta.max_span = static_cast<int>(max_span);
            ta.tile_out = tile_out;
            ta.tiles_per_channel = (a.n_out + tile_out - 1) / tile_out;
            ta.total_tiles = ta.tiles_per_channel * a.nch;
            if (mode != 1 && ta.total_tiles < static_cast<long long>(num_cus)) return false;   // (below a tile per CU the universal kernel's grid spreads wider)
            *out = ta;
            *lds = total;
            return true;
        }
        tile_out /= 2;
    }
}

hipError_t launch_poly_bank_tiled(const TypeKey &tk, bool fused, const PolyArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                  const char **kname, int num_cus)
{
    if (!tk.bank || tk.complex_h || a.dyn) return hipErrorInvalidValue;
    *kname = "poly_bank_tiled_kernel";
    // MRHIP_BANK_GRID: a cap on the workgroups of the launch (a small test makes one workgroup cross channel boundaries with it)
    const int grid_cap = MRHIP_ENV_INT("MRHIP_BANK_GRID", 0);
    return dispatch_bank(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto go = [&](auto kfn) -> hipError_t {
            const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kBankThreads, lds, num_cus, ta.total_tiles);
            if (pg.err != hipSuccess) return pg.err;
            long long g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
            if (grid_cap > 0) g = std::min<long long>(g, grid_cap);
            launch_kernel(kfn, dim3(static_cast<unsigned>(g)), dim3(kBankThreads), lds, s, a, ta);
            return hipGetLastError();
        };
        return fused ? go(poly_bank_tiled_kernel<TX, R, NCX, true>) : go(poly_bank_tiled_kernel<TX, R, NCX, false>);
    });
}

}  // namespace mrhip
