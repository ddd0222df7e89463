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
#include <algorithm>
#include <cstdlib>

#include "ctaps_device.h"
#include "mrhip_internal.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kBankCtapsThreads = 256;

// One thread per output, any (L, M, T, hLen): poly_ctaps_generic_kernel with the tap pointer offset by ch * L * T pairs inside the
// channel loop.  Serves host-planned calls (one lane files the end state in the record) and device-planned ones (a.dyn:
// mrhip_filt_device_async, calls under HIP-graph capture, cascade stages, a ring's stream-ordered launches).
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kBankCtapsThreads) void poly_bank_ctaps_generic_kernel(PolyArgs a)
{
    using Sample = CSample<TX, NCX>;
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
        const CPair<R> *__restrict__ tp = static_cast<const CPair<R> *>(a.taps) + static_cast<long long>(ch) * bank + static_cast<long long>(phi) * a.T;
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
        CPair<R> *__restrict__ yc = static_cast<CPair<R> *>(a.y) + static_cast<long long>(ch) * a.y_stride;
        auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
        CPair<R> acc = ctap_product<TX, R, NCX>(tp[0], sample(base));
        if (n < a.zero_start_below) acc = ctap_zero_start<R>(acc);
        for (int i = 1; i < a.T; ++i) acc = ctap_add<R>(acc, ctap_product<TX, R, NCX>(tp[i], sample(base + i)));
        yc[k] = acc;
    }
}

// Persistent workgroups in the tile order of poly_bank_tiled_kernel.  A tile is (channel, run of tile_out outputs); the tiles are ordered
// channel-major and workgroup b owns ONE contiguous run of that order, so it holds one channel's complex bank in LDS as (re, im) pairs
// (column pitch T + 1 pairs: lanes of different phases read different LDS banks; a pair of Float32 is one 8-byte LDS read, a pair of
// Float64 one 16-byte read) and reloads it only when its run crosses into the next channel.  The [history ; x] window of a tile is staged
// through LDS by plain loads; each lane owns one output.  No workgroup communicates with or waits for another one.  Host-planned calls
// only (the tiling follows the call's own count).
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kBankCtapsThreads) void poly_bank_ctaps_tiled_kernel(PolyArgs a, ArbTileArgs ta)
{
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_ctaps_smem[];
    CPair<R> *const lpfb = reinterpret_cast<CPair<R> *>(bank_ctaps_smem);
    Sample *const lx = reinterpret_cast<Sample *>(bank_ctaps_smem + ta.x_offset_bytes);

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
    const int bank_pairs = a.L * T;
    int ch_in_lds = -1;

    for (long long tile = t_begin; tile < t_end; ++tile) {
        const int ch = static_cast<int>(tile / ta.tiles_per_channel);
        const long long tau = tile - static_cast<long long>(ch) * ta.tiles_per_channel;
        const long long k0 = tau * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        int phi_unused;
        const long long n_lo = newest_of(k0, &phi_unused), n_hi = newest_of(klast, &phi_unused);
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (may be < 0)
        const int span = static_cast<int>(n_hi - n_lo) + T;                             // <= ta.max_span (plan_bank_ctaps_tiled: span_of)

        __syncthreads();   // the previous tile's reads of bank and window are done
        if (ch != ch_in_lds) {   // (uniform over the workgroup) channel ch's bank -> LDS: pair (phi, i) at phi*TP + i
            const CPair<R> *__restrict__ g0 = static_cast<const CPair<R> *>(a.taps) + static_cast<long long>(ch) * bank_pairs;
            for (int e = tid; e < bank_pairs; e += kBankCtapsThreads) {
                const int phi = e / T, i = e - phi * T;
                lpfb[phi * TP + i] = g0[e];
            }
            ch_in_lds = ch;
        }
        {
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            for (int s = tid; s < span; s += kBankCtapsThreads) {
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

        CPair<R> *__restrict__ yc = static_cast<CPair<R> *>(a.y) + static_cast<long long>(ch) * a.y_stride;
        for (long long k = k0 + tid; k <= klast; k += kBankCtapsThreads) {
            int phi;
            const long long n = newest_of(k, &phi);
            const CPair<R> *tp = lpfb + phi * TP;
            const Sample *wp = lx + (n - n_lo);             // oldest sample of this output's window
            CPair<R> acc = ctap_product<TX, R, NCX>(tp[0], wp[0]);
            if (n < a.zero_start_below) acc = ctap_zero_start<R>(acc);
#pragma unroll 4
            for (int i = 1; i < T; ++i) acc = ctap_add<R>(acc, ctap_product<TX, R, NCX>(tp[i], wp[i]));
            yc[k] = acc;
        }
    }
}

}  // namespace

hipError_t launch_poly_bank_ctaps_generic(const TypeKey &tk, const PolyArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || !tk.complex_h) return hipErrorInvalidValue;
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    const long long bx = a.n_out > 0 ? (a.n_out + kBankCtapsThreads - 1) / kBankCtapsThreads : 1;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "poly_bank_ctaps_generic_kernel";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(poly_bank_ctaps_generic_kernel<TX, R, NCX>, grid, dim3(kBankCtapsThreads), 0, s, a);
        return hipGetLastError();
    });
}

// Eligibility of poly_bank_ctaps_tiled_kernel: plan_bank_tiled's rule with the bank counted in pairs -- ONE channel's bank of pairs
// (at most 96 KB) plus the window of a tile fit the LDS budget (at most 150 KB), otherwise the call runs on the universal kernel.
// MRHIP_BANK_CTAPS_TILED: 0 never, 1 wherever the LDS plan fits (tests, measurements), -1 (default) the measured plan: calls with at
// least one tile per CU, where the tiled kernel was 1.48 ... 4.1 times faster in every row measured (DESIGN.md 9 item 11,
// profiles/r07/bank_ctaps.txt); smaller calls are unmeasured and stay on the universal kernel.
bool plan_bank_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, ArbTileArgs *out, size_t *lds)
{
    const int mode = MRHIP_ENV_INT("MRHIP_BANK_CTAPS_TILED", -1);
    if (mode == 0 || !tk.bank || !tk.complex_h || a.dyn || a.n_out < 1 || a.T < 1) return false;
    const size_t ps = (tk.r_f64 ? 8 : 4) * 2;                                           // one tap pair
    const size_t sb = (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1);                      // one sample
    const int TP = a.T + 1;
    const size_t bank_pairs = static_cast<size_t>(a.L) * TP;
    const size_t bank_bytes = (bank_pairs * ps + 15) / 16 * 16;
    if (bank_bytes > 96 * 1024) return false;
    long long tile_out = kBankCtapsThreads;
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
            ta.bank_elems = static_cast<int>(bank_pairs);
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

hipError_t launch_poly_bank_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                        const char **kname, int num_cus)
{
    if (!tk.bank || !tk.complex_h || a.dyn) return hipErrorInvalidValue;
    *kname = "poly_bank_ctaps_tiled_kernel";
    // MRHIP_BANK_CTAPS_GRID: a cap on the workgroups of the launch (a small test makes one workgroup cross channel boundaries with it)
    const int grid_cap = MRHIP_ENV_INT("MRHIP_BANK_CTAPS_GRID", 0);
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        const auto kfn = poly_bank_ctaps_tiled_kernel<TX, R, NCX>;
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kBankCtapsThreads, lds, num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        long long g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
        if (grid_cap > 0) g = std::min<long long>(g, grid_cap);
        launch_kernel(kfn, dim3(static_cast<unsigned>(g)), dim3(kBankCtapsThreads), lds, s, a, ta);
        return hipGetLastError();
    });
}

}  // namespace mrhip
