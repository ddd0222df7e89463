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
#include <algorithm>
#include <cstdlib>

#include "ctaps_device.h"
#include "mrhip_internal.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kCtapsThreads = 256;

// (CPair, CSample, ctap_product, ctap_zero_start, ctap_add, dispatch_ctaps: ctaps_device.h, shared with kernels_ctaps_arb.hip)

// One thread per output, any (L, M, T, hLen): poly_generic_kernel with complex taps.  Serves host-planned calls (files the end
// state in the record) and device-planned ones (a.dyn: mrhip_filt_device_async, calls under HIP-graph capture).
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kCtapsThreads) void poly_ctaps_generic_kernel(PolyArgs a)
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
    const CPair<R> *__restrict__ tp = static_cast<const CPair<R> *>(a.taps) + static_cast<long long>(phi) * a.T;
    for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
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

// Persistent workgroups, modelled on poly_tiled_kernel: the complex bank sits in LDS once per workgroup as (re, im) pairs with a
// column pitch of T + 1 pairs (lanes of different phases read different banks; a pair of Float32 is one 8-byte LDS read), the
// contiguous [history ; x] run of a tile of outputs is staged for CPL channels, one lane owns one output index of CPL channels.
// Host-planned calls only (the tiling follows the call's own count).
template <typename TX, typename R, int NCX, int CPL>
__global__ __launch_bounds__(kCtapsThreads) void poly_ctaps_tiled_kernel(PolyArgs a, ArbTileArgs ta)
{
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctaps_smem[];
    CPair<R> *const lpfb = reinterpret_cast<CPair<R> *>(ctaps_smem);
    Sample *const lx = reinterpret_cast<Sample *>(ctaps_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    if (a.rec && tid == 0 && blockIdx.x == 0) {                     // the host planned the call: file its end state
        a.rec->phiIdx = a.phi_end; a.rec->inputDeficit = a.d_end; a.rec->n_written = a.n_out; a.rec->calls += 1;
    }
    {   // the tap bank -> LDS once per workgroup: pair (phi, i) at phi*TP + i
        const CPair<R> *__restrict__ g0 = static_cast<const CPair<R> *>(a.taps);
        const int total = a.L * T;
        for (int e = tid; e < total; e += kCtapsThreads) {
            const int phi = e / T, i = e - phi * T;
            lpfb[phi * TP + i] = g0[e];
        }
    }
    auto newest_of = [&](long long k, int *phi) -> long long {     // 1-based index of the newest sample of output k
        const long long u = a.u0 + k * a.M;
        const long long q = u / a.L;
        *phi = static_cast<int>(u - q * a.L);
        return a.d0 + q;
    };

    for (long long tile = blockIdx.x; tile < ta.total_tiles; tile += gridDim.x) {
        const int cg = static_cast<int>(tile / ta.tiles_per_channel);                  // channel group
        const long long tau = tile - static_cast<long long>(cg) * ta.tiles_per_channel;
        const int ch0 = cg * CPL;
        const int nchl = a.nch - ch0 < CPL ? a.nch - ch0 : CPL;
        const long long k0 = tau * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        int phi_unused;
        const long long n_lo = newest_of(k0, &phi_unused), n_hi = newest_of(klast, &phi_unused);
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (may be < 0)
        const int span = static_cast<int>(n_hi - n_lo) + T;                             // <= ta.max_span (plan_ctaps_tiled: span_of)

        __syncthreads();   // previous tile's reads are done (and, first time, the tap bank is written)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            if (cc < nchl) {
                const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride;
                const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H;
                Sample *const lxc = lx + static_cast<size_t>(cc) * ta.max_span;
                for (int s = tid; s < span; s += kCtapsThreads) {
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
        __syncthreads();

        for (long long k = k0 + tid; k <= klast; k += kCtapsThreads) {
            int phi;
            const long long n = newest_of(k, &phi);
            const CPair<R> *tp = lpfb + phi * TP;
            const Sample *wp = lx + (n - n_lo);             // oldest sample of this output's window (channel 0 of the group)
            CPair<R> acc[CPL];
            {
                const CPair<R> t = tp[0];
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) acc[cc] = ctap_product<TX, R, NCX>(t, wp[static_cast<size_t>(cc) * ta.max_span]);
            }
            if (n < a.zero_start_below) {
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) acc[cc] = ctap_zero_start<R>(acc[cc]);
            }
#pragma unroll 4
            for (int i = 1; i < T; ++i) {
                const CPair<R> t = tp[i];
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc)
                    acc[cc] = ctap_add<R>(acc[cc], ctap_product<TX, R, NCX>(t, wp[static_cast<size_t>(cc) * ta.max_span + i]));
            }
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                if (cc < nchl) {
                    CPair<R> *__restrict__ yc = static_cast<CPair<R> *>(a.y) + static_cast<long long>(ch0 + cc) * a.y_stride;
                    yc[k] = acc[cc];
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_poly_ctaps_generic(const TypeKey &tk, const PolyArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    const long long bx = a.n_out > 0 ? (a.n_out + kCtapsThreads - 1) / kCtapsThreads : 1;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "poly_ctaps_generic_kernel";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(poly_ctaps_generic_kernel<TX, R, NCX>, grid, dim3(kCtapsThreads), 0, s, a);
        return hipGetLastError();
    });
}

// Eligibility of poly_ctaps_tiled_kernel: the bank of pairs plus a tile of samples fit LDS, and the call is large enough to give
// every CU a tile (below that the universal kernel's one-lane-per-output grid spreads wider than the tiles do).
// MRHIP_CTAPS_TILED=0: never; =1: whenever LDS allows (tests, measurements).
bool plan_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, ArbTileArgs *out, size_t *lds)
{
    const int mode = MRHIP_ENV_INT("MRHIP_CTAPS_TILED", -1);
    if (mode == 0 || !tk.complex_h || a.dyn || a.n_out < 1 || a.T < 1) return false;
    const size_t ps = (tk.r_f64 ? 8 : 4) * 2;                                           // one tap pair
    const size_t sb = (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1);                      // one sample
    const int TP = a.T + 1;
    const size_t bank_pairs = static_cast<size_t>(a.L) * TP;
    const size_t bank_bytes = (bank_pairs * ps + 15) / 16 * 16;
    if (bank_bytes > 96 * 1024) return false;
    int cpl = a.nch >= 32 ? 4 : (a.nch >= 8 ? 2 : 1);
    long long tile_out = kCtapsThreads;
    // samples a tile of `t` outputs can touch: floor((u_first + (t-1)*M)/L) - floor(u_first/L) + T
    auto span_of = [&](long long t) { return ((t - 1) * a.M + a.L - 1) / a.L + a.T + 1; };
    const size_t budget = std::max<size_t>(64 * 1024, std::min<size_t>(bank_bytes + 40 * 1024, 150 * 1024));
    for (;;) {
        const long long max_span = span_of(tile_out);
        const size_t total = bank_bytes + static_cast<size_t>(max_span) * sb * cpl;
        if (total <= budget || (cpl == 1 && tile_out == 64)) {
            if (total > 150 * 1024 || max_span > (1 << 30)) return false;
            const long long groups = (a.nch + cpl - 1) / cpl;
            ArbTileArgs ta{};
            ta.tap_pitch = TP;
            ta.bank_elems = static_cast<int>(bank_pairs);
            ta.x_offset_bytes = static_cast<int>(bank_bytes);
            ta.max_span = static_cast<int>(max_span);
            ta.tile_out = tile_out;
            ta.tiles_per_channel = (a.n_out + tile_out - 1) / tile_out;
            ta.total_tiles = ta.tiles_per_channel * groups;
            ta.cpl = cpl;
            if (mode != 1 && ta.total_tiles < static_cast<long long>(num_cus)) return false;
            *out = ta;
            *lds = total;
            return true;
        }
        if (cpl > 1) cpl /= 2;
        else tile_out /= 2;
    }
}

hipError_t launch_poly_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                   const char **kname, int num_cus)
{
    if (!tk.complex_h || a.dyn) return hipErrorInvalidValue;
    *kname = "poly_ctaps_tiled_kernel";
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto go = [&](auto kfn) -> hipError_t {
            const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kCtapsThreads, lds, num_cus, ta.total_tiles);
            if (pg.err != hipSuccess) return pg.err;
            launch_kernel(kfn, dim3(static_cast<unsigned>(pg.grid)), dim3(kCtapsThreads), lds, s, a, ta);
            return hipGetLastError();
        };
        switch (ta.cpl) {
        case 4: return go(poly_ctaps_tiled_kernel<TX, R, NCX, 4>);
        case 2: return go(poly_ctaps_tiled_kernel<TX, R, NCX, 2>);
        default: return go(poly_ctaps_tiled_kernel<TX, R, NCX, 1>);
        }
    });
}

}  // namespace mrhip
