// kernels_ctaps_farrow.hip -- FIRFarrow (src/Filters.jl:123-147, 764-839) with COMPLEX taps.
//
// The reference is generic over the tap type: pnfb holds one Poly{Complex{T}} per ROW of taps2pfb(h, N𝜙), and per output
// tapsforphase! stores polyval(pnfb[i], 𝜙Idx) into currentTaps::Vector{Complex{T}} before ONE Vector unsafedot over the window.
// Per output k the phase schedule (update(), :780-788; arb_schedule.hip evaluates it, the tap type plays no part in it)
// supplies the input index n_k and the Float64 phase 𝜙_k:
//
//     taps[i] = Complex{T}(polyval(pnfb[i], 𝜙_k))              i = 1 .. tapsPer𝜙
//     y_k     = sum_i taps[i] * ext[n_k - T + i]               ext = [history ; x]
//
// Arithmetic contract (include/multirate_hip.h, "Complex taps", FIRFarrow part): Horner in Float64 from the highest power PER
// COMPONENT (t = 𝜙*v; v = coef + t, the product and the sum each rounded once), the result rounded once to the tap's real
// scalar and widened exactly to R; the dot exactly as the rational family's -- oldest sample first, the first product
// initialises the accumulator, Complex*Real / Complex*Complex written out, every operation rounded separately in R
// (ctaps_device.h) -- and outputs on the seam (n < seam_below: xIdx < tapsPer𝜙 in a call that is no continuation piece) start
// from zero per component (support.jl:46).  There is no FUSED form.  This file is compiled with -ffp-contract=off.
//
// The coefficient bank is [T][polyorder+1] (re, im) pairs of Float64 on the device, ascending powers, values representable in
// the tap type; the history is Tx (real for real samples); the output is (re, im) pairs of R.  Both kernels take the ShiftFold
// epilogue (shiftin! by the workgroup that leaves last) exactly as arb_ctaps_generic_kernel does.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "ctaps_device.h"
#include "mrhip_internal.h"
#include "pair_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kCtapsFarrowThreads = 256;
// outputs a channel from which plan_ctaps_farrow_tiled takes a call by default: the smallest call measured, at which -- as at every
// larger one -- the tiled kernel beat the universal one in every run (profiles/r07/ctaps_farrow.txt); negative: only when
// MRHIP_CTAPS_TILED=1 asks for it
constexpr int kCtapsFarrowTiledMinDefault = 21000;
constexpr int kCtapsFarrowMeasuredT = 32;                  // the tapsPer𝜙 those measurements were taken at
// LDS a workgroup of the tiled kernel may take: the 160 KiB of a CU less the kernel's static words
constexpr size_t kCtapsFarrowLdsBudget = 159 * 1024;
constexpr size_t kCtapsFarrowSampleBytes = 40 * 1024;

// One complex tap of one output: polyval(Poly{Complex{T}}, 𝜙::Float64) written out (y = p[i] + x*y; Real*Complex and
// Complex+Complex are by components), stored into a Vector{Complex{T}} (one rounding to T per component), widened exactly to R.
// `c`: the polynomial's polyorder+1 (re, im) pairs, ascending powers.
template <typename R>
__device__ __forceinline__ CPair<R> farrow_ctap(const double *c, const int P, const double phase, const bool tap_f32)
{
    double vr = c[2 * P], vi = c[2 * P + 1];
    for (int j = P - 1; j >= 0; --j) {
        const double tr = phase * vr;
        vr = c[2 * j] + tr;
        const double ti = phase * vi;
        vi = c[2 * j + 1] + ti;
    }
    CPair<R> t;
    t.re = tap_f32 ? static_cast<R>(static_cast<float>(vr)) : static_cast<R>(vr);
    t.im = tap_f32 ? static_cast<R>(static_cast<float>(vi)) : static_cast<R>(vi);
    return t;
}

// One thread per output, any (Nphi, T, polyorder, rate): farrow_kernel with complex taps.  Serves every call the tiled plan
// does not take, among them the calls whose count only the device knows (a.dyn: asynchronous, device-planned and
// graph-captured calls).  cache != 0: the thread evaluates its T taps ONCE into an LDS column of its own (the taps depend on
// the output, not on the channel) and reuses them for every channel it visits; 0: the columns do not fit, the taps are
// evaluated per channel.
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kCtapsFarrowThreads) void farrow_ctaps_generic_kernel(FarrowArgs a, int cache)
{
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctaps_farrow_smem[];
    CPair<R> *const tl = reinterpret_cast<CPair<R> *>(ctaps_farrow_smem);
    const int tid = threadIdx.x, bs = blockDim.x;
    const long long k = static_cast<long long>(blockIdx.x) * bs + tid;
    if (a.dyn) a.n_out = a.dyn->n_out;              // a device-planned call: the count the schedule's FINISH kernel left
    if (k < a.n_out) {                               // (no early return: every thread takes part in the history epilogue below)
        const long long n = a.n_idx[k];
        const double phase = a.acc[k];
        const int P = a.polyorder;
        const bool tap_f32 = a.tap_f32 != 0;
        auto tap = [&](int i) -> CPair<R> { return farrow_ctap<R>(a.pnfb + static_cast<long long>(i) * (P + 1) * 2, P, phase, tap_f32); };
        if (cache)                                   // (no barrier: each thread only reads its own column)
            for (int i = 0; i < a.T; ++i) tl[i * bs + tid] = tap(i);
        const long long base = n - a.T;             // 0-based index of the oldest sample (>= -H: n >= 1)
        const bool seam = n < a.seam_below;         // kernel.xIdx < kernel.tapsPer𝜙, Filters.jl:818 (never in a piece that continues a call)
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            CPair<R> *__restrict__ yc = static_cast<CPair<R> *>(a.y) + static_cast<long long>(ch) * a.y_stride;
            auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
            CPair<R> acc = ctap_product<TX, R, NCX>(cache ? tl[tid] : tap(0), sample(base));
            if (seam) acc = ctap_zero_start<R>(acc);
            for (int i = 1; i < a.T; ++i)
                acc = ctap_add<R>(acc, ctap_product<TX, R, NCX>(cache ? tl[i * bs + tid] : tap(i), sample(base + i)));
            yc[k] = acc;
        }
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// Persistent workgroups, modelled on arb_ctaps_tiled_kernel and on the way farrow_pipe_kernel treats taps.  A tile is 256
// consecutive outputs (a lane each) of EVERY channel: the lane evaluates its output's T complex taps ONCE per tile -- 2 T
// polyorder Float64 multiply-adds, the cost that sets this kind apart -- from the coefficient bank (copied to LDS once per
// workgroup; every lane reads the same coefficient: a broadcast) into an LDS column of its own (tap i of lane l at i*256 + l: a
// wave's reads are consecutive), then walks the channel groups, CPL channels at a time: the contiguous [history ; x] run between
// the tile's first and last n_idx (the schedule is non-decreasing in k) is staged per group, and one tap read serves CPL
// products.  The span of a tile is read from the schedule HERE, so the kernel serves device-planned calls too (a.dyn); a tile
// whose run is longer than the planned span (ta.max_span: a heavily decimating rate, rate << 1) reads its windows from global
// memory.  Tiles are assigned statically (tile += gridDim.x): no tile counter, no waiting between workgroups beyond the
// shiftin_by_last_workgroup epilogue.
// LDS: [T][polyorder+1] pairs of Float64 | [T][256] pairs of R | [CPL][max_span] samples.
template <typename TX, typename R, int NCX, int CPL>
__global__ __launch_bounds__(kCtapsFarrowThreads) void farrow_ctaps_tiled_kernel(FarrowArgs a, ArbTileArgs ta)
{
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctaps_farrow_smem[];
    double *const lcoef = reinterpret_cast<double *>(ctaps_farrow_smem);
    CPair<R> *const tl = reinterpret_cast<CPair<R> *>(ctaps_farrow_smem + static_cast<size_t>(ta.bank_elems) * 2 * sizeof(double));
    Sample *const lx = reinterpret_cast<Sample *>(ctaps_farrow_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, P = a.polyorder;
    const bool tap_f32 = a.tap_f32 != 0;
    for (int e = tid; e < ta.bank_elems * 2; e += kCtapsFarrowThreads) lcoef[e] = a.pnfb[e];
    long long ngroups;                                              // (1: a tile is every channel of its outputs)
    tiles_take_dyn(a.n_out, ta, ngroups, a.dyn);                    // (a device-planned call: the count from the call record)
    const int ncg = (a.nch + CPL - 1) / CPL;
    __syncthreads();                                                // the coefficient bank is written

    for (long long tile = blockIdx.x; tile < ta.total_tiles; tile += gridDim.x) {
        const long long k0 = tile * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        const long long n_lo = a.n_idx[k0], n_hi = a.n_idx[klast];
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (>= -H)
        const long long span = n_hi - n_lo + T;
        const bool staged = span <= ta.max_span;                                        // (uniform over the workgroup)
        const long long k = k0 + tid;
        const bool active = k <= klast;
        long long n = n_lo;
        bool seam = false;
        if (active) {
            n = a.n_idx[k];
            seam = n < a.seam_below;
            const double phase = a.acc[k];
            for (int i = 0; i < T; ++i)                  // (the column is this lane's alone: no barrier between tiles or before the reads)
                tl[i * kCtapsFarrowThreads + tid] = farrow_ctap<R>(lcoef + i * (P + 1) * 2, P, phase, tap_f32);
        }
        const CPair<R> *const tcol = tl + tid;

#pragma unroll 1
        for (int cg = 0; cg < ncg; ++cg) {
            const int ch0 = cg * CPL;
            const int nchl = a.nch - ch0 < CPL ? a.nch - ch0 : CPL;
            __syncthreads();   // the previous group's (and tile's) reads of the samples are done
            if (staged) {
#pragma unroll 1
                for (int cc = 0; cc < nchl; ++cc) {
                    const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride;
                    const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H;
                    Sample *const lxc = lx + static_cast<size_t>(cc) * ta.max_span;
                    for (int s = tid; s < static_cast<int>(span); s += kCtapsFarrowThreads) {
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
            if (!active) continue;                       // (no barrier below)

            CPair<R> acc[CPL];
            if (staged) {
                const Sample *wp = lx + (n - n_lo);      // oldest sample of this output's window (channel 0 of the group)
                {
                    const CPair<R> t = tcol[0];
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) {
                        acc[cc] = ctap_product<TX, R, NCX>(t, wp[static_cast<size_t>(cc) * ta.max_span]);
                        if (seam) acc[cc] = ctap_zero_start<R>(acc[cc]);
                    }
                }
#pragma unroll 2
                for (int i = 1; i < T; ++i) {
                    const CPair<R> t = tcol[i * kCtapsFarrowThreads];
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc)
                        acc[cc] = ctap_add<R>(acc[cc], ctap_product<TX, R, NCX>(t, wp[static_cast<size_t>(cc) * ta.max_span + i]));
                }
            } else {
                // the windows from global memory, a channel at a time (the taps are read from the lane's column once per channel here)
                const long long base = n - T;
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    if (cc < nchl) {
                        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride;
                        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H + a.H;
                        CPair<R> l = ctap_product<TX, R, NCX>(tcol[0], base >= 0 ? xc[base] : hc[base]);
                        if (seam) l = ctap_zero_start<R>(l);
                        for (int i = 1; i < T; ++i) {
                            const long long xi = base + i;
                            l = ctap_add<R>(l, ctap_product<TX, R, NCX>(tcol[i * kCtapsFarrowThreads], xi >= 0 ? xc[xi] : hc[xi]));
                        }
                        acc[cc] = l;
                    }
                }
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
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

}  // namespace

hipError_t launch_farrow_ctaps_generic(const TypeKey &tk, const FarrowArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    *kname = "farrow_ctaps_generic_kernel";
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        // block size: as many outputs as keep one LDS column of T tap pairs per thread within 64 KiB (launch_farrow's rule)
        const long long per_thread = static_cast<long long>(a.T) * static_cast<long long>(sizeof(CPair<R>));
        int bs = static_cast<int>(65536 / per_thread) / 64 * 64;
        const bool cache = bs >= 64;
        if (bs > kCtapsFarrowThreads || !cache) bs = kCtapsFarrowThreads;
        const size_t lds = cache ? static_cast<size_t>(per_thread) * bs : 0;
        const long long bx = std::max<long long>((a.n_out + bs - 1) / bs, 1);
        if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
        // channels are split over blockIdx.y only as far as needed to fill the machine: the taps are evaluated once per
        // (output, blockIdx.y)
        long long by = 1;
        while (by < a.nch && bx * by < 2048) by *= 2;
        if (by > a.nch) by = a.nch;
        const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(by), 1);
        launch_kernel(farrow_ctaps_generic_kernel<TX, R, NCX>, grid, dim3(bs), lds, s, a, cache ? 1 : 0);
        return hipGetLastError();
    });
}

// Eligibility of farrow_ctaps_tiled_kernel (beside plan_ctaps_arb_tiled, kernels_ctaps_arb.hip): the coefficient bank of pairs,
// 256 tap columns and a tile of samples fit the 160 KiB of LDS of a CU.  A tile is 256 outputs (a lane each) of every channel,
// CPL channels at a time; its planned span follows from the rate -- consecutive outputs are 1/rate samples apart -- and is
// cut to what the samples may take (40 KiB, or what the bank and the columns leave): tiles with a longer run read global
// memory, so a rate that makes EVERY full tile such a tile is left to the universal kernel unless the kernel is forced.
// MRHIP_CTAPS_TILED=0: never; =1: whenever LDS allows (tests, measurements); unset: the measured rule at the end.
bool plan_ctaps_farrow_tiled(const TypeKey &tk, const FarrowArgs &a, double rate, int /*num_cus*/, ArbTileArgs *out, size_t *lds)
{
    const int mode = MRHIP_ENV_INT("MRHIP_CTAPS_TILED", -1);
    if (mode == 0 || !tk.complex_h || a.n_out < 1 || a.T < 1 || a.polyorder < 0 || !(rate > 0.0)) return false;
    const size_t ps = (tk.r_f64 ? 8 : 4) * 2;                                           // one tap pair
    const size_t sb = (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1);                      // one sample
    const size_t bank_pairs = static_cast<size_t>(a.T) * (a.polyorder + 1);
    const size_t bank_bytes = bank_pairs * 2 * sizeof(double);                          // (whole 16-byte units)
    const size_t col_bytes = static_cast<size_t>(a.T) * kCtapsFarrowThreads * ps;
    if (bank_bytes + col_bytes >= kCtapsFarrowLdsBudget) return false;
    const size_t sample_bytes = std::min(kCtapsFarrowSampleBytes, kCtapsFarrowLdsBudget - bank_bytes - col_bytes) / 16 * 16;
    const long long tile_out = kCtapsFarrowThreads;
    // samples the run of a tile can hold: n advances by at most ceil(1/rate) + 1 per output (update(), Filters.jl:780-788)
    const double per_tile = std::ceil(static_cast<double>(tile_out - 1) / rate) + static_cast<double>(a.T) + 2.0;
    // (CPL = 1 or 2, as in arb_ctaps_tiled_kernel)
    int cpl = a.nch >= 2 ? 2 : 1;
    while (cpl > 1 && per_tile * static_cast<double>(sb * cpl) > static_cast<double>(sample_bytes)) cpl /= 2;
    long long max_span = static_cast<long long>(sample_bytes / (sb * cpl));
    const bool cut = per_tile > static_cast<double>(max_span);
    if (!cut) max_span = static_cast<long long>(per_tile);
    if (max_span < a.T + 1) return false;                                               // not even one window
    if (cut && mode != 1) return false;
    ArbTileArgs ta{};
    ta.cpl = cpl;
    ta.bank_elems = static_cast<int>(bank_pairs);
    ta.x_offset_bytes = static_cast<int>(bank_bytes + col_bytes);
    ta.max_span = static_cast<int>(max_span);
    ta.tile_out = tile_out;
    ta.tiles_per_channel = (a.n_out + tile_out - 1) / tile_out;
    ta.total_tiles = ta.tiles_per_channel;                                              // a tile covers every channel
    if (mode != 1) {
        // The default rule: only where the tiled kernel was measured, and faster than the universal one in every run
        // (profiles/r07/ctaps_farrow.txt): Float32 arithmetic, 32 taps per phase, 1 to 64 channels, 21 230 outputs a channel and more
        // (83 tiles: fewer than the chip has CUs, and still ahead).  Float64 arithmetic and other banks are not measured yet and stay
        // on the universal kernel.  MRHIP_CTAPS_FARROW_TILED_MIN: another threshold, in outputs a channel.
        if (tk.r_f64 || a.T != kCtapsFarrowMeasuredT) return false;
        const long long min_out = MRHIP_ENV_INT("MRHIP_CTAPS_FARROW_TILED_MIN", kCtapsFarrowTiledMinDefault);
        if (min_out < 0 || a.n_out < min_out) return false;
    }
    *out = ta;
    *lds = bank_bytes + col_bytes + static_cast<size_t>(max_span) * sb * cpl;
    return true;
}

hipError_t launch_farrow_ctaps_tiled(const TypeKey &tk, const FarrowArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                     const char **kname, int num_cus)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    *kname = "farrow_ctaps_tiled_kernel";
    return dispatch_ctaps(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto go = [&](auto kfn) -> hipError_t {
            const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kCtapsFarrowThreads, lds, num_cus, ta.total_tiles);
            if (pg.err != hipSuccess) return pg.err;
            launch_kernel(kfn, dim3(static_cast<unsigned>(pg.grid)), dim3(kCtapsFarrowThreads), lds, s, a, ta);
            return hipGetLastError();
        };
        return ta.cpl == 2 ? go(farrow_ctaps_tiled_kernel<TX, R, NCX, 2>) : go(farrow_ctaps_tiled_kernel<TX, R, NCX, 1>);
    });
}

}  // namespace mrhip
