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
// Shared with the other variant units: variant_device.h (staging, launch shapes); the tiled plan: host_logic.cpp.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

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
__global__ __launch_bounds__(kVariantThreads) void farrow_ctaps_generic_kernel(FarrowArgs a, int cache)
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

// Persistent workgroups, as arb_ctaps_tiled_kernel, with taps treated as in farrow_pipe_kernel.  A tile is 256
// consecutive outputs (a lane each) of EVERY channel: the lane evaluates its output's T complex taps ONCE per tile -- 2 T
// polyorder Float64 multiply-adds, the cost that sets this kind apart -- from the coefficient bank (copied to LDS once per
// workgroup; every lane reads the same coefficient: a broadcast) into an LDS column of its own (tap i of lane l at i*256 + l: a
// wave's reads are consecutive), then walks the channel groups, CPL channels at a time: the tile's run of samples (tile_span) is
// staged per group, and one tap read serves CPL products.  Tiles are assigned statically (tile += gridDim.x): no tile counter, no
// waiting between workgroups beyond the shiftin_by_last_workgroup epilogue.
// LDS: [T][polyorder+1] pairs of Float64 | [T][256] pairs of R | [CPL][max_span] samples.
template <typename TX, typename R, int NCX, int CPL>
__global__ __launch_bounds__(kVariantThreads) void farrow_ctaps_tiled_kernel(FarrowArgs a, ArbTileArgs ta)
{
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ctaps_farrow_smem[];
    double *const lcoef = reinterpret_cast<double *>(ctaps_farrow_smem);
    CPair<R> *const tl = reinterpret_cast<CPair<R> *>(ctaps_farrow_smem + static_cast<size_t>(ta.bank_elems) * 2 * sizeof(double));
    Sample *const lx = reinterpret_cast<Sample *>(ctaps_farrow_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, P = a.polyorder;
    const bool tap_f32 = a.tap_f32 != 0;
    for (int e = tid; e < ta.bank_elems * 2; e += kVariantThreads) lcoef[e] = a.pnfb[e];
    long long ngroups;                                              // (1: a tile is every channel of its outputs)
    tiles_take_dyn(a.n_out, ta, ngroups, a.dyn);                    // (a device-planned call: the count from the call record)
    const int ncg = (a.nch + CPL - 1) / CPL;
    __syncthreads();                                                // the coefficient bank is written

    for (long long tile = blockIdx.x; tile < ta.total_tiles; tile += gridDim.x) {
        const long long k0 = tile * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        const TileSpan w = tile_span(a.n_idx, k0, klast, T, ta.max_span);
        const long long k = k0 + tid;
        const bool active = k <= klast;
        long long n = w.n_lo;
        bool seam = false;
        if (active) {
            n = a.n_idx[k];
            seam = n < a.seam_below;
            const double phase = a.acc[k];
            for (int i = 0; i < T; ++i)                  // (the column is this lane's alone: no barrier between tiles or before the reads)
                tl[i * kVariantThreads + tid] = farrow_ctap<R>(lcoef + i * (P + 1) * 2, P, phase, tap_f32);
        }
        const CPair<R> *const tcol = tl + tid;

#pragma unroll 1
        for (int cg = 0; cg < ncg; ++cg) {
            const int ch0 = cg * CPL;
            const int nchl = a.nch - ch0 < CPL ? a.nch - ch0 : CPL;
            __syncthreads();   // the previous group's (and tile's) reads of the samples are done
            if (w.staged) {
#pragma unroll 1
                for (int cc = 0; cc < nchl; ++cc)
                    stage_window(lx + static_cast<size_t>(cc) * ta.max_span, static_cast<const Sample *>(a.x) + static_cast<long long>(ch0 + cc) * a.x_stride,
                                 static_cast<const Sample *>(a.hist) + static_cast<long long>(ch0 + cc) * a.H, w.o, static_cast<int>(w.span), a.x_len, a.H, tid);
            }
            __syncthreads();
            if (!active) continue;                       // (no barrier below)

            CPair<R> acc[CPL];
            if (w.staged) {
                const Sample *wp = lx + (n - w.n_lo);      // oldest sample of this output's window (channel 0 of the group)
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
                    const CPair<R> t = tcol[i * kVariantThreads];
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
                            l = ctap_add<R>(l, ctap_product<TX, R, NCX>(tcol[i * kVariantThreads], xi >= 0 ? xc[xi] : hc[xi]));
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
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        // block size: as many outputs as keep one LDS column of T tap pairs per thread within 64 KiB (launch_farrow's rule)
        const long long per_thread = static_cast<long long>(a.T) * static_cast<long long>(sizeof(CPair<R>));
        int bs = static_cast<int>(65536 / per_thread) / 64 * 64;
        const bool cache = bs >= 64;
        if (bs > kVariantThreads || !cache) bs = kVariantThreads;
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

// (MRHIP_CTAPS_FARROW_TILED_MIN: the threshold of the default rule, outputs a channel)
bool plan_ctaps_farrow_tiled(const TypeKey &tk, const FarrowArgs &a, double rate, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_ctaps_farrow_tiled(tk, a, rate, num_cus, MRHIP_ENV_INT("MRHIP_CTAPS_TILED", -1),
                                   MRHIP_ENV_INT("MRHIP_CTAPS_FARROW_TILED_MIN", kCtapsFarrowTiledMinDefault), out, lds);
}

hipError_t launch_farrow_ctaps_tiled(const TypeKey &tk, const FarrowArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                     const char **kname, int num_cus)
{
    if (!tk.complex_h) return hipErrorInvalidValue;
    *kname = "farrow_ctaps_tiled_kernel";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return ta.cpl == 2 ? launch_persistent(farrow_ctaps_tiled_kernel<TX, R, NCX, 2>, a, ta, lds, s, num_cus)
                           : launch_persistent(farrow_ctaps_tiled_kernel<TX, R, NCX, 1>, a, ta, lds, s, num_cus);
    });
}

}  // namespace mrhip
