// variant_device.h -- what the nine "variant" units (complex taps: kernels_ctaps*.hip; per-channel taps: kernels_bank*.hip) share,
// stated ONCE: the dispatch over (Tx scalar, R, components), the staging of a [history ; x] window into LDS, the hand-out of the
// channel-major tile order, the small statements of the rational and FIRArbitrary kernels, the TAP ALGEBRA -- the only thing in which a
// real-tap and a complex-tap body differ -- the bodies that are one kernel under two algebras, and the two launch shapes.  The plans of
// the tiled kernels: host_logic.cpp.  The statements inside the algebras are the contract of include/multirate_hip.h: oldest sample
// first, the first product initialises the sum, every operation rounded separately in R, FUSED (real taps only) one explicit fma per
// tap (mac, pipe_stage.h).  The two per-channel-rate units (kernels_rates_arb.hip, kernels_rates_farrow.hip: shared and per-channel taps in
// ONE text each, BANK the kernels' last template argument) use the dispatch, the staging, the tile hand-out, RealTaps and the FIRFarrow
// coefficient reads from here and keep their kernels to themselves.  The including units are compiled with -ffp-contract=off.
#pragma once

#include <algorithm>

#include "ctaps_device.h"
#include "mrhip_internal.h"
#include "pipe_stage.h"

#pragma clang fp contract(off)

namespace mrhip {

// (Tx scalar, R, components of a sample) that promote_type can produce: (f32,f32) (f32,f64) (f64,f64), real and complex samples
template <typename F>
hipError_t dispatch_variant(const TypeKey &tk, F &&f)
{
    if (!tk.x_f64 && !tk.r_f64) return tk.complex_x ? f.template operator()<float, float, 2>() : f.template operator()<float, float, 1>();
    if (!tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<float, double, 2>() : f.template operator()<float, double, 1>();
    if (tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<double, double, 2>() : f.template operator()<double, double, 1>();
    return hipErrorInvalidValue;
}
// ... and one bool beside them: the last template argument of the per-channel-rate kernels (BANK, kernels_rates_*.hip)
template <typename F>
hipError_t dispatch_variant_flag(const TypeKey &tk, bool flag, F &&f)
{
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return flag ? f.template operator()<TX, R, NCX, true>() : f.template operator()<TX, R, NCX, false>();
    });
}

// ---- FIRFarrow with per-channel taps: the coefficient reads and the Horner chains ------------------------------------------------
// The polynomial bank is never written while a filter exists: through the constant address space the compiler uses scalar loads for
// the wave-uniform coefficient indices (it cannot prove that for a global pointer next to the y stores).
typedef const __attribute__((address_space(4))) double *farrow_coef_t;

// polyorder 4 is the default of every constructor above this library and the one every measurement was taken at: its Horner chains are
// unrolled (kFarrowBankUnrolledP); every other polyorder takes the runtime loop.  The branch is on a kernel argument: uniform.
constexpr int kFarrowBankUnrolledP = 4;

// polyval(pnfb_c[i], 𝜙) by Horner in Float64 (Polynomials.jl: y = p[end]; y = p[i] + x*y), NC chains side by side: 1 for a real
// polynomial, 2 for a Poly{Complex} (Real*Complex and Complex+Complex are by components; the coefficients are (re, im) pairs).
// `c`: the polynomial's (P+1)*NC scalars, ascending powers, wave-uniform.  Per step and component t = 𝜙*v; v = coef + t, the product and
// the sum each rounded once, never fused.  PP >= 0: the polyorder at compile time -- the (P+1)*NC scalar loads of a tap are issued
// together and waited for once; PP < 0: any polyorder, the loads inside the loop.  The arithmetic is the same statement either way.
template <int PP, int NC>
__device__ __forceinline__ void farrow_bank_horner(farrow_coef_t c, const int P, const double phase, double (&v)[NC])
{
    if constexpr (PP >= 0) {
        double cj[(PP + 1) * NC];
#pragma unroll
        for (int e = 0; e < (PP + 1) * NC; ++e) cj[e] = c[e];
#pragma unroll
        for (int q = 0; q < NC; ++q) v[q] = cj[PP * NC + q];
#pragma unroll
        for (int j = PP - 1; j >= 0; --j) {
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const double t = phase * v[q];
                v[q] = cj[j * NC + q] + t;
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < NC; ++q) v[q] = c[P * NC + q];
        for (int j = P - 1; j >= 0; --j) {
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const double t = phase * v[q];
                v[q] = c[j * NC + q] + t;
            }
        }
    }
}

// ---- the tap algebras --------------------------------------------------------------------------------------------------------
// Tap: one tap in global memory and LDS; Sum: the running sum(s) of one output; first / zero_start (support.jl:46) / step / the
// FIRArbitrary combine (yLower + yUpper * α in Float64: src/Filters.jl:724-730) / the store of one output; ComplexTaps also the FIRFarrow
// tap of one (channel, output) from its polynomial (stored into currentTaps::Vector{Th}: one rounding to the tap's real scalar, widened
// exactly to R) -- RealTaps would evaluate one chain to an R (farrow_bank_horner<PP, 1>) once farrow_bank_generic_kernel joins the body.

// real taps: NCX independent real dot products
template <typename TX, typename R, int NCX, bool FUSED>
struct RealTaps {
    using Tx = TX;
    static constexpr int NC = NCX;
    using Sample = CSample<TX, NCX>;
    using Tap = R;
    struct Sum { R c[NCX]; };
    using Out = R;
    static __device__ __forceinline__ Sum first(const Tap t, const Sample v)
    {
        Sum s;
#pragma unroll
        for (int c = 0; c < NCX; ++c) s.c[c] = t * static_cast<R>(v.c[c]);
        return s;
    }
    static __device__ __forceinline__ Sum zero_start(Sum s)
    {
#pragma unroll
        for (int c = 0; c < NCX; ++c) s.c[c] = static_cast<R>(0) + s.c[c];
        return s;
    }
    static __device__ __forceinline__ Sum step(Sum s, const Tap t, const Sample v)
    {
#pragma unroll
        for (int c = 0; c < NCX; ++c) s.c[c] = mac<FUSED, R>(t, static_cast<R>(v.c[c]), s.c[c]);
        return s;
    }
    // both sides promote to Float64 (α is a Float64 in the reference): product and sum each rounded once, the store rounds to R
    static __device__ __forceinline__ Sum arb_combine(const Sum lo, const Sum up, const double alpha)
    {
        Sum y;
#pragma unroll
        for (int c = 0; c < NCX; ++c) {
            const double prod = static_cast<double>(up.c[c]) * alpha;
            const double sum = static_cast<double>(lo.c[c]) + prod;
            y.c[c] = static_cast<R>(sum);
        }
        return y;
    }
    static __device__ __forceinline__ Out *channel_out(void *y, long long ch, long long y_stride) { return static_cast<R *>(y) + ch * y_stride * NCX; }
    static __device__ __forceinline__ void store(Out *yc, long long k, const Sum s)
    {
#pragma unroll
        for (int c = 0; c < NCX; ++c) yc[k * NCX + c] = s.c[c];
    }
};

// complex taps: (re, im) pairs of R, the statements of ctaps_device.h; no FUSED form
template <typename TX, typename R, int NCX>
struct ComplexTaps {
    using Tx = TX;
    static constexpr int NC = NCX;
    using Sample = CSample<TX, NCX>;
    using Tap = CPair<R>;
    using Sum = CPair<R>;
    using Out = CPair<R>;
    static __device__ __forceinline__ Sum first(const Tap t, const Sample v) { return ctap_product<TX, R, NCX>(t, v); }
    static __device__ __forceinline__ Sum zero_start(const Sum s) { return ctap_zero_start<R>(s); }
    static __device__ __forceinline__ Sum step(const Sum s, const Tap t, const Sample v) { return ctap_add<R>(s, ctap_product<TX, R, NCX>(t, v)); }
    static __device__ __forceinline__ Sum arb_combine(const Sum lo, const Sum up, const double alpha) { return ctap_arb_combine<R>(lo, up, alpha); }
    static constexpr int kCoefScalars = 2;       // an (re, im) pair of Float64 per polynomial coefficient
    template <int PP>
    static __device__ __forceinline__ Tap farrow_tap(farrow_coef_t c, const int P, const double phase, const bool tap_f32)
    {
        double v[2];
        farrow_bank_horner<PP, 2>(c, P, phase, v);
        Tap t;
        t.re = tap_f32 ? static_cast<R>(static_cast<float>(v[0])) : static_cast<R>(v[0]);
        t.im = tap_f32 ? static_cast<R>(static_cast<float>(v[1])) : static_cast<R>(v[1]);
        return t;
    }
    static __device__ __forceinline__ Out *channel_out(void *y, long long ch, long long y_stride) { return static_cast<Out *>(y) + ch * y_stride; }
    static __device__ __forceinline__ void store(Out *yc, long long k, const Sum s) { yc[k] = s; }
};

// ---- shared statements -------------------------------------------------------------------------------------------------------

// `span` samples of one channel's [history ; x] from x index `o` (may be < 0: history; zero outside both) -> LDS
template <typename Sample>
__device__ __forceinline__ void stage_window(Sample *lx, const Sample *__restrict__ xc, const Sample *__restrict__ hc, long long o, int span,
                                             long long x_len, int H, int tid)
{
    for (int s = tid; s < span; s += kVariantThreads) {
        const long long gi = o + s;
        Sample v;
#pragma unroll
        for (int c = 0; c < static_cast<int>(sizeof(v.c) / sizeof(v.c[0])); ++c) v.c[c] = 0;
        if (gi >= 0) { if (gi < x_len) v = xc[gi]; }
        else if (gi >= -static_cast<long long>(H)) v = hc[H + gi];
        lx[s] = v;
    }
}

// one tap bank [Nphi][T] -> LDS with a column pitch of TP taps: element (phi, i) at phi*TP + i
template <typename Tap>
__device__ __forceinline__ void bank_to_lds(Tap *lpfb, const Tap *__restrict__ g0, int elems, int T, int TP, int tid)
{
    for (int e = tid; e < elems; e += kVariantThreads) {
        const int phi = e / T, i = e - phi * T;
        lpfb[phi * TP + i] = g0[e];
    }
}

// The bank tiled kernels: a tile is (channel, run of tile_out outputs), the tiles are ordered channel-major and workgroup b owns
// ONE contiguous run [begin, end) of that order, so it reloads a channel's bank only when its run crosses into the next channel.
struct TileRun { long long begin, end; };
__device__ __forceinline__ TileRun tile_run(long long total_tiles)
{
    const long long per = total_tiles / gridDim.x, extra = total_tiles - per * gridDim.x;
    const long long b = blockIdx.x;
    const long long t_begin = b * per + (b < extra ? b : extra);
    return TileRun{t_begin, t_begin + per + (b < extra ? 1 : 0)};
}
struct BankTile { int ch; long long k0, klast; };     // channel, first and last output of a tile
template <bool SCALAR_CH = false>                     // the channel is uniform over the workgroup: true says so to the compiler
__device__ __forceinline__ BankTile bank_tile(long long tile, const ArbTileArgs &ta, long long n_out)
{
    int ch = static_cast<int>(tile / ta.tiles_per_channel);
    if constexpr (SCALAR_CH) ch = __builtin_amdgcn_readfirstlane(ch);
    const long long tau = tile - static_cast<long long>(ch) * ta.tiles_per_channel;
    const long long k0 = tau * ta.tile_out;
    return BankTile{ch, k0, (k0 + ta.tile_out < n_out ? k0 + ta.tile_out : n_out) - 1};
}

// FIRArbitrary / FIRFarrow tiles: the contiguous [history ; x] run between the tile's first and last n_idx (the schedule is
// non-decreasing in k: x[n_idx[k0] - T ... n_idx[klast])) is read from the schedule in the kernel, so device-planned calls are served
// too; a tile whose run is longer than the planned span (max_span: the plan goes by the rate and by what LDS holds -- a heavily
// decimating rate) is not staged: it reads its windows from global memory.
struct TileSpan { long long n_lo, o, span; bool staged; };    // o: 0-based x index of LDS sample 0 (>= -H); staged: uniform over the workgroup
__device__ __forceinline__ TileSpan tile_span(const int *n_idx, long long k0, long long klast, int T, int max_span)
{
    const long long n_lo = n_idx[k0], n_hi = n_idx[klast];
    const long long span = n_hi - n_lo + T;
    return TileSpan{n_lo, n_lo - T, span, span <= max_span};
}

// the host planned the call: its end state into the filter's record
__device__ __forceinline__ void file_end_state(const PolyArgs &a)
{
    a.rec->phiIdx = a.phi_end; a.rec->inputDeficit = a.d_end; a.rec->n_written = a.n_out; a.rec->calls += 1;
}
// rational family: 1-based index of the newest sample of output k, and its phase
__device__ __forceinline__ long long newest_of(const PolyArgs &a, long long k, int *phi)
{
    const long long u = a.u0 + k * a.M;
    const long long q = u / a.L;
    *phi = static_cast<int>(u - q * a.L);
    return a.d0 + q;
}
// FIRArbitrary: the schedule's accumulator -> 0-based column 𝜙Idx - 1 and α (src/Filters.jl:671-672)
__device__ __forceinline__ int arb_phase(double pacc, double *alpha)
{
    const double phif = __builtin_floor(pacc);
    *alpha = pacc - phif;
    return static_cast<int>(phif) - 1;
}

// FIRArbitrary, a tile that is not staged: both dots of one output over a window in global memory (x from index 0, below that
// he[index], he = the end of the channel's history); the taps still come from LDS
template <typename A>
__device__ __forceinline__ void arb_dots_global(const typename A::Tap *tp, const typename A::Tap *dp, const typename A::Sample *__restrict__ xc,
                                                const typename A::Sample *__restrict__ he, long long base, int T, typename A::Sum &lo, typename A::Sum &up)
{
    typename A::Sample v = base >= 0 ? xc[base] : he[base];
    lo = A::first(tp[0], v);
    up = A::first(dp[0], v);
    for (int i = 1; i < T; ++i) {
        const long long xi = base + i;
        v = xi >= 0 ? xc[xi] : he[xi];
        lo = A::step(lo, tp[i], v);
        up = A::step(up, dp[i], v);
    }
}

// ---- bodies that are one kernel under two algebras (A) --------------------------------------------------------------------------

// Rational family, one thread per output, any (L, M, T, hLen): poly_generic_kernel under algebra A; BANK: channel c reads bank c
// of a.taps, [nch][Nphi][T] (the pointer is offset inside the channel loop), else the one bank (hoisted).  Serves host-planned
// calls (one lane files the end state) and device-planned ones (a.dyn: asynchronous, captured, chunked, cascaded and ring calls).
template <typename A, bool BANK>
__device__ __forceinline__ void poly_variant_generic_body(PolyArgs a)
{
    using Sample = typename A::Sample;
    using Tap = typename A::Tap;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a.dyn) { a.n_out = a.dyn->n_out; a.u0 = a.dyn->u0; a.d0 = a.dyn->d0; }
    else if (a.rec && k == 0 && blockIdx.y == 0) file_end_state(a);
    if (k >= a.n_out) return;
    int phi;
    const long long n = newest_of(a, k, &phi);
    const long long base = n - a.T;            // 0-based index of the oldest sample
    const long long bank = static_cast<long long>(a.L) * a.T;
    const Tap *const shared = static_cast<const Tap *>(a.taps) + static_cast<long long>(phi) * a.T;
    for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
        const Tap *__restrict__ tp = shared;
        if constexpr (BANK) tp = static_cast<const Tap *>(a.taps) + static_cast<long long>(ch) * bank + static_cast<long long>(phi) * a.T;
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
        typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
        typename A::Sum acc = A::first(tp[0], sample(base));
        if (n < a.zero_start_below) acc = A::zero_start(acc);
        for (int i = 1; i < a.T; ++i) acc = A::step(acc, tp[i], sample(base + i));
        A::store(yc, k, acc);
    }
}

// Rational family, per-channel taps, persistent workgroups in the channel-major tile order (tile_run): the workgroup holds one
// channel's bank in LDS (column pitch T + 1: lanes of different phases read different LDS banks), the [history ; x] window of a tile is
// staged through LDS, each lane owns one output.  No workgroup waits for another.  Host-planned calls only (the tiling follows the count).
template <typename A>
__device__ __forceinline__ void poly_variant_bank_tiled_body(PolyArgs a, ArbTileArgs ta)
{
    using Sample = typename A::Sample;
    using Tap = typename A::Tap;
    extern __shared__ __attribute__((aligned(16))) unsigned char variant_smem[];
    Tap *const lpfb = reinterpret_cast<Tap *>(variant_smem);
    Sample *const lx = reinterpret_cast<Sample *>(variant_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    if (a.rec && tid == 0 && blockIdx.x == 0) file_end_state(a);
    const TileRun run = tile_run(ta.total_tiles);
    const int bank_elems = a.L * T;
    int ch_in_lds = -1;

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile(tile, ta, a.n_out);
        const int ch = t.ch;
        int phi_unused;
        const long long n_lo = newest_of(a, t.k0, &phi_unused), n_hi = newest_of(a, t.klast, &phi_unused);
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (may be < 0)
        const int span = static_cast<int>(n_hi - n_lo) + T;                             // <= ta.max_span (plan_variant_poly_tiled: span_of)

        __syncthreads();   // the previous tile's reads of bank and window are done
        if (ch != ch_in_lds) {   // (uniform over the workgroup) channel ch's bank -> LDS
            bank_to_lds(lpfb, static_cast<const Tap *>(a.taps) + static_cast<long long>(ch) * bank_elems, bank_elems, T, TP, tid);
            ch_in_lds = ch;
        }
        stage_window(lx, static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride,
                     static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H, o, span, a.x_len, a.H, tid);
        __syncthreads();

        typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        for (long long k = t.k0 + tid; k <= t.klast; k += kVariantThreads) {
            int phi;
            const long long n = newest_of(a, k, &phi);
            const Tap *tp = lpfb + phi * TP;
            const Sample *wp = lx + (n - n_lo);             // oldest sample of this output's window
            typename A::Sum acc = A::first(tp[0], wp[0]);
            if (n < a.zero_start_below) acc = A::zero_start(acc);
#pragma unroll 4
            for (int i = 1; i < T; ++i) acc = A::step(acc, tp[i], wp[i]);
            A::store(yc, k, acc);
        }
    }
}

// FIRArbitrary, one thread per output, any (Nphi, T, hLen, rate): arb_generic_kernel under algebra A -- both dots over one window,
// no start-from-zero seam (support.jl:16-31); BANK: channel c reads bank c of a.taps and a.dtaps, [nch][Nphi][T].  Serves every path:
// device-planned calls (a.dyn), host-scheduled calls, the pieces of a split call; takes the ShiftFold epilogue (so no early return).
template <typename A, bool BANK>
__device__ __forceinline__ void arb_variant_generic_body(ArbArgs a, const long long k)     // k: the lane's output
{
    using Sample = typename A::Sample;
    using Tap = typename A::Tap;
    if (a.dyn) a.n_out = a.dyn->n_out;
    if (k < a.n_out) {
        const long long n = a.n_idx[k];
        double alpha;
        const int phi = arb_phase(a.acc[k], &alpha);
        const long long bank = static_cast<long long>(a.Nphi) * a.T;
        const long long col = static_cast<long long>(phi) * a.T;
        const long long base = n - a.T;             // 0-based index of the oldest sample (>= -H: n >= 1)
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            const Tap *__restrict__ tp = static_cast<const Tap *>(a.taps) + col;
            const Tap *__restrict__ dp = static_cast<const Tap *>(a.dtaps) + col;
            if constexpr (BANK) {
                tp = static_cast<const Tap *>(a.taps) + static_cast<long long>(ch) * bank + col;
                dp = static_cast<const Tap *>(a.dtaps) + static_cast<long long>(ch) * bank + col;
            }
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
            auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
            Sample v = sample(base);
            typename A::Sum lo = A::first(tp[0], v);
            typename A::Sum up = A::first(dp[0], v);
            for (int i = 1; i < a.T; ++i) {
                v = sample(base + i);
                lo = A::step(lo, tp[i], v);
                up = A::step(up, dp[i], v);
            }
            A::store(yc, k, A::arb_combine(lo, up, alpha));
        }
    }
    dev::shiftin_by_last_workgroup<typename A::Tx, A::NC>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// FIRArbitrary, per-channel taps, persistent workgroups in the channel-major tile order (tile_run): arb_bank_tiled_kernel's body under
// algebra A.  arb_bank_ctaps_tiled_kernel (complex taps) is a wrapper of it; arb_bank_tiled_kernel (real taps) keeps its own copy in
// kernels_bank_arb.hip: as a wrapper of this body it measured 0.1 % slower than the parent's two runs at 64 ch x 1e7 Float64 in both of
// its runs (profiles/r08/arb_bank_ctaps.txt), which is the condition under which it was to stay as it is.  A tile is (channel, run of tile_out = 256 outputs); the workgroup
// holds one channel's pfb and dpfb in LDS as A::Tap (column pitch T + 1: lanes of different phases read different LDS banks; a pair
// is aligned to its size, so a tap is one LDS read) and reloads them only when its run crosses into the next channel.  The tile's run
// of samples is staged through LDS (tile_span); a tile whose run exceeds the planned span reads its windows from global memory.  The
// count and the tiling follow the call record when a.dyn is set (tiles_take_dyn with nch groups), so every workgroup's run is computed
// from the device-side count.  No workgroup communicates with or waits for another; ends with the ShiftFold epilogue.
template <typename A>
__device__ __forceinline__ void arb_variant_bank_tiled_body(ArbArgs a, ArbTileArgs ta)
{
    using Sample = typename A::Sample;
    using Tap = typename A::Tap;
    extern __shared__ __attribute__((aligned(16))) unsigned char variant_smem[];
    Tap *const lpfb = reinterpret_cast<Tap *>(variant_smem);
    Tap *const ldpfb = lpfb + ta.bank_elems;
    Sample *const lx = reinterpret_cast<Sample *>(variant_smem + ta.x_offset_bytes);

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
            const Tap *__restrict__ g0 = static_cast<const Tap *>(a.taps) + static_cast<long long>(ch) * bank_elems;
            const Tap *__restrict__ g1 = static_cast<const Tap *>(a.dtaps) + static_cast<long long>(ch) * bank_elems;
            for (int e = tid; e < bank_elems; e += kVariantThreads) {
                const int phi = e / T, i = e - phi * T;
                lpfb[phi * TP + i] = g0[e];
                ldpfb[phi * TP + i] = g1[e];
            }
            ch_in_lds = ch;
        }
        if (w.staged) stage_window(lx, xc, hc, w.o, static_cast<int>(w.span), a.x_len, a.H, tid);
        __syncthreads();

        typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        for (long long k = t.k0 + tid; k <= t.klast; k += kVariantThreads) {
            const long long n = a.n_idx[k];
            double alpha;
            const int phi = arb_phase(a.acc[k], &alpha);
            const Tap *tp = lpfb + phi * TP;
            const Tap *dp = ldpfb + phi * TP;
            typename A::Sum lo, up;
            if (w.staged) {
                const Sample *wp = lx + (n - w.n_lo);             // oldest sample of this output's window
                const Tap t0 = tp[0], d0 = dp[0];
                const Sample v0 = wp[0];
                lo = A::first(t0, v0);
                up = A::first(d0, v0);
#pragma unroll 4
                for (int i = 1; i < T; ++i) {
                    const Tap ti = tp[i], di = dp[i];
                    const Sample v = wp[i];
                    lo = A::step(lo, ti, v);
                    up = A::step(up, di, v);
                }
            } else arb_dots_global<A>(tp, dp, xc, hc + a.H, n - T, T, lo, up);
            A::store(yc, k, A::arb_combine(lo, up, alpha));
        }
    }
    dev::shiftin_by_last_workgroup<typename A::Tx, A::NC>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// FIRFarrow, per-channel taps, one thread per output, any (T, polyorder, rate): farrow_kernel with bank ch of a.pnfb,
// [nch][T][polyorder+1] coefficients of A::kCoefScalars Float64 each.  A tap belongs to one (channel, output) and feeds exactly one
// product: it is evaluated in the inner loop (A::farrow_tap), used and dropped.  The coefficient address is the same for every lane of a
// wave (the channel is uniform per block, i and j are loop counters): scalar loads, the coefficients reach the Float64 adds as scalar
// operands.  blockIdx.y strides the channels.  Serves every path: device-planned calls (a.dyn), host-scheduled calls, the pieces of a
// split call (seam_below == 0 on continuation pieces) and captured calls.  No dynamic LDS; ends with the ShiftFold epilogue.
// farrow_bank_ctaps_generic_kernel (complex taps) is a wrapper of it; farrow_bank_generic_kernel (real taps) keeps its own copy in
// kernels_bank_farrow.hip, with farrow_coef_t and kFarrowBankUnrolledP restated in its anonymous namespace: as a wrapper of this body its
// twelve code objects did not keep their instructions, which (or a timing run that was not made) was the condition for merging them
// (DESIGN.md 5.16).  k: the lane's output, computed in the kernel (there blockDim.x is one scalar load).
template <typename A>
__device__ __forceinline__ void farrow_variant_bank_generic_body(FarrowArgs a, const long long k)
{
    using Sample = typename A::Sample;
    if (a.dyn) a.n_out = a.dyn->n_out;              // a device-planned call: the count the schedule's FINISH kernel left
    if (k < a.n_out) {                               // (no early return: every thread takes part in the history epilogue below)
        const long long n = a.n_idx[k];
        const double phase = a.acc[k];
        const int P = a.polyorder, T = a.T;
        const bool tap_f32 = a.tap_f32 != 0;
        const long long base = n - T;               // 0-based index of the oldest sample (>= -H: n >= 1)
        const bool seam = n < a.seam_below;         // kernel.xIdx < kernel.tapsPer𝜙, Filters.jl:818 (never in a piece that continues a call)
        const int poly = (P + 1) * A::kCoefScalars;  // Float64 scalars of one tap's polynomial
        auto channels = [&]<int PP>() {
            for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
                farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + static_cast<long long>(ch) * T * poly;
                const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
                const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
                typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
                auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
                const Sample v0 = sample(base);
                typename A::Sum acc = A::first(A::template farrow_tap<PP>(pc, P, phase, tap_f32), v0);
                if (seam) acc = A::zero_start(acc);
                for (int i = 1; i < T; ++i) {
                    const Sample v = sample(base + i);
                    acc = A::step(acc, A::template farrow_tap<PP>(pc + i * poly, P, phase, tap_f32), v);
                }
                A::store(yc, k, acc);
            }
        };
        if (P == kFarrowBankUnrolledP) channels.template operator()<kFarrowBankUnrolledP>();
        else channels.template operator()<-1>();
    }
    dev::shiftin_by_last_workgroup<typename A::Tx, A::NC>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// ---- host side: the two launch shapes --------------------------------------------------------------------------------------------

// One lane per output: blockIdx.x covers the outputs (one block for a device-planned call of unknown count), blockIdx.y strides
// the channels.  `pick` returns the kernel for <TX, R, NCX>.  An empty host-planned call launches nothing.
template <typename Args, typename F>
hipError_t launch_lane_per_output(const TypeKey &tk, const Args &a, hipStream_t s, const char *name, const char **kname, F &&pick)
{
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    const long long bx = a.n_out > 0 ? (a.n_out + kVariantThreads - 1) / kVariantThreads : 1;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = name;
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(pick.template operator()<TX, R, NCX>(), grid, dim3(kVariantThreads), 0, s, a);
        return hipGetLastError();
    });
}

// Persistent workgroups: as many as the chip holds (persistent_grid).  The bank kernels clamp that to the tile count and take a test's
// override (MRHIP_*_GRID): a CAP on the grid (rational family: one workgroup crosses channel boundaries) or a REPLACEMENT of it
// (FIRArbitrary, FIRFarrow: also more workgroups than tiles); the complex-tap kernels (tile += gridDim.x) take the grid as it is.
enum class GridOverride { none, cap, replace };
template <typename K, typename Args>
hipError_t launch_persistent(K kfn, const Args &a, const ArbTileArgs &ta, size_t lds, hipStream_t s, int num_cus,
                             GridOverride how = GridOverride::none, int value = 0)
{
    const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kVariantThreads, lds, num_cus, ta.total_tiles);
    if (pg.err != hipSuccess) return pg.err;
    long long g = pg.grid;
    if (how != GridOverride::none) {
        g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
        if (value > 0) g = how == GridOverride::cap ? std::min<long long>(g, value) : std::min<long long>(value, 65535);
    }
    launch_kernel(kfn, dim3(static_cast<unsigned>(g)), dim3(kVariantThreads), lds, s, a, ta);
    return hipGetLastError();
}

}  // namespace mrhip
