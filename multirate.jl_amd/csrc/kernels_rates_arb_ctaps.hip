// kernels_rates_arb_ctaps.hip -- FIRArbitrary (src/Filters.jl:91-117, 663-742) with PER-CHANNEL RATES and COMPLEX PER-CHANNEL TAPS.
//
// The general case of the reference's model with a complex prototype: N FIRFilter(h_c::Vector{Complex}, rate_c, N𝜙) objects, taps and
// rate both differing per channel -- per-emitter Doppler correction is both at once, a time scale (a rate per channel) and a carrier
// offset (a prototype rotated to the channel's own frequency).  A filter of mrhip_create_arbitrary_rates on which
// mrhip_set_channel_ctaps or mrhip_set_channel_ctaps_device was called holds nch pfb and nch dpfb banks of (re, im) pairs of R,
// [nch][Nphi][T] (include/multirate_hip.h, "Complex per-channel taps with per-channel rates for FIRArbitrary"), and TypeKey::complex_h
// and ::bank are both set.  A call is the two launches of kernels_rates_arb.hip: its schedule kernel (the walk does not depend on the
// taps), then one of the two filter kernels below, a lane per (channel, output): n and acc from the channel's slice, the count from the
// channel's record.
//
//   arb_rates_ctaps_generic_kernel: any (Nphi, T, hLen, rates); the column of bank ch is read from global memory.
//   arb_rates_ctaps_tiled_kernel: persistent workgroups over the channel-major tile order, one channel's two banks in LDS, the tile's
//      run of samples staged through LDS (behind plan_arb_rates_ctaps_tiled, host_logic.cpp).
//   rates_cbank_build_kernel: the nch pairs of banks from rows of complex taps in DEVICE memory (mrhip_set_channel_ctaps_device).
//
// These are the statements of arb_rates_generic_kernel and arb_rates_tiled_kernel with BANK true, and of rates_bank_build_kernel, under
// the complex tap algebra (ComplexTaps, variant_device.h: the arithmetic of ctaps_device.h).  They stand in a unit of their own because
// kernels_rates_arb.hip is one text over RealTaps whose instantiations are counted; one text over the algebra for both units is a later
// refactor.
//
// Arithmetic (include/multirate_hip.h, "Complex taps"): both dots over one window, oldest sample first, the first product initialises
// the sum, every multiply, add and subtract rounded separately in R, the combine per component in Float64 and rounded to R; no FUSED
// form.  So channel c is bit for bit mrhip_create_arbitrary_ctaps(h_c, rates[c], N𝜙, nch = 1) fed x_c.  This file is compiled with
// -ffp-contract=off.  Both filter kernels end with the ShiftFold epilogue (the history depends on neither the rate nor the taps).  No
// workgroup waits for another; plain HIP.
#include "rates_arb.h"
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// One lane per (channel, output), any (Nphi, T, hLen, rates): blockIdx.x covers the outputs up to the call's bound, blockIdx.y strides
// the channels; the channel's count is uniform over the workgroup.  tp / dp start at column phi of bank ch.
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void arb_rates_ctaps_generic_kernel(ArbArgs a, RatesArgs r)
{
    using A = ComplexTaps<TX, R, NCX>;
    using Sample = typename A::Sample;
    using Tap = typename A::Tap;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const long long bank_elems = static_cast<long long>(a.Nphi) * a.T;
    for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
        if (k >= r.rec[ch].count) continue;
        const long long n = a.n_idx[static_cast<long long>(ch) * r.slice + k];
        double alpha;
        const int phi = arb_phase(a.acc[static_cast<long long>(ch) * r.slice + k], &alpha);
        const long long col = ch * bank_elems + static_cast<long long>(phi) * a.T;      // column phi of bank ch
        const long long base = n - a.T;             // 0-based index of the oldest sample (>= -H: n >= 1)
        const Tap *__restrict__ tp = static_cast<const Tap *>(a.taps) + col;
        const Tap *__restrict__ dp = static_cast<const Tap *>(a.dtaps) + col;
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
    if (r.x_lens) dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{});
    else dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// Persistent workgroups in the channel-major tile order (tile_run, variant_device.h).  A tile is (channel, run of tile_out = 256
// outputs); the tiling goes by the call's bound.  A tile at or behind its channel's count is skipped BEFORE any barrier (the skip is
// uniform over the workgroup).  The workgroup holds ONE channel's pfb and dpfb in LDS as (re, im) pairs (column pitch T + 1 pairs: lanes
// of different phases read different LDS banks; a pair is aligned to its size -- the banks start at the 16-byte aligned base and every
// offset is a whole number of pairs -- so a Float32 pair is one 8-byte and a Float64 pair one 16-byte LDS read), reloaded only when a
// live tile belongs to another channel than the one in LDS (ch_in_lds): a channel without outputs in this call never has its banks
// loaded.  The tile's run of samples is read from the channel's own slice of the schedule (tile_span) -- so it follows that channel's
// rate -- and staged through LDS up to the channel's own length (stage_window); a tile whose run is longer than the planned span (a
// channel that decimates heavily) reads its windows from global memory (arb_dots_global), its taps still from LDS.
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void arb_rates_ctaps_tiled_kernel(ArbArgs a, RatesArgs r, ArbTileArgs ta)
{
    using A = ComplexTaps<TX, R, NCX>;
    using Sample = typename A::Sample;
    using Tap = typename A::Tap;
    extern __shared__ __attribute__((aligned(16))) unsigned char rates_arb_ctaps_smem[];
    Tap *const lpfb = reinterpret_cast<Tap *>(rates_arb_ctaps_smem);
    Tap *const ldpfb = lpfb + ta.bank_elems;
    Sample *const lx = reinterpret_cast<Sample *>(rates_arb_ctaps_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    const TileRun run = tile_run(ta.total_tiles);
    const int bank_elems = a.Nphi * T;
    int ch_in_lds = -1;

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile<true>(tile, ta, a.n_out);
        const int ch = t.ch;
        const long long count = r.rec[ch].count;
        if (t.k0 >= count) continue;     // (uniform over the workgroup) a tile at or behind the channel's count: no barrier, no banks
        const long long len = rates_channel_len(r.x_lens, a.x_len, ch);      // (uniform too: the window is staged up to the channel's own end)
        const long long klast = (t.klast < count ? t.klast : count - 1);
        const int *__restrict__ nc = a.n_idx + static_cast<long long>(ch) * r.slice;
        const double *__restrict__ ac = a.acc + static_cast<long long>(ch) * r.slice;
        const TileSpan w = tile_span(nc, t.k0, klast, T, ta.max_span);
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;

        __syncthreads();   // the previous live tile's reads of the window and of the banks are done
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
        if (w.staged) stage_window(lx, xc, hc, w.o, static_cast<int>(w.span), len, a.H, tid);
        __syncthreads();

        typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        for (long long k = t.k0 + tid; k <= klast; k += kVariantThreads) {
            const long long n = nc[k];
            double alpha;
            const int phi = arb_phase(ac[k], &alpha);
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
    if (r.x_lens) dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{});
    else dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// rates_bank_build_kernel over pairs: the pfb and dpfb banks of every channel from the channel's row of (re, im) taps -- what
// create_pfb_banks and the widening of mrhip_set_channel_ctaps produce, bit for bit: the index map is rates_bank_tap_index, the values
// rates_cbank_pfb_value / rates_cbank_dpfb_value of rates_arb.h (one subtraction per component, rounded in the tap's scalar type); the
// widening TAP -> R is exact.  One workgroup per (channel, slab of kBankBuildSlab bank elements); the row goes through LDS first, with
// coalesced loads, when its hLen pairs fit kBankBuildLdsBytes, a longer row is read from global memory directly.
template <typename TAP, typename R>
__global__ __launch_bounds__(kBankBuildThreads) void rates_cbank_build_kernel(BankBuildArgs b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rates_cbuild_smem[];
    TAP *const lrow = reinterpret_cast<TAP *>(rates_cbuild_smem);
    const int tid = threadIdx.x;
    const long long bank = b.Nphi * b.T;
    const long long e0 = static_cast<long long>(blockIdx.x) * kBankBuildSlab;
    const long long e1 = e0 + kBankBuildSlab < bank ? e0 + kBankBuildSlab : bank;
    for (int ch = blockIdx.y; ch < b.nch; ch += gridDim.y) {       // (uniform over the workgroup)
        const TAP *__restrict__ h = static_cast<const TAP *>(b.h) + static_cast<long long>(ch) * b.hLen * 2;
        const TAP *src = h;
        if (b.row_in_lds) {
            __syncthreads();                                       // the previous channel's reads of the row are done
            for (long long j = tid; j < 2 * b.hLen; j += kBankBuildThreads) lrow[j] = h[j];
            __syncthreads();
            src = lrow;
        }
        CPair<R> *__restrict__ p = static_cast<CPair<R> *>(b.pfb) + static_cast<long long>(ch) * bank;
        CPair<R> *__restrict__ d = static_cast<CPair<R> *>(b.dpfb) + static_cast<long long>(ch) * bank;
        for (long long e = e0 + tid; e < e1; e += kBankBuildThreads) {
            const long long j = rates_bank_tap_index(e, b.T, b.Nphi);
            const RatesTapPair<TAP> pv = rates_cbank_pfb_value<TAP>(src, b.hLen, j);
            const RatesTapPair<TAP> dv = rates_cbank_dpfb_value<TAP>(src, b.hLen, j);
            CPair<R> po, dout;
            po.re = static_cast<R>(pv.re); po.im = static_cast<R>(pv.im);
            dout.re = static_cast<R>(dv.re); dout.im = static_cast<R>(dv.im);
            p[e] = po;
            d[e] = dout;
        }
    }
}

// the two switches, each a literal name at a site of its own (MRHIP_ENV_INT caches per call site)
int ctaps_tiled_mode() { return MRHIP_ENV_INT("MRHIP_ARB_RATES_CTAPS_TILED", -1); }
int ctaps_grid_fixed() { return MRHIP_ENV_INT("MRHIP_ARB_RATES_CTAPS_GRID", 0); }

bool ctaps_key(const TypeKey &tk) { return tk.complex_h && tk.bank; }

}  // namespace

hipError_t launch_arb_rates_ctaps_generic(const TypeKey &tk, const ArbArgs &a, const RatesArgs &r, hipStream_t s, const char **kname)
{
    if (!ctaps_key(tk) || a.dyn) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    const long long bx = (a.n_out + kVariantThreads - 1) / kVariantThreads;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "arb_rates_ctaps_generic";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(arb_rates_ctaps_generic_kernel<TX, R, NCX>, grid, dim3(kVariantThreads), 0, s, a, r);
        return hipGetLastError();
    });
}

bool plan_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_arb_rates_ctaps_tiled(tk, a, rate_min, num_cus, ctaps_tiled_mode(), out, lds);
}

hipError_t prepare_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbTileArgs &ta, size_t lds, int num_cus, long long *grid)
{
    if (!ctaps_key(tk)) return hipErrorInvalidValue;
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(arb_rates_ctaps_tiled_kernel<TX, R, NCX>), kVariantThreads, lds,
                                                  num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        long long g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
        const int grid_fixed = ctaps_grid_fixed();
        if (grid_fixed > 0) g = std::min<long long>(grid_fixed, 65535);       // (tests: also more workgroups than tiles)
        *grid = g;
        return hipSuccess;
    });
}

hipError_t launch_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, const RatesArgs &r, const ArbTileArgs &ta, size_t lds, long long grid,
                                        hipStream_t s, const char **kname)
{
    if (!ctaps_key(tk) || a.dyn || grid < 1) return hipErrorInvalidValue;
    *kname = "arb_rates_ctaps_tiled";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(arb_rates_ctaps_tiled_kernel<TX, R, NCX>, dim3(static_cast<unsigned>(grid)), dim3(kVariantThreads), lds, s, a, r, ta);
        return hipGetLastError();
    });
}

hipError_t launch_rates_cbank_build(bool tap_f64, bool r_f64, const BankBuildArgs &b, hipStream_t st)
{
    if (b.nch < 1 || b.hLen < 1 || b.T < 1 || b.Nphi < 1 || (tap_f64 && !r_f64)) return hipErrorInvalidValue;
    const long long slabs = (b.Nphi * b.T + kBankBuildSlab - 1) / kBankBuildSlab;
    if (slabs > 0x7fffffffLL) return hipErrorInvalidValue;
    BankBuildArgs a = b;
    const long long row_bytes = 2 * b.hLen * static_cast<long long>(tap_f64 ? sizeof(double) : sizeof(float));
    a.row_in_lds = row_bytes <= kBankBuildLdsBytes ? 1 : 0;
    const size_t lds = a.row_in_lds ? static_cast<size_t>(row_bytes) : 0;
    const dim3 grid(static_cast<unsigned>(slabs), static_cast<unsigned>(b.nch < 65535 ? b.nch : 65535), 1);
    auto kfn = tap_f64 ? rates_cbank_build_kernel<double, double> : r_f64 ? rates_cbank_build_kernel<float, double> : rates_cbank_build_kernel<float, float>;
    hipLaunchKernelGGL(kfn, grid, dim3(kBankBuildThreads), lds, st, a);
    return hipGetLastError();
}

}  // namespace mrhip
