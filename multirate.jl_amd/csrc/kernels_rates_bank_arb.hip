// kernels_rates_bank_arb.hip -- FIRArbitrary (src/Filters.jl:91-117, 663-742) with PER-CHANNEL RATES and PER-CHANNEL TAPS.
//
// The general case of the reference's model, N signals as N FIRFilter(h_c, rate_c, N𝜙) objects with both differing per channel (receivers
// each off its own clock AND each with its own front-end equaliser; per-emitter Doppler correction with the emitter's own matched
// pulse).  A filter of mrhip_create_arbitrary_rates on which mrhip_set_channel_taps was called holds nch pfb and nch dpfb banks,
// [nch][Nphi][T] in R, in the place of the one shared pair (include/multirate_hip.h, "Per-channel taps with per-channel rates for
// FIRArbitrary"); everything else of a call is kernels_rates_arb.hip's: the schedule kernel (one lane per channel, the serial walk of
// update()), the channels' records and slices, the ragged lengths.  Only the filter kernel differs, and api.hip (rates_call) comes here
// when TypeKey::bank is set on such a filter:
//
//   arb_rates_bank_generic_kernel  a lane per (channel, output): arb_rates_generic_kernel with tp / dp starting at bank ch
//   arb_rates_bank_tiled_kernel    persistent workgroups, ONE channel's banks in LDS, reloaded when the run crosses into another channel
//                                  (arb_bank_tiled_kernel's hand-out with arb_rates_tiled_kernel's per-channel count, span and length)
//
// Arithmetic: that of arb_generic_kernel on bank c -- both dots over one window, oldest sample first, the first product initialises the
// accumulator, no start-from-zero seam; STRICT: every multiply and add rounded separately in R, FUSED: one fma per tap; the combine in
// Float64, then rounded to R (RealTaps, variant_device.h) -- so channel c is bit for bit mrhip_create_arbitrary(h_c, rates[c], N𝜙,
// nch = 1) fed x_c.  This file is compiled with -ffp-contract=off.  Both kernels end with the ShiftFold epilogue (the history depends on
// neither the rate nor the taps).  No workgroup waits for another.
#include "rates_arb.h"
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// One lane per (channel, output), any (Nphi, T, hLen, rates): blockIdx.x covers the outputs up to the call's bound, blockIdx.y strides
// the channels; the channel's count is uniform over the workgroup.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void arb_rates_bank_generic_kernel(ArbArgs a, RatesArgs r)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const long long bank_elems = static_cast<long long>(a.Nphi) * a.T;
    for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
        if (k >= r.rec[ch].count) continue;
        const long long n = a.n_idx[static_cast<long long>(ch) * r.slice + k];
        double alpha;
        const int phi = arb_phase(a.acc[static_cast<long long>(ch) * r.slice + k], &alpha);
        const long long col = ch * bank_elems + static_cast<long long>(phi) * a.T;       // column phi of bank ch
        const long long base = n - a.T;             // 0-based index of the oldest sample (>= -H: n >= 1)
        const R *__restrict__ tp = static_cast<const R *>(a.taps) + col;
        const R *__restrict__ dp = static_cast<const R *>(a.dtaps) + col;
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
        R *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
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
// uniform over the workgroup), so a channel without outputs in this call never has its banks loaded.  The workgroup holds ONE channel's
// pfb and dpfb in LDS (column pitch T + 1: lanes of different phases read different LDS banks) and reloads them only when a live tile
// belongs to another channel than the one in LDS (ch_in_lds): the first live tile after any number of skipped ones finds its own
// channel's banks or loads them.  The tile's run of samples is read from the channel's own slice of the schedule (tile_span) and staged
// through LDS up to the channel's own length (stage_window); a tile whose run is longer than the planned span reads its windows from
// global memory (arb_dots_global), its taps still from LDS.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void arb_rates_bank_tiled_kernel(ArbArgs a, RatesArgs r, ArbTileArgs ta)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    extern __shared__ __attribute__((aligned(16))) unsigned char rates_bank_arb_smem[];
    R *const lpfb = reinterpret_cast<R *>(rates_bank_arb_smem);
    R *const ldpfb = lpfb + ta.bank_elems;
    Sample *const lx = reinterpret_cast<Sample *>(rates_bank_arb_smem + ta.x_offset_bytes);

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

        __syncthreads();   // the previous live tile's reads of the BANKS and of the window are done
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
        if (w.staged) stage_window(lx, xc, hc, w.o, static_cast<int>(w.span), len, a.H, tid);
        __syncthreads();

        R *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        for (long long k = t.k0 + tid; k <= klast; k += kVariantThreads) {
            const long long n = nc[k];
            double alpha;
            const int phi = arb_phase(ac[k], &alpha);
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
    if (r.x_lens) dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{});
    else dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

}  // namespace

// (the names mrhip_last_kernel_name reports carry no kernel suffix: include/multirate_hip.h at mrhip_last_kernel_name)
hipError_t launch_arb_rates_bank_generic(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h || a.dyn) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    const long long bx = (a.n_out + kVariantThreads - 1) / kVariantThreads;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "arb_rates_bank_generic";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(fused ? arb_rates_bank_generic_kernel<TX, R, NCX, true> : arb_rates_bank_generic_kernel<TX, R, NCX, false>, grid,
                      dim3(kVariantThreads), 0, s, a, r);
        return hipGetLastError();
    });
}

bool plan_arb_rates_bank_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_arb_rates_bank_tiled(tk, a, rate_min, num_cus, MRHIP_ENV_INT("MRHIP_ARB_RATES_BANK_TILED", -1), out, lds);
}

hipError_t prepare_arb_rates_bank_tiled(const TypeKey &tk, bool fused, const ArbTileArgs &ta, size_t lds, int num_cus, long long *grid)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_ARB_RATES_BANK_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto kfn = fused ? arb_rates_bank_tiled_kernel<TX, R, NCX, true> : arb_rates_bank_tiled_kernel<TX, R, NCX, false>;
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kVariantThreads, lds, num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        long long g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
        if (grid_fixed > 0) g = std::min<long long>(grid_fixed, 65535);       // (tests: also more workgroups than tiles)
        *grid = g;
        return hipSuccess;
    });
}

hipError_t launch_arb_rates_bank_tiled(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, const ArbTileArgs &ta, size_t lds,
                                       long long grid, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h || a.dyn || grid < 1) return hipErrorInvalidValue;
    *kname = "arb_rates_bank_tiled";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto kfn = fused ? arb_rates_bank_tiled_kernel<TX, R, NCX, true> : arb_rates_bank_tiled_kernel<TX, R, NCX, false>;
        launch_kernel(kfn, dim3(static_cast<unsigned>(grid)), dim3(kVariantThreads), lds, s, a, r, ta);
        return hipGetLastError();
    });
}

}  // namespace mrhip
