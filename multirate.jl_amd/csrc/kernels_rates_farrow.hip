// kernels_rates_farrow.hip -- FIRFarrow (src/Filters.jl:123-147, 764-839) with PER-CHANNEL RATES.
//
// In the reference N signals are N FIRFilter(h, rate_c, N𝜙, polyorder) objects, and every rate_c may differ (receivers each off its own
// clock, per-emitter Doppler time-scale correction, per-channel fractional delay -- FIRFarrow is the kernel the reference offers for a
// continuously variable rate).  mrhip_create_farrow_rates builds ONE filter whose channels share h -- so the ONE polynomial bank pnfb,
// [T][polyorder+1] Float64 -- N𝜙, polyorder, the call length and the history length, and each have their own Δ, 𝜙Idx, xIdx, inputDeficit
// and per-call output count (RateChannel, rates_arb.h).  A call is two launches on the caller's stream and nothing else:
//
//   1. rates_schedule_kernel (kernels_rates_arb.hip), one lane per channel: update() of FIRFarrow (:780-786) is FIRArbitrary's recurrence
//      on the same Float64 quantity, the short-input rule (:805-809) and the walk (:812-828) are the same statements.  Entry k of channel
//      c: the 1-based input index and the Float64 phase 𝜙Idx the output is computed at.
//   2. a filter kernel of this file: the universal one (farrow_rates_generic_kernel) or farrow_rates_multi_kernel.
//
// Per output k of channel c:   taps[i] = Th(polyval(pnfb[i], 𝜙_c,k)),   y_c,k = sum_i taps[i] * ext_c[n_c,k - T + i],   ext = [history ; x]
//
// Arithmetic (include/multirate_hip.h, "Per-channel rates for FIRFarrow"): that of farrow_kernel (kernels_generic.hip), as restated at
// the top of kernels_bank_farrow.hip -- Horner in Float64 from the highest power (t = 𝜙*v; v = coef + t, the product and the sum each
// rounded once, NEVER fused, also under FUSED), the tap rounded once to the tap type and widened exactly to R; the dot oldest sample
// first, the first product initialises the accumulator, outputs on the seam (n < T: every call of this filter starts a filt!, none
// continues one) then take R(0) + acc per component (support.jl:46); STRICT: a separately rounded multiply and add per tap, FUSED: one
// explicit fma per tap -- so channel c is bit for bit mrhip_create_farrow(h, rates[c], ..., nch = 1) fed x_c.  This file is compiled with
// -ffp-contract=off.
//
// What sets this filter apart from the Farrow bank (kernels_bank_farrow.hip): there the coefficients are uniform per CHANNEL; here pnfb is
// shared by all channels, so the coefficient address pnfb + i*(P+1) + j is uniform over the whole grid, whatever channel or output a lane
// holds.  Every coefficient is a scalar operand read through the constant address space (farrow_coef_t, variant_device.h), and ONE set
// of scalar loads can serve several outputs of a lane: the multi kernel.  The rounding of a tap, the Horner chains and the dots of a
// lane (farrow_rates_round, farrow_rates_horner, farrow_rates_dots) are stated in rates_farrow_device.h, which this unit shares with
// kernels_rates_bank_farrow.hip (a bank per channel).
// Both kernels end with the ShiftFold epilogue (the history does not depend on the rate).  No workgroup waits for another.
#include "rates_arb.h"
#include "variant_device.h"
#include "rates_farrow_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// One lane per (channel, output), any (T, polyorder, rates): farrow_bank_generic_kernel's statement with the ONE bank and per-channel
// slices of the schedule.  blockIdx.x covers the outputs up to the call's bound, blockIdx.y strides the channels; the channel's count
// is uniform over the workgroup.  The Horner chain: farrow_bank_horner<PP, 1> (variant_device.h).
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_generic_kernel(FarrowArgs a, RatesArgs r)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb));
    auto channels = [&]<int PP>() {
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            if (k >= r.rec[ch].count) continue;
            const long long n = a.n_idx[static_cast<long long>(ch) * r.slice + k];
            const double phase = a.acc[static_cast<long long>(ch) * r.slice + k];
            const long long base = n - T;               // 0-based index of the oldest sample (>= -H: n >= 1)
            const bool seam = n < a.seam_below;         // kernel.xIdx < kernel.tapsPer𝜙, Filters.jl:819
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            R *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
            auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
            auto tap = [&](int i) -> R {
                double v[1];
                farrow_bank_horner<PP, 1>(pc + i * (P + 1), P, phase, v);
                return farrow_rates_round<R>(v[0], tap_f32);
            };
            typename A::Sum acc = A::first(tap(0), sample(base));
            if (seam) acc = A::zero_start(acc);
            for (int i = 1; i < T; ++i) {
                const Sample v = sample(base + i);
                acc = A::step(acc, tap(i), v);
            }
            A::store(yc, k, acc);
        }
    };
    if (P == kFarrowBankUnrolledP) channels.template operator()<kFarrowBankUnrolledP>();
    else channels.template operator()<-1>();
    if (r.x_lens) dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{});
    else dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// Persistent workgroups in the channel-major tile order (tile_run, variant_device.h).  A tile is (channel, OPL consecutive runs of 256
// outputs); lane `tid` owns output `tid` of each run (slot j: k0 + tid + 256 j), so neighbouring lanes keep neighbouring outputs and the
// y stores stay coalesced.  The tiling goes by the call's bound; tiles at or behind the channel's count are skipped, and so are a lane's
// slots at or behind it (farrow_rates_live_slots, rates_arb.h: the live slots are the first ones).  A slot that is not live computes on
// slot 0's entry -- loads from valid addresses, no store -- so the OPL chains stay one straight-line statement.  The windows are read
// from global memory and the history: no LDS, no barrier (staging the run of samples measured worthless for the Farrow bank, DESIGN.md 9
// item 13, and has not been measured ahead here).
template <typename TX, typename R, int NCX, bool FUSED, int OPL>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_multi_kernel(FarrowArgs a, RatesArgs r, ArbTileArgs ta)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const int tid = threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb));
    const TileRun run = tile_run(ta.total_tiles);

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile<true>(tile, ta, a.n_out);
        const int ch = t.ch;
        const long long count = r.rec[ch].count;
        if (t.k0 >= count) continue;     // (uniform over the workgroup) a tile at or behind the channel's count
        const int live = farrow_rates_live_slots(t.k0, tid, count);
        if (live == 0) continue;         // (no barrier in this kernel: a lane may leave a tile on its own)
        const int *__restrict__ nc = a.n_idx + static_cast<long long>(ch) * r.slice;
        const double *__restrict__ ac = a.acc + static_cast<long long>(ch) * r.slice;
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ he = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H + a.H;   // the end of the history
        R *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        const long long k_first = t.k0 + tid;

        long long base[OPL];             // 0-based index of the oldest sample of each slot's window (>= -H: n >= 1)
        double phase[OPL];
        bool seam[OPL];
#pragma unroll
        for (int j = 0; j < OPL; ++j) {
            const long long kj = k_first + (j < live ? j : 0) * kVariantThreads;
            const long long n = nc[kj];
            phase[j] = ac[kj];
            base[j] = n - T;
            seam[j] = n < a.seam_below;  // kernel.xIdx < kernel.tapsPer𝜙, Filters.jl:819
        }
        if (P == kFarrowBankUnrolledP)
            farrow_rates_dots<A, kFarrowBankUnrolledP, OPL>(pc, P, T, tap_f32, phase, base, seam, xc, he, yc, k_first, live);
        else farrow_rates_dots<A, -1, OPL>(pc, P, T, tap_f32, phase, base, seam, xc, he, yc, k_first, live);
    }
    if (r.x_lens) dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{});
    else dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

template <typename TX, typename R, int NCX>
auto farrow_rates_multi_fn(bool fused)
{
    return fused ? farrow_rates_multi_kernel<TX, R, NCX, true, kFarrowRatesOPL> : farrow_rates_multi_kernel<TX, R, NCX, false, kFarrowRatesOPL>;
}

}  // namespace

// (the names mrhip_last_kernel_name reports carry no kernel suffix: include/multirate_hip.h at mrhip_last_kernel_name)
hipError_t launch_farrow_rates_generic(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, hipStream_t s, const char **kname)
{
    if (tk.bank || tk.complex_h || a.dyn) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    const long long bx = (a.n_out + kVariantThreads - 1) / kVariantThreads;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "farrow_rates_generic";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(fused ? farrow_rates_generic_kernel<TX, R, NCX, true> : farrow_rates_generic_kernel<TX, R, NCX, false>, grid,
                      dim3(kVariantThreads), 0, s, a, r);
        return hipGetLastError();
    });
}

bool plan_farrow_rates_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, ArbTileArgs *out)
{
    return plan_farrow_rates_multi(tk, a, num_cus, MRHIP_ENV_INT("MRHIP_FARROW_RATES_MULTI", -1), out);
}

hipError_t prepare_farrow_rates_multi(const TypeKey &tk, bool fused, const ArbTileArgs &ta, int num_cus, long long *grid)
{
    if (tk.bank || tk.complex_h) return hipErrorInvalidValue;
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_FARROW_RATES_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(farrow_rates_multi_fn<TX, R, NCX>(fused)), kVariantThreads, 0,
                                                  num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        *grid = farrow_rates_multi_grid(ta.total_tiles, pg.grid, grid_fixed);
        return hipSuccess;
    });
}

hipError_t launch_farrow_rates_multi(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, const ArbTileArgs &ta,
                                     long long grid, hipStream_t s, const char **kname)
{
    if (tk.bank || tk.complex_h || a.dyn || grid < 1 || ta.tile_out != static_cast<long long>(kFarrowRatesOPL) * kVariantThreads)
        return hipErrorInvalidValue;
    *kname = "farrow_rates_multi";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(farrow_rates_multi_fn<TX, R, NCX>(fused), dim3(static_cast<unsigned>(grid)), dim3(kVariantThreads), 0, s, a, r, ta);
        return hipGetLastError();
    });
}

}  // namespace mrhip
