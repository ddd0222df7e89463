// kernels_rates_farrow.hip -- FIRFarrow (src/Filters.jl:123-147, 764-839) with PER-CHANNEL RATES, over one polynomial bank or a
// BANK PER CHANNEL.
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
// lane (farrow_rates_round, farrow_rates_horner, farrow_rates_dots) are stated once below.
//
// A BANK PER CHANNEL (BANK, the kernels' last template argument): the general case of the reference's model for a continuously variable
// rate, N FIRFilter(h_c, rate_c, N𝜙, polyorder) objects with taps and rate both differing per channel (Doppler and clock trackers that
// carry a per-emitter matched pulse or a per-receiver equaliser).  A filter on which mrhip_set_channel_taps_farrow or
// mrhip_set_channel_pnfb was called holds nch polynomial banks, [nch][T][polyorder+1] Float64, in the place of the one shared bank
// (include/multirate_hip.h, "Per-channel taps with per-channel rates for FIRFarrow"), and TypeKey::bank is set; everything else of a
// call is as above, and channel c is bit for bit mrhip_create_farrow_pnfb(bank_c, rates[c], ..., nch = 1) fed x_c.  The kernels are ONE
// text for both: BANK moves the first coefficient to bank ch.  The coefficients stay scalar operands: in the universal kernel the
// channel is uniform per workgroup (blockIdx.y strides the channels), in the multi kernel a tile is one channel, so the bank base
// pnfb + ch*T*(P+1) is uniform over the workgroup either way.  rates_key is the one place that reads TypeKey::bank on the launch side.
//
// Both kernels end with the ShiftFold epilogue (the history depends on neither the rate nor the taps), with no return in front of it.
// No LDS, no barrier; no workgroup waits for another.
#include "rates_arb.h"
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// the evaluated tap, stored into currentTaps::Vector{Th} (one rounding to the tap type), widened exactly to R
template <typename R>
__device__ __forceinline__ R farrow_rates_round(const double v, const bool tap_f32)
{
    return tap_f32 ? static_cast<R>(static_cast<float>(v)) : static_cast<R>(v);
}

// OPL Horner chains of ONE polynomial side by side, each at its own phase: the P+1 coefficients are loaded once as scalars and feed all
// the chains, which are independent, so they interleave and cover each other's Float64 latency.  Per chain the statement of
// farrow_bank_horner (variant_device.h): t = 𝜙*v; v = coef + t, the product and the sum each rounded once, never fused.  PP >= 0: the
// polyorder at compile time, the loads issued together and waited for once; PP < 0: any polyorder, one load per Horner step.
template <int PP, int OPL>
__device__ __forceinline__ void farrow_rates_horner(farrow_coef_t c, const int P, const double (&phase)[OPL], double (&v)[OPL])
{
    if constexpr (PP >= 0) {
        double cj[PP + 1];
#pragma unroll
        for (int e = 0; e <= PP; ++e) cj[e] = c[e];
#pragma unroll
        for (int q = 0; q < OPL; ++q) v[q] = cj[PP];
#pragma unroll
        for (int j = PP - 1; j >= 0; --j) {
#pragma unroll
            for (int q = 0; q < OPL; ++q) {
                const double t = phase[q] * v[q];
                v[q] = cj[j] + t;
            }
        }
    } else {
        const double top = c[P];
#pragma unroll
        for (int q = 0; q < OPL; ++q) v[q] = top;
        for (int j = P - 1; j >= 0; --j) {
            const double cj = c[j];
#pragma unroll
            for (int q = 0; q < OPL; ++q) {
                const double t = phase[q] * v[q];
                v[q] = cj + t;
            }
        }
    }
}

// The OPL dots of one lane: per tap ONE evaluation of the coefficients' scalar loads, OPL Horner chains, OPL multiply-adds; sample xi of
// a window comes from x (xi >= 0) or from the end of the history (he[xi], xi < 0).  The first `live` slots are stored.  pc: the first
// coefficient of the polynomial bank the lane's channel reads, [T][P+1].
template <typename A, int PP, int OPL>
__device__ __forceinline__ void farrow_rates_dots(farrow_coef_t pc, const int P, const int T, const bool tap_f32, const double (&phase)[OPL],
                                                  const long long (&base)[OPL], const bool (&seam)[OPL],
                                                  const typename A::Sample *__restrict__ xc, const typename A::Sample *__restrict__ he,
                                                  typename A::Out *__restrict__ yc, const long long k_first, const int live)
{
    using R = typename A::Tap;
    typename A::Sum acc[OPL];
    double v[OPL];
    farrow_rates_horner<PP, OPL>(pc, P, phase, v);
#pragma unroll
    for (int j = 0; j < OPL; ++j) {
        const long long xi = base[j];
        acc[j] = A::first(farrow_rates_round<R>(v[j], tap_f32), xi >= 0 ? xc[xi] : he[xi]);
        if (seam[j]) acc[j] = A::zero_start(acc[j]);
    }
    for (int i = 1; i < T; ++i) {
        farrow_rates_horner<PP, OPL>(pc + i * (P + 1), P, phase, v);
#pragma unroll
        for (int j = 0; j < OPL; ++j) {
            const long long xi = base[j] + i;
            acc[j] = A::step(acc[j], farrow_rates_round<R>(v[j], tap_f32), xi >= 0 ? xc[xi] : he[xi]);
        }
    }
#pragma unroll
    for (int j = 0; j < OPL; ++j)
        if (j < live) A::store(yc, k_first + j * kVariantThreads, acc[j]);
}

// One lane per (channel, output), any (T, polyorder, rates): farrow_bank_generic_kernel's statement with per-channel slices of the
// schedule, over the ONE bank or (BANK) the bank of the lane's channel.  blockIdx.x covers the outputs up to the call's bound,
// blockIdx.y strides the channels; the channel's count and its bank are uniform over the workgroup.  The Horner chain:
// farrow_bank_horner<PP, 1> (variant_device.h).
template <typename TX, typename R, int NCX, bool FUSED, bool BANK>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_generic_kernel(FarrowArgs a, RatesArgs r)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    const long long bank_elems = BANK ? static_cast<long long>(T) * (P + 1) : 0;      // (read under BANK only; see DESIGN.md 5.14 on the 0)
    farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb));
    auto channels = [&]<int PP>() {
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            if (k >= r.rec[ch].count) continue;
            if constexpr (BANK) pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + ch * bank_elems;   // bank ch
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
// item 13, and has not been measured ahead here).  BANK: a tile is ONE channel, so its bank base is taken per tile, uniform over the
// workgroup, and one set of scalar loads per tap still feeds the lane's OPL Horner chains (farrow_rates_dots).
template <typename TX, typename R, int NCX, bool FUSED, int OPL, bool BANK>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_multi_kernel(FarrowArgs a, RatesArgs r, ArbTileArgs ta)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const int tid = threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    const long long bank_elems = BANK ? static_cast<long long>(T) * (P + 1) : 0;      // (read under BANK only; see DESIGN.md 5.14 on the 0)
    farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb));
    const TileRun run = tile_run(ta.total_tiles);

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile<true>(tile, ta, a.n_out);
        const int ch = t.ch;
        const long long count = r.rec[ch].count;
        if (t.k0 >= count) continue;     // (uniform over the workgroup) a tile at or behind the channel's count
        const int live = farrow_rates_live_slots(t.k0, tid, count);
        if (live == 0) continue;         // (no barrier in this kernel: a lane may leave a tile on its own)
        if constexpr (BANK) pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + ch * bank_elems;       // bank ch
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

template <typename TX, typename R, int NCX, bool BANK>
auto farrow_rates_multi_fn(bool fused)
{
    return fused ? farrow_rates_multi_kernel<TX, R, NCX, true, kFarrowRatesOPL, BANK> : farrow_rates_multi_kernel<TX, R, NCX, false, kFarrowRatesOPL, BANK>;
}

}  // namespace

// TypeKey::bank is read HERE and nowhere else in this unit: it chooses the kernels' BANK argument (dispatch_variant_flag), the names
// mrhip_last_kernel_name reports (without a kernel suffix: include/multirate_hip.h at mrhip_last_kernel_name) and the environment switches
// together.  (MRHIP_ENV_INT caches per call site behind a literal name: two sites a switch.)
static RatesKey rates_key(const TypeKey &tk)
{
    return RatesKey{tk.bank, tk.bank ? "farrow_rates_bank_generic" : "farrow_rates_generic", tk.bank ? "farrow_rates_bank_multi" : "farrow_rates_multi",
                    tk.bank ? MRHIP_ENV_INT("MRHIP_FARROW_RATES_BANK_MULTI", -1) : MRHIP_ENV_INT("MRHIP_FARROW_RATES_MULTI", -1),
                    tk.bank ? MRHIP_ENV_INT("MRHIP_FARROW_RATES_BANK_GRID", 0) : MRHIP_ENV_INT("MRHIP_FARROW_RATES_GRID", 0)};
}

hipError_t launch_farrow_rates_generic(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, hipStream_t s, const char **kname)
{
    if (tk.complex_h || a.dyn) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    const long long bx = (a.n_out + kVariantThreads - 1) / kVariantThreads;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    const RatesKey key = rates_key(tk);
    *kname = key.generic;
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>() -> hipError_t {
        launch_kernel(fused ? farrow_rates_generic_kernel<TX, R, NCX, true, BANK> : farrow_rates_generic_kernel<TX, R, NCX, false, BANK>, grid,
                      dim3(kVariantThreads), 0, s, a, r);
        return hipGetLastError();
    });
}

bool plan_farrow_rates_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, ArbTileArgs *out)
{
    return plan_farrow_rates_multi(tk, a, num_cus, rates_key(tk).tiled_mode, out);
}

hipError_t prepare_farrow_rates_multi(const TypeKey &tk, bool fused, const ArbTileArgs &ta, int num_cus, long long *grid)
{
    if (tk.complex_h) return hipErrorInvalidValue;
    const RatesKey key = rates_key(tk);
    return dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>() -> hipError_t {
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(farrow_rates_multi_fn<TX, R, NCX, BANK>(fused)), kVariantThreads, 0,
                                                  num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        *grid = farrow_rates_multi_grid(ta.total_tiles, pg.grid, key.grid_fixed);
        return hipSuccess;
    });
}

hipError_t launch_farrow_rates_multi(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, const ArbTileArgs &ta,
                                     long long grid, hipStream_t s, const char **kname)
{
    if (tk.complex_h || a.dyn || grid < 1 || ta.tile_out != static_cast<long long>(kFarrowRatesOPL) * kVariantThreads)
        return hipErrorInvalidValue;
    const RatesKey key = rates_key(tk);
    *kname = key.tiled;
    return dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>() -> hipError_t {
        launch_kernel(farrow_rates_multi_fn<TX, R, NCX, BANK>(fused), dim3(static_cast<unsigned>(grid)), dim3(kVariantThreads), 0, s, a, r, ta);
        return hipGetLastError();
    });
}

}  // namespace mrhip
