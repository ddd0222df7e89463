// kernels_rates_bank_farrow.hip -- FIRFarrow (src/Filters.jl:123-147, 764-839) with PER-CHANNEL RATES and PER-CHANNEL TAPS.
//
// The general case of the reference's model for a continuously variable rate: N signals as N FIRFilter(h_c, rate_c, N𝜙, polyorder)
// objects with taps and rate both differing per channel (Doppler and clock trackers that carry a per-emitter matched pulse or a
// per-receiver equaliser).  A filter of mrhip_create_farrow_rates* on which mrhip_set_channel_taps_farrow or mrhip_set_channel_pnfb was
// called holds nch polynomial banks, [nch][T][polyorder+1] Float64, in the place of the one shared bank (include/multirate_hip.h,
// "Per-channel taps with per-channel rates for FIRFarrow"); everything else of a call is kernels_rates_farrow.hip's: the schedule kernel
// (kernels_rates_arb.hip, one lane per channel), the channels' records and slices, the ragged lengths.  Only the filter kernel differs,
// and api.hip (rates_call) comes here when TypeKey::bank is set on such a filter:
//
//   farrow_rates_bank_generic_kernel  a lane per (channel, output): farrow_rates_generic_kernel with the coefficients of bank ch
//   farrow_rates_bank_multi_kernel    four outputs a lane share each tap's scalar loads: farrow_rates_multi_kernel, the bank of the tile's channel
//
// Arithmetic: that of farrow_kernel (kernels_generic.hip) on bank c, as restated at the top of kernels_rates_farrow.hip -- Horner in
// Float64 from the highest power, the product and the sum each rounded once, NEVER fused, also under FUSED; the tap rounded once to the
// tap type and widened exactly to R; the dot oldest sample first, outputs on the seam (n < T, every call) take R(0) + acc
// (zero_start); STRICT: a separately rounded multiply and add per tap, FUSED: one explicit fma per tap (RealTaps) -- so channel c is bit
// for bit mrhip_create_farrow_pnfb(bank_c, rates[c], ..., nch = 1) fed x_c.  This file is compiled with -ffp-contract=off.
//
// The coefficients stay scalar operands: in the universal kernel the channel is uniform per workgroup (blockIdx.y strides the
// channels), in the multi kernel a tile is one channel, so the bank base pnfb + ch*T*(P+1) is uniform over the workgroup either way and
// the reads go through the constant address space (farrow_coef_t, variant_device.h).  The Horner chains and the dots are the sibling
// unit's, stated once in rates_farrow_device.h.  Both kernels end with the ShiftFold epilogue (the history depends on neither the rate
// nor the taps), with no return in front of it.  No LDS, no barrier; no workgroup waits for another.
#include "rates_arb.h"
#include "variant_device.h"
#include "rates_farrow_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// One lane per (channel, output), any (T, polyorder, rates): blockIdx.x covers the outputs up to the call's bound, blockIdx.y strides
// the channels; the channel's count and its bank are uniform over the workgroup.  The Horner chain: farrow_bank_horner<PP, 1>.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_bank_generic_kernel(FarrowArgs a, RatesArgs r)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    const long long bank_elems = static_cast<long long>(T) * (P + 1);
    auto channels = [&]<int PP>() {
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            if (k >= r.rec[ch].count) continue;
            farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + ch * bank_elems;   // bank ch
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
// outputs) and lane `tid` owns output `tid` of each run, as in farrow_rates_multi_kernel; tiles at or behind the channel's count are
// skipped, and so are a lane's slots at or behind it (farrow_rates_live_slots, rates_arb.h).  A tile is ONE channel: its bank base is
// taken per tile, uniform over the workgroup, and one set of scalar loads per tap still feeds the lane's OPL Horner chains
// (farrow_rates_dots, rates_farrow_device.h).  The windows are read from global memory and the history: no LDS, no barrier.
template <typename TX, typename R, int NCX, bool FUSED, int OPL>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_bank_multi_kernel(FarrowArgs a, RatesArgs r, ArbTileArgs ta)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const int tid = threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    const long long bank_elems = static_cast<long long>(T) * (P + 1);
    const TileRun run = tile_run(ta.total_tiles);

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile<true>(tile, ta, a.n_out);
        const int ch = t.ch;
        const long long count = r.rec[ch].count;
        if (t.k0 >= count) continue;     // (uniform over the workgroup) a tile at or behind the channel's count
        const int live = farrow_rates_live_slots(t.k0, tid, count);
        if (live == 0) continue;         // (no barrier in this kernel: a lane may leave a tile on its own)
        farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + ch * bank_elems;       // bank ch
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
auto farrow_rates_bank_multi_fn(bool fused)
{
    return fused ? farrow_rates_bank_multi_kernel<TX, R, NCX, true, kFarrowRatesOPL> : farrow_rates_bank_multi_kernel<TX, R, NCX, false, kFarrowRatesOPL>;
}

}  // namespace

// (the names mrhip_last_kernel_name reports carry no kernel suffix: include/multirate_hip.h at mrhip_last_kernel_name)
hipError_t launch_farrow_rates_bank_generic(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h || a.dyn) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    const long long bx = (a.n_out + kVariantThreads - 1) / kVariantThreads;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "farrow_rates_bank_generic";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(fused ? farrow_rates_bank_generic_kernel<TX, R, NCX, true> : farrow_rates_bank_generic_kernel<TX, R, NCX, false>, grid,
                      dim3(kVariantThreads), 0, s, a, r);
        return hipGetLastError();
    });
}

bool plan_farrow_rates_bank_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, ArbTileArgs *out)
{
    return plan_farrow_rates_bank_multi(tk, a, num_cus, MRHIP_ENV_INT("MRHIP_FARROW_RATES_BANK_MULTI", -1), out);
}

hipError_t prepare_farrow_rates_bank_multi(const TypeKey &tk, bool fused, const ArbTileArgs &ta, int num_cus, long long *grid)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_FARROW_RATES_BANK_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(farrow_rates_bank_multi_fn<TX, R, NCX>(fused)), kVariantThreads, 0,
                                                  num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        *grid = farrow_rates_multi_grid(ta.total_tiles, pg.grid, grid_fixed);
        return hipSuccess;
    });
}

hipError_t launch_farrow_rates_bank_multi(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, const ArbTileArgs &ta,
                                          long long grid, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h || a.dyn || grid < 1 || ta.tile_out != static_cast<long long>(kFarrowRatesOPL) * kVariantThreads)
        return hipErrorInvalidValue;
    *kname = "farrow_rates_bank_multi";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(farrow_rates_bank_multi_fn<TX, R, NCX>(fused), dim3(static_cast<unsigned>(grid)), dim3(kVariantThreads), 0, s, a, r, ta);
        return hipGetLastError();
    });
}

}  // namespace mrhip
