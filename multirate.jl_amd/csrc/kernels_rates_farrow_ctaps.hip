// kernels_rates_farrow_ctaps.hip -- FIRFarrow (src/Filters.jl:123-147, 764-839) with PER-CHANNEL RATES and COMPLEX PER-CHANNEL TAPS.
//
// The general case of the reference's model for a continuously variable rate with a complex prototype: N
// FIRFilter(h_c::Vector{Complex}, rate_c, N𝜙, polyorder) objects, taps and rate both differing per channel -- per-emitter Doppler
// correction is both at once, a time scale that a tracker moves every chunk (a rate per channel) and a carrier offset (a matched pulse
// or equaliser rotated to the channel's own frequency).  A filter of mrhip_create_farrow_rates* on which mrhip_set_channel_ctaps_farrow,
// mrhip_set_channel_pnfb_ctaps or mrhip_set_channel_pnfb_ctaps_device was called holds nch polynomial banks of (re, im) pairs of
// Float64, [nch][T][polyorder+1][2] (include/multirate_hip.h, "Complex per-channel taps with per-channel rates for FIRFarrow"), and
// TypeKey::complex_h and ::bank are both set.  A call is the two launches of kernels_rates_farrow.hip: the schedule kernel (the walk
// does not depend on the taps), then one of the two filter kernels below: n and phase from the channel's slice, the count from the
// channel's record.
//
//   farrow_rates_ctaps_generic_kernel: one lane per (channel, output), any (T, polyorder, rates).
//   farrow_rates_ctaps_multi_kernel: persistent workgroups over the channel-major tile order, a lane owns kFarrowRatesCtapsOPL outputs of
//      one channel and one set of scalar coefficient loads per tap feeds all their Horner chains (behind plan_farrow_rates_ctaps_multi,
//      host_logic.cpp).
//
// These are the statements of farrow_rates_generic_kernel and farrow_rates_multi_kernel with BANK true under the complex tap algebra
// (ComplexTaps, variant_device.h: the arithmetic of ctaps_device.h).  They stand in a unit of their own because kernels_rates_farrow.hip
// is one text over RealTaps whose instantiations are counted, and farrow_variant_bank_generic_body (variant_device.h) reads ONE slice and
// the call's one count; one text over the algebra for both units is a later refactor.
//
// Arithmetic (include/multirate_hip.h, "FIRFarrow with complex taps", on bank c): Horner in Float64 from the highest power PER COMPONENT
// (t = 𝜙*v; v = coef + t, the product and the sum each rounded once, never fused), one rounding to the tap's real scalar, widened
// exactly to R; the dot oldest sample first, the first product initialises the sum, Complex*Real / Complex*Complex written out, every
// multiply, add and subtract rounded separately in R; outputs on the seam (n < seam_below: every call of this filter starts a filt!)
// start from +0 per component (support.jl:46).  STRICT only: there is no FUSED form.  So channel c is bit for bit
// mrhip_create_farrow_pnfb_ctaps(bank_c, rates[c], N𝜙, polyorder, nch = 1) fed x_c.  This file is compiled with -ffp-contract=off.
//
// The channel is uniform per workgroup in both kernels (blockIdx.y strides the channels; a tile is one channel), so the bank base
// pnfb + ch*T*(P+1)*2 is, and every coefficient is a scalar operand read through the constant address space (farrow_coef_t).  Both
// kernels end with the ShiftFold epilogue (the history depends on neither the rate nor the taps), with no return in front of it.  No
// LDS, no barrier; no workgroup waits for another.
#include "rates_arb.h"
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// One lane per (channel, output): blockIdx.x covers the outputs up to the call's bound, blockIdx.y strides the channels; the channel's
// count and its bank are uniform over the workgroup.  The tap: ComplexTaps::farrow_tap<PP> (two Horner chains, farrow_bank_horner<PP, 2>).
template <typename TX, typename R, int NCX>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_ctaps_generic_kernel(FarrowArgs a, RatesArgs r)
{
    using A = ComplexTaps<TX, R, NCX>;
    using Sample = typename A::Sample;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    const int poly = (P + 1) * A::kCoefScalars;      // Float64 scalars of one tap's polynomial
    const long long bank_elems = static_cast<long long>(T) * poly;
    auto channels = [&]<int PP>() {
        for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
            if (k >= r.rec[ch].count) continue;
            farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + ch * bank_elems;      // bank ch
            const long long n = a.n_idx[static_cast<long long>(ch) * r.slice + k];
            const double phase = a.acc[static_cast<long long>(ch) * r.slice + k];
            const long long base = n - T;               // 0-based index of the oldest sample (>= -H: n >= 1)
            const bool seam = n < a.seam_below;         // kernel.xIdx < kernel.tapsPer𝜙, Filters.jl:819
            const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
            const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
            typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
            auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
            typename A::Sum acc = A::first(A::template farrow_tap<PP>(pc, P, phase, tap_f32), sample(base));
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
    if (r.x_lens) dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{});
    else dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// The OPL complex taps of ONE polynomial of (re, im) pairs, each at its own phase: the 2(P+1) coefficients are loaded once as scalars and
// feed all 2 OPL Horner chains, which are independent, so they interleave and cover each other's Float64 latency.  Per chain the
// statement of farrow_bank_horner<PP, 2> (variant_device.h) and the rounding of ComplexTaps::farrow_tap.  PP >= 0: the polyorder at
// compile time, the loads issued together and waited for once; PP < 0: any polyorder, one pair of loads per Horner step.
template <typename Tap, typename R, int PP, int OPL>
__device__ __forceinline__ void farrow_rates_ctaps_taps(farrow_coef_t c, const int P, const bool tap_f32, const double (&phase)[OPL], Tap (&tap)[OPL])
{
    double vr[OPL], vi[OPL];
    if constexpr (PP >= 0) {
        double cj[(PP + 1) * 2];
#pragma unroll
        for (int e = 0; e < (PP + 1) * 2; ++e) cj[e] = c[e];
#pragma unroll
        for (int q = 0; q < OPL; ++q) { vr[q] = cj[PP * 2]; vi[q] = cj[PP * 2 + 1]; }
#pragma unroll
        for (int j = PP - 1; j >= 0; --j) {
#pragma unroll
            for (int q = 0; q < OPL; ++q) {
                const double tr = phase[q] * vr[q];
                vr[q] = cj[j * 2] + tr;
                const double ti = phase[q] * vi[q];
                vi[q] = cj[j * 2 + 1] + ti;
            }
        }
    } else {
        const double top_re = c[P * 2], top_im = c[P * 2 + 1];
#pragma unroll
        for (int q = 0; q < OPL; ++q) { vr[q] = top_re; vi[q] = top_im; }
        for (int j = P - 1; j >= 0; --j) {
            const double cre = c[j * 2], cim = c[j * 2 + 1];
#pragma unroll
            for (int q = 0; q < OPL; ++q) {
                const double tr = phase[q] * vr[q];
                vr[q] = cre + tr;
                const double ti = phase[q] * vi[q];
                vi[q] = cim + ti;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < OPL; ++q) {
        tap[q].re = tap_f32 ? static_cast<R>(static_cast<float>(vr[q])) : static_cast<R>(vr[q]);
        tap[q].im = tap_f32 ? static_cast<R>(static_cast<float>(vi[q])) : static_cast<R>(vi[q]);
    }
}

// The OPL dots of one lane: per tap ONE set of the coefficients' scalar loads, 2 OPL Horner chains, OPL complex multiply-adds; sample xi
// of a window comes from x (xi >= 0) or from the end of the history (he[xi], xi < 0).  The first `live` slots are stored.  pc: the first
// coefficient of the lane's channel's bank, [T][P+1] pairs.
template <typename A, typename R, int PP, int OPL>
__device__ __forceinline__ void farrow_rates_ctaps_dots(farrow_coef_t pc, const int P, const int T, const bool tap_f32, const double (&phase)[OPL],
                                                        const long long (&base)[OPL], const bool (&seam)[OPL],
                                                        const typename A::Sample *__restrict__ xc, const typename A::Sample *__restrict__ he,
                                                        typename A::Out *__restrict__ yc, const long long k_first, const int live)
{
    const int poly = (P + 1) * A::kCoefScalars;
    typename A::Sum acc[OPL];
    typename A::Tap tap[OPL];
    farrow_rates_ctaps_taps<typename A::Tap, R, PP, OPL>(pc, P, tap_f32, phase, tap);
#pragma unroll
    for (int j = 0; j < OPL; ++j) {
        const long long xi = base[j];
        acc[j] = A::first(tap[j], xi >= 0 ? xc[xi] : he[xi]);
        if (seam[j]) acc[j] = A::zero_start(acc[j]);
    }
    for (int i = 1; i < T; ++i) {
        farrow_rates_ctaps_taps<typename A::Tap, R, PP, OPL>(pc + i * poly, P, tap_f32, phase, tap);
#pragma unroll
        for (int j = 0; j < OPL; ++j) {
            const long long xi = base[j] + i;
            acc[j] = A::step(acc[j], tap[j], xi >= 0 ? xc[xi] : he[xi]);
        }
    }
#pragma unroll
    for (int j = 0; j < OPL; ++j)
        if (j < live) A::store(yc, k_first + j * kVariantThreads, acc[j]);
}

// Persistent workgroups in the channel-major tile order (tile_run, variant_device.h).  A tile is (channel, OPL consecutive runs of 256
// outputs); lane `tid` owns output `tid` of each run (slot j: k0 + tid + 256 j), so neighbouring lanes keep neighbouring outputs and the
// y stores stay coalesced.  The tiling goes by the call's bound; tiles at or behind the channel's count are skipped, and so are a lane's
// slots at or behind it (farrow_rates_ctaps_live_slots, rates_arb.h: the live slots are the first ones).  A slot that is not live computes
// on slot 0's entry -- loads from valid addresses, no store -- so the chains stay one straight-line statement.  The windows are read from
// global memory and the history: no LDS, no barrier.  A tile is ONE channel, so its bank base is taken per tile, uniform over the
// workgroup.
template <typename TX, typename R, int NCX, int OPL>
__global__ __launch_bounds__(kVariantThreads) void farrow_rates_ctaps_multi_kernel(FarrowArgs a, RatesArgs r, ArbTileArgs ta)
{
    using A = ComplexTaps<TX, R, NCX>;
    using Sample = typename A::Sample;
    const int tid = threadIdx.x;
    const int P = a.polyorder, T = a.T;
    const bool tap_f32 = a.tap_f32 != 0;
    const long long bank_elems = static_cast<long long>(T) * (P + 1) * A::kCoefScalars;
    const TileRun run = tile_run(ta.total_tiles);

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile<true>(tile, ta, a.n_out);
        const int ch = t.ch;
        const long long count = r.rec[ch].count;
        if (t.k0 >= count) continue;     // (uniform over the workgroup) a tile at or behind the channel's count
        const int live = farrow_rates_ctaps_live_slots(t.k0, tid, count);
        if (live == 0) continue;         // (no barrier in this kernel: a lane may leave a tile on its own)
        farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + ch * bank_elems;       // bank ch
        const int *__restrict__ nc = a.n_idx + static_cast<long long>(ch) * r.slice;
        const double *__restrict__ ac = a.acc + static_cast<long long>(ch) * r.slice;
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ he = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H + a.H;   // the end of the history
        typename A::Out *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
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
            farrow_rates_ctaps_dots<A, R, kFarrowBankUnrolledP, OPL>(pc, P, T, tap_f32, phase, base, seam, xc, he, yc, k_first, live);
        else farrow_rates_ctaps_dots<A, R, -1, OPL>(pc, P, T, tap_f32, phase, base, seam, xc, he, yc, k_first, live);
    }
    if (r.x_lens) dev::shiftin_ragged_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, r.x_lens, a.H, a.nch, RatesHistSource{});
    else dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// the two switches, each a literal name at a site of its own (MRHIP_ENV_INT caches per call site)
int ctaps_multi_mode() { return MRHIP_ENV_INT("MRHIP_FARROW_RATES_CTAPS_MULTI", -1); }
int ctaps_grid_fixed() { return MRHIP_ENV_INT("MRHIP_FARROW_RATES_CTAPS_GRID", 0); }

bool ctaps_key(const TypeKey &tk) { return tk.complex_h && tk.bank; }

}  // namespace

hipError_t launch_farrow_rates_ctaps_generic(const TypeKey &tk, const FarrowArgs &a, const RatesArgs &r, hipStream_t s, const char **kname)
{
    if (!ctaps_key(tk) || a.dyn) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    const long long bx = (a.n_out + kVariantThreads - 1) / kVariantThreads;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "farrow_rates_ctaps_generic";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(farrow_rates_ctaps_generic_kernel<TX, R, NCX>, grid, dim3(kVariantThreads), 0, s, a, r);
        return hipGetLastError();
    });
}

bool plan_farrow_rates_ctaps_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, ArbTileArgs *out)
{
    return plan_farrow_rates_ctaps_multi(tk, a, num_cus, ctaps_multi_mode(), out);
}

hipError_t prepare_farrow_rates_ctaps_multi(const TypeKey &tk, const ArbTileArgs &ta, int num_cus, long long *grid)
{
    if (!ctaps_key(tk)) return hipErrorInvalidValue;
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(farrow_rates_ctaps_multi_kernel<TX, R, NCX, kFarrowRatesCtapsOPL>),
                                                  kVariantThreads, 0, num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        *grid = farrow_rates_multi_grid(ta.total_tiles, pg.grid, ctaps_grid_fixed());
        return hipSuccess;
    });
}

hipError_t launch_farrow_rates_ctaps_multi(const TypeKey &tk, const FarrowArgs &a, const RatesArgs &r, const ArbTileArgs &ta, long long grid,
                                           hipStream_t s, const char **kname)
{
    if (!ctaps_key(tk) || a.dyn || grid < 1 || ta.tile_out != static_cast<long long>(kFarrowRatesCtapsOPL) * kVariantThreads)
        return hipErrorInvalidValue;
    *kname = "farrow_rates_ctaps_multi";
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        launch_kernel(farrow_rates_ctaps_multi_kernel<TX, R, NCX, kFarrowRatesCtapsOPL>, dim3(static_cast<unsigned>(grid)), dim3(kVariantThreads), 0, s,
                      a, r, ta);
        return hipGetLastError();
    });
}

}  // namespace mrhip
