// kernels_rates_arb.hip -- FIRArbitrary (src/Filters.jl:91-117, 663-742) with PER-CHANNEL RATES, over shared or PER-CHANNEL TAPS.
//
// In the reference N signals are N FIRFilter(h, rate_c, N𝜙) objects, and every rate_c may differ (receivers each off its own clock trimmed
// to a common rate, per-emitter Doppler time-scale correction, per-channel fractional delay).  The phase schedule (update(), :663-673)
// depends on the rate, so mrhip_create_arbitrary_rates builds ONE filter whose channels share h -- pfb and dpfb -- N𝜙, the call length
// and the history length, and each have their own Δ, 𝜙Accumulator, xIdx, inputDeficit and per-call output count (RateChannel, rates_arb.h).
// A call is two launches on the caller's stream and nothing else:
//
//   1. rates_schedule_kernel, one lane per channel: the short-input rule of filt! (:705-709), else the serial walk of update() from
//      xIdx = inputDeficit while xIdx <= x_len (:715-732).  Entry k of channel c goes into the channel's slice of the schedule in the
//      existing entry format (1-based input index, accumulator); the count and the end state go into the channel's record.  The step is
//      sched_step_nb (sched_step.h): the text kernels_schedule.hip runs, and the one tests/rates_step_check.cpp checks on the CPU against
//      the oracle.  The lanes of a wave store into slices a stride apart, an entry each per step.  Consecutive steps of a lane fill one
//      cache line, so the L2 may gather them; nobody has measured the store path, nor the alternative of collecting 64 steps in LDS and
//      storing whole lines.
//      A call with per-channel input lengths (mrhip_filt_device_rates_ragged) runs rates_ragged_schedule_kernel: the same walk, every
//      lane against its channel's own length.
//   2. a filter kernel, a lane per (channel, output): n and acc from the channel's slice, the count from the channel's record; the
//      universal kernel (arb_rates_generic_kernel) or the LDS-tiled one (arb_rates_tiled_kernel, behind plan_arb_rates_tiled).
//
// Arithmetic (include/multirate_hip.h, "Per-channel rates for FIRArbitrary"): that of arb_generic_kernel -- both dots over one window,
// oldest sample first, the first product initialises the accumulator, no start-from-zero seam; STRICT: every multiply and add rounded
// separately in R, FUSED: one fma per tap; the combine in Float64, then rounded to R (RealTaps, variant_device.h) -- so channel c is bit
// for bit mrhip_create_arbitrary(h, rates[c], N𝜙, nch = 1) fed x_c.  This file is compiled with -ffp-contract=off.
// Both filter kernels end with the ShiftFold epilogue (the history depends on neither the rate nor the taps).  No workgroup waits for
// another.
//
// PER-CHANNEL TAPS (BANK, the kernels' last template argument): the general case of the reference's model, N FIRFilter(h_c, rate_c, N𝜙)
// objects with taps and rate both differing per channel (receivers each off its own clock AND each with its own front-end equaliser;
// per-emitter Doppler correction with the emitter's own matched pulse).  A filter on which mrhip_set_channel_taps was called holds nch
// pfb and nch dpfb banks, [nch][Nphi][T] in R, in the place of the one shared pair (include/multirate_hip.h, "Per-channel taps with
// per-channel rates for FIRArbitrary"), and TypeKey::bank is set; everything else of a call is as above.  The kernels are ONE text for
// both: BANK moves the column of the universal kernel to bank ch, and in the tiled kernel moves the copy of the banks into LDS from in
// front of the tile loop to the first live tile of each channel.  Channel c is then bit for bit mrhip_create_arbitrary(h_c, rates[c], N𝜙,
// nch = 1) fed x_c.  rates_key is the one place that reads TypeKey::bank on the launch side.
#include "rates_arb.h"
#include "sched_step.h"
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kRatesSchedThreads = 64;     // one wave a workgroup: the walks of a wave's lanes run side by side, the waves spread over the CUs

struct RateStep { double delta, N, invN; };

// The walk of lane c.  RAGGED: against the channel's own length (mrhip_filt_device_rates_ragged); else against the call's one length, a
// scalar -- the statement mrhip_filt_device_rates has always run, in instantiations of its own: with the lookup decided at run time the
// old call's walk measured 3 % slower.
template <bool POW2, bool RAGGED>
__device__ __forceinline__ void rates_walk(const RatesSchedArgs &s)
{
    const int c = static_cast<int>(blockIdx.x) * kRatesSchedThreads + static_cast<int>(threadIdx.x);
    if (c >= s.nch) return;
    RateChannel *const rec = s.rec + c;
    const long long len = RAGGED ? rates_channel_len(s.x_lens, s.x_len, c) : s.x_len;
    long long deficit = rec->inputDeficit;
    long long count = 0;
    if (len < deficit) {                                       // :705-709: nothing but the deficit moves (len == 0: nothing at all)
        rec->inputDeficit = deficit - len;
    } else {
        const RateStep step{rec->delta, s.N, s.invN};
        double acc = rec->acc;
        long long x = deficit;                                 // :715
        int *const n = s.n_idx + static_cast<long long>(c) * s.slice;
        double *const pa = s.acc + static_cast<long long>(c) * s.slice;
        while (x <= len && count < s.slice) {                  // :717 (the slice holds the call's bound: the second test never ends a walk)
            n[count] = static_cast<int>(x);
            pa[count] = acc;
            ++count;
            sched_step_nb<POW2>(acc, x, step);                 // :731
        }
        if (x <= len) rec->error = MRHIP_ERR_BUFFER_TOO_SMALL;
        rec->acc = acc;
        rec->xIdx = x;
        rec->inputDeficit = x - len;                           // :734
    }
    rec->count = count;
    if (s.counts_out) s.counts_out[c] = count;
}

template <bool POW2>
__global__ __launch_bounds__(kRatesSchedThreads) void rates_schedule_kernel(RatesSchedArgs s) { rates_walk<POW2, false>(s); }
template <bool POW2>
__global__ __launch_bounds__(kRatesSchedThreads) void rates_ragged_schedule_kernel(RatesSchedArgs s) { rates_walk<POW2, true>(s); }

__global__ __launch_bounds__(kRatesSchedThreads) void rates_reset_kernel(RateChannel *rec, int nch)
{
    const int c = static_cast<int>(blockIdx.x) * kRatesSchedThreads + static_cast<int>(threadIdx.x);
    if (c >= nch) return;
    rec[c].acc = 1.0; rec[c].inputDeficit = 1; rec[c].xIdx = 1; rec[c].count = 0; rec[c].error = 0;    // Filters.jl:110-115
    rec[c].len_refused = 0;
}

// mrhip_set_channel_rates_device: the rate of channel c from DEVICE memory, in stream order.  A value that is finite and inside the range
// the caller declared (lo <= r <= hi, both finite and > 0: a NaN fails both comparisons) is installed as mrhip_set_channel_rates installs
// it -- delta = N𝜙 / r, one Float64 division --; any other leaves the record's rate and delta alone and marks the record, unless an
// earlier status is still there.  Accumulator, inputDeficit, xIdx and count are not touched.
__global__ __launch_bounds__(kRatesSchedThreads) void rates_set_kernel(RateChannel *rec, const double *__restrict__ rates, double lo, double hi,
                                                                       double N, int nch)
{
    const int c = static_cast<int>(blockIdx.x) * kRatesSchedThreads + static_cast<int>(threadIdx.x);
    if (c >= nch) return;
    const double r = rates[c];
    if (r >= lo && r <= hi) { rec[c].rate = r; rec[c].delta = N / r; }      // Filters.jl:113
    else if (rec[c].error == 0) rec[c].error = MRHIP_ERR_INVALID_ARG;
}

// mrhip_filt_device_rates_lens_device, mrhip_filt_device_rates_chained: the length of channel c from DEVICE memory, in stream order, into
// the filter's array of lengths that the ragged schedule kernel and the filter kernels behind it read.  The value comes from the caller's
// array, from record c of the previous filter (its latest call's count) or from the previous one-state filter's call record (one count
// for every channel).  rates_length_accepted (rates_arb.h) decides: an accepted value is stored; any other stores 0 -- the channel is fed
// nothing, as by a ragged call's length 0 -- and marks the record.  Nothing else of the record is touched; every lane stores to its own
// channel's words only.
__global__ __launch_bounds__(kRatesSchedThreads) void rates_lens_set_kernel(RatesLensArgs a)
{
    const int c = static_cast<int>(blockIdx.x) * kRatesSchedThreads + static_cast<int>(threadIdx.x);
    if (c >= a.nch) return;
    const long long l = a.source == kRatesLensCaller ? a.src[c] : a.source == kRatesLensRecords ? a.prev_rec[c].count : a.prev_call->n_out;
    const bool ok = rates_length_accepted(l, a.len_max);
    a.x_lens[c] = ok ? l : 0;
    if (!ok) a.rec[c].len_refused = 1;
}

// One lane per (channel, output), any (Nphi, T, hLen, rates): blockIdx.x covers the outputs up to the call's bound, blockIdx.y strides
// the channels; the channel's count is uniform over the workgroup.  BANK: tp / dp start at bank ch.
template <typename TX, typename R, int NCX, bool FUSED, bool BANK>
__global__ __launch_bounds__(kVariantThreads) void arb_rates_generic_kernel(ArbArgs a, RatesArgs r)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    [[maybe_unused]] const long long bank_elems = static_cast<long long>(a.Nphi) * a.T;      // (read under BANK only)
    for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
        if (k >= r.rec[ch].count) continue;
        const long long n = a.n_idx[static_cast<long long>(ch) * r.slice + k];
        double alpha;
        const int phi = arb_phase(a.acc[static_cast<long long>(ch) * r.slice + k], &alpha);
        long long col = static_cast<long long>(phi) * a.T;
        if constexpr (BANK) col = ch * bank_elems + col;       // column phi of bank ch
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

// The pfb and the dpfb bank that start at element `first` of taps / dtaps -> LDS with a column pitch of TP taps, both in ONE pass over the
// elements (one index division for the pair; bank_to_lds of variant_device.h is this loop for one bank): element (phi, i) at phi*TP + i.
template <typename R>
__device__ __forceinline__ void rates_banks_to_lds(R *lpfb, R *ldpfb, const void *taps, const void *dtaps, long long first, int elems, int T, int TP, int tid)
{
    const R *__restrict__ g0 = static_cast<const R *>(taps) + first;
    const R *__restrict__ g1 = static_cast<const R *>(dtaps) + first;
    for (int e = tid; e < elems; e += kVariantThreads) {
        const int phi = e / T, i = e - phi * T;
        lpfb[phi * TP + i] = g0[e];
        ldpfb[phi * TP + i] = g1[e];
    }
}

// Persistent workgroups in the channel-major tile order (tile_run, variant_device.h).  A tile is (channel, run of tile_out = 256
// outputs); the tiling goes by the call's bound.  A tile at or behind its channel's count is skipped BEFORE any barrier (the skip is
// uniform over the workgroup).  The workgroup holds ONE pfb and dpfb in LDS (column pitch T + 1: lanes of different phases read different
// LDS banks).  !BANK: the pair all channels share, copied ONCE per workgroup in front of the tile loop.  BANK: one channel's pair,
// reloaded only when a live tile belongs to another channel than the one in LDS (ch_in_lds): the first live tile after any number of
// skipped ones finds its own channel's banks or loads them, and a channel without outputs in this call never has its banks loaded.  The
// tile's run of samples is read from the channel's own slice of the schedule (tile_span) -- so it follows that channel's rate -- and
// staged through LDS up to the channel's own length (stage_window); a tile whose run is longer than the planned span (a channel that
// decimates heavily) reads its windows from global memory (arb_dots_global), its taps still from LDS.
template <typename TX, typename R, int NCX, bool FUSED, bool BANK>
__global__ __launch_bounds__(kVariantThreads) void arb_rates_tiled_kernel(ArbArgs a, RatesArgs r, ArbTileArgs ta)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = typename A::Sample;
    extern __shared__ __attribute__((aligned(16))) unsigned char rates_arb_smem[];
    R *const lpfb = reinterpret_cast<R *>(rates_arb_smem);
    R *const ldpfb = lpfb + ta.bank_elems;
    Sample *const lx = reinterpret_cast<Sample *>(rates_arb_smem + ta.x_offset_bytes);

    const int tid = threadIdx.x;
    const int T = a.T, TP = ta.tap_pitch;
    const TileRun run = tile_run(ta.total_tiles);
    const int bank_elems = a.Nphi * T;
    [[maybe_unused]] int ch_in_lds = -1;
    if constexpr (!BANK) {
        if (run.begin < run.end) rates_banks_to_lds(lpfb, ldpfb, a.taps, a.dtaps, 0, bank_elems, T, TP, tid);
    }

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

        __syncthreads();   // the previous live tile's reads of the window (BANK: and of the banks) are done
        if constexpr (BANK) {
            if (ch != ch_in_lds) {   // (uniform over the workgroup) channel ch's banks
                rates_banks_to_lds(lpfb, ldpfb, a.taps, a.dtaps, static_cast<long long>(ch) * bank_elems, bank_elems, T, TP, tid);
                ch_in_lds = ch;
            }
        }
        if (w.staged) stage_window(lx, xc, hc, w.o, static_cast<int>(w.span), len, a.H, tid);
        __syncthreads();   // (!BANK, the first one of a workgroup: the banks are in LDS too)

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

template <typename TX, typename R, int NCX, bool BANK>
auto arb_rates_tiled_fn(bool fused)
{
    return fused ? arb_rates_tiled_kernel<TX, R, NCX, true, BANK> : arb_rates_tiled_kernel<TX, R, NCX, false, BANK>;
}

}  // namespace

hipError_t launch_rates_schedule(const RatesSchedArgs &s, bool pow2, hipStream_t st)
{
    const dim3 grid(static_cast<unsigned>((s.nch + kRatesSchedThreads - 1) / kRatesSchedThreads));
    if (s.x_lens) launch_kernel(pow2 ? rates_ragged_schedule_kernel<true> : rates_ragged_schedule_kernel<false>, grid, dim3(kRatesSchedThreads), 0, st, s);
    else if (pow2) launch_kernel(rates_schedule_kernel<true>, grid, dim3(kRatesSchedThreads), 0, st, s);
    else launch_kernel(rates_schedule_kernel<false>, grid, dim3(kRatesSchedThreads), 0, st, s);
    return hipGetLastError();
}

hipError_t launch_rates_reset(RateChannel *rec, int nch, hipStream_t st)
{
    const dim3 grid(static_cast<unsigned>((nch + kRatesSchedThreads - 1) / kRatesSchedThreads));
    hipLaunchKernelGGL(rates_reset_kernel, grid, dim3(kRatesSchedThreads), 0, st, rec, nch);
    return hipGetLastError();
}

hipError_t launch_rates_set(RateChannel *rec, const double *rates, double lo, double hi, double N, int nch, hipStream_t st)
{
    const dim3 grid(static_cast<unsigned>((nch + kRatesSchedThreads - 1) / kRatesSchedThreads));
    hipLaunchKernelGGL(rates_set_kernel, grid, dim3(kRatesSchedThreads), 0, st, rec, rates, lo, hi, N, nch);
    return hipGetLastError();
}

hipError_t launch_rates_lens_set(const RatesLensArgs &l, hipStream_t st)
{
    const dim3 grid(static_cast<unsigned>((l.nch + kRatesSchedThreads - 1) / kRatesSchedThreads));
    hipLaunchKernelGGL(rates_lens_set_kernel, grid, dim3(kRatesSchedThreads), 0, st, l);
    return hipGetLastError();
}

// TypeKey::bank is read HERE and nowhere else in this unit: it chooses the kernels' BANK argument (dispatch_variant_flag), the names
// mrhip_last_kernel_name reports (without a kernel suffix: include/multirate_hip.h at mrhip_last_kernel_name) and the environment switches
// together.  (MRHIP_ENV_INT caches per call site behind a literal name: two sites a switch.)
static RatesKey rates_key(const TypeKey &tk)
{
    return RatesKey{tk.bank, tk.bank ? "arb_rates_bank_generic" : "arb_rates_generic", tk.bank ? "arb_rates_bank_tiled" : "arb_rates_tiled",
                    tk.bank ? MRHIP_ENV_INT("MRHIP_ARB_RATES_BANK_TILED", -1) : MRHIP_ENV_INT("MRHIP_ARB_RATES_TILED", -1),
                    tk.bank ? MRHIP_ENV_INT("MRHIP_ARB_RATES_BANK_GRID", 0) : MRHIP_ENV_INT("MRHIP_ARB_RATES_GRID", 0)};
}

hipError_t launch_arb_rates_generic(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, hipStream_t s, const char **kname)
{
    if (tk.complex_h || a.dyn) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    const long long bx = (a.n_out + kVariantThreads - 1) / kVariantThreads;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    const RatesKey key = rates_key(tk);
    *kname = key.generic;
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>() -> hipError_t {
        launch_kernel(fused ? arb_rates_generic_kernel<TX, R, NCX, true, BANK> : arb_rates_generic_kernel<TX, R, NCX, false, BANK>, grid,
                      dim3(kVariantThreads), 0, s, a, r);
        return hipGetLastError();
    });
}

bool plan_arb_rates_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_arb_rates_tiled(tk, a, rate_min, num_cus, rates_key(tk).tiled_mode, out, lds);
}

hipError_t prepare_arb_rates_tiled(const TypeKey &tk, bool fused, const ArbTileArgs &ta, size_t lds, int num_cus, long long *grid)
{
    if (tk.complex_h) return hipErrorInvalidValue;
    const RatesKey key = rates_key(tk);
    return dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>() -> hipError_t {
        const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(arb_rates_tiled_fn<TX, R, NCX, BANK>(fused)), kVariantThreads, lds,
                                                  num_cus, ta.total_tiles);
        if (pg.err != hipSuccess) return pg.err;
        long long g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
        if (key.grid_fixed > 0) g = std::min<long long>(key.grid_fixed, 65535);       // (tests: also more workgroups than tiles)
        *grid = g;
        return hipSuccess;
    });
}

hipError_t launch_arb_rates_tiled(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, const ArbTileArgs &ta, size_t lds,
                                  long long grid, hipStream_t s, const char **kname)
{
    if (tk.complex_h || a.dyn || grid < 1) return hipErrorInvalidValue;
    const RatesKey key = rates_key(tk);
    *kname = key.tiled;
    return dispatch_variant_flag(tk, key.bank, [&]<typename TX, typename R, int NCX, bool BANK>() -> hipError_t {
        launch_kernel(arb_rates_tiled_fn<TX, R, NCX, BANK>(fused), dim3(static_cast<unsigned>(grid)), dim3(kVariantThreads), lds, s, a, r, ta);
        return hipGetLastError();
    });
}

}  // namespace mrhip
