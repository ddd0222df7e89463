// rates_arb.h -- FIRArbitrary with PER-CHANNEL RATES (mrhip_create_arbitrary_rates; include/multirate_hip.h, "Per-channel rates for
// FIRArbitrary"): what api.hip, host_logic.cpp (the tiled kernel's plan) and kernels_rates_arb.hip (the kernels) share; and, below,
// FIRFarrow with per-channel rates (mrhip_create_farrow_rates; kernels_rates_farrow.hip), which uses the same records and schedule
// kernel.  Either filter may hold shared taps or a bank per channel (TypeKey::bank): one set of functions per family serves both.  Kept
// out of mrhip_internal.h so that only those units depend on it.
#pragma once

#include "mrhip_internal.h"

namespace mrhip {

// One channel's stream state on the device: what update() and filt! (src/Filters.jl:663-673, 693-742) mutate, per channel.  Written by
// the schedule kernel of every call in stream order; the filter kernels of that call read `count`.  𝜙Idx and α are floor(acc) and
// acc - 𝜙Idx (:671-672): derived where they are asked for.
struct RateChannel {
    double rate, delta;            // constants: rates[c], N𝜙 / rates[c] (:113)
    double acc;                    // 𝜙Accumulator
    long long inputDeficit, xIdx;  // 1-based, reference field names
    long long count;               // outputs of the latest call
    long long error;               // sticky: a call whose walk ran past the slice its bound gave it (mrhip_get_channel_states reports it)
    long long len_refused;         // sticky, apart from `error`: a device-resident LENGTH of this channel was refused (rates_lens_set_kernel)
};
static_assert(sizeof(RateChannel) == 64, "one record a cache line half");

struct RatesSchedArgs {            // the schedule kernel: one lane per channel
    RateChannel *rec;              // [nch]
    int *n_idx;                    // [nch][slice]: entry k of channel c, the existing entry format (1-based input index ...
    double *acc;                   //                ... and the accumulator the output is computed at)
    long long *counts_out;         // NULL, or [nch]: the counts, in stream order
    long long slice;               // entries per channel (>= the call's bound)
    long long x_len;
    double N, invN;                // N𝜙, 1 / N𝜙
    int nch;
    const long long *x_lens;       // NULL (mrhip_filt_device_rates: every channel is fed x_len samples), or [nch]: the channels' own lengths
};

struct RatesArgs {                 // beside ArbArgs (whose n_idx / acc are the bases of the slices, n_out the call's bound, dyn NULL)
    const RateChannel *rec;
    long long slice;
    const long long *x_lens;       // as in RatesSchedArgs (the filter's one device array, written in stream order ahead of the call)
};

#if defined(__HIPCC__)
#define MRHIP_RATES_HD __host__ __device__
#else
#define MRHIP_RATES_HD
#endif

// the samples channel c is fed by this call: its own length (mrhip_filt_device_rates_ragged), else the call's one length
MRHIP_RATES_HD inline long long rates_channel_len(const long long *x_lens, long long x_len, int c) { return x_lens ? x_lens[c] : x_len; }

// shiftin! (support.jl:61-80) of ONE channel that was fed `len` samples: the new history is the last H samples of [hist ; x[0:len)], so
// element i (0 <= i < H) comes from the old history at index i + len when that is < H, else from x at index i + len - H.  len == 0
// gives the old history back; len >= H takes everything from x.  The kernels' ragged epilogue and tests/rates_ragged_check.cpp run
// this text.
struct HistSource { bool from_hist; long long index; };
MRHIP_RATES_HD inline HistSource rates_hist_source(long long i, long long len, int H)
{
    const long long e = i + len;                                 // index into [hist ; x]
    return e < H ? HistSource{true, e} : HistSource{false, e - H};
}
struct RatesHistSource {           // the rule as the argument of dev::shiftin_ragged_by_last_workgroup (pair_device.h)
    MRHIP_RATES_HD HistSource operator()(long long i, long long len, int H) const { return rates_hist_source(i, len, H); }
};

// ---- Input lengths from device memory, and chaining (mrhip_filt_device_rates_lens_device, mrhip_filt_device_rates_chained;
// include/multirate_hip.h, "Input lengths from device memory, and chaining, for the filters with per-channel rates") ---------------------
// The acceptance rule of a length the host never saw: channel c is fed l samples where 0 <= l <= len_max (the maximum the caller
// declared, for which the launch is sized and the buffers were checked); any other value feeds the channel NOTHING in this call.  The
// import kernel (rates_lens_set_kernel, kernels_rates_arb.hip) and tests/rates_device_lengths_check.cpp run this text.
MRHIP_RATES_HD inline bool rates_length_accepted(long long l, long long len_max) { return l >= 0 && l <= len_max; }

enum RatesLensSource { kRatesLensCaller = 0, kRatesLensRecords = 1, kRatesLensCall = 2 };
struct RatesLensArgs {             // the import kernel: one lane per channel
    RateChannel *rec;              // [nch]: the filter's records (the mark of a refused length)
    long long *x_lens;             // [nch]: the filter's device array of lengths, which the schedule and filter kernels of the call read
    const long long *src;          // kRatesLensCaller: the caller's lengths, DEVICE, [nch]
    const RateChannel *prev_rec;   // kRatesLensRecords: the records of the previous filter (per-channel rates), [nch]: `count`
    const DevCall *prev_call;      // kRatesLensCall: the call record of the previous one-state filter: `n_out`, for every channel
    long long len_max;
    int nch;
    int source;                    // RatesLensSource
};
// kernels_rates_arb.hip: the accepted length, or 0 and the mark, into x_lens[c], in stream order
hipError_t launch_rates_lens_set(const RatesLensArgs &l, hipStream_t st);

// What TypeKey::bank chooses on the launch side of a family, read in ONE place per unit (rates_key there): the kernels' BANK argument,
// the names mrhip_last_kernel_name reports and the values of the family's two environment switches.
struct RatesKey { bool bank; const char *generic, *tiled; int tiled_mode, grid_fixed; };

// kernels_rates_arb.hip.  Every function below takes either bank key: shared taps (ArbArgs::taps / dtaps hold the ONE pair of banks) or
// per-channel taps (mrhip_set_channel_taps on a filter of mrhip_create_arbitrary_rates; include/multirate_hip.h, "Per-channel taps with
// per-channel rates for FIRArbitrary": nch banks, [nch][Nphi][T] in R, and TypeKey::bank is set).  Records, slices, schedule kernel and
// RatesArgs serve both unchanged.  The key selects the reported name (arb_rates_generic / arb_rates_tiled, arb_rates_bank_generic /
// arb_rates_bank_tiled) and the switches (MRHIP_ARB_RATES_TILED / _GRID, MRHIP_ARB_RATES_BANK_TILED / _BANK_GRID).
hipError_t launch_rates_schedule(const RatesSchedArgs &s, bool pow2, hipStream_t st);
hipError_t launch_rates_reset(RateChannel *rec, int nch, hipStream_t st);                  // constructor state, in stream order
hipError_t launch_arb_rates_generic(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, hipStream_t s, const char **kname);
bool plan_arb_rates_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, ArbTileArgs *out, size_t *lds);   // (reads the key's TILED switch)
// the tiled kernel's persistent grid (occupancy query, LDS attribute; the key's GRID switch): everything about its launch that can fail
// ahead of the launch
hipError_t prepare_arb_rates_tiled(const TypeKey &tk, bool fused, const ArbTileArgs &ta, size_t lds, int num_cus, long long *grid);
hipError_t launch_arb_rates_tiled(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, const ArbTileArgs &ta, size_t lds,
                                  long long grid, hipStream_t s, const char **kname);
// host_logic.cpp: the switch value passed in (0 never, 1 wherever the plan fits, -1 the default rule of the bank key)
bool plan_arb_rates_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, int mode, ArbTileArgs *out, size_t *lds);

// ---- FIRFarrow with per-channel rates (mrhip_create_farrow_rates;include/multirate_hip.h, "Per-channel rates for FIRFarrow") --------
// The schedule kernel, the records, the reset kernel and RatesArgs above serve it unchanged: update() of FIRFarrow (Filters.jl:780-786)
// is FIRArbitrary's recurrence on the same Float64 quantity, and the constructor state (:141-144) is the one rates_reset_kernel writes
// (𝜙Idx = 1.0 is the accumulator, inputDeficit = xIdx = 1).  RatesArgs stands beside FarrowArgs (n_idx / acc: the bases of the slices,
// n_out: the call's bound, dyn NULL, seam_below = T, pnfb: the ONE bank [T][polyorder+1], or one per channel).
//
// farrow_rates_multi_kernel: a lane owns kFarrowRatesOPL outputs of one channel, output `tid` of as many consecutive runs of
// kVariantThreads outputs; a tile is those runs (tile_out = kFarrowRatesOPL * kVariantThreads outputs of one channel).
constexpr int kFarrowRatesOPL = 4;
// the slots of lane `tid` in the tile that starts at output k0 that lie in front of the channel's count: slot j is output
// k0 + tid + j * kVariantThreads; 0 ... kFarrowRatesOPL (the live slots are the first ones)
MRHIP_RATES_HD inline int farrow_rates_live_slots(long long k0, int tid, long long count)
{
    const long long left = count - k0 - tid;                     // outputs from the lane's first slot to the count
    if (left <= 0) return 0;
    const long long slots = (left + kVariantThreads - 1) / kVariantThreads;
    return slots < kFarrowRatesOPL ? static_cast<int>(slots) : kFarrowRatesOPL;
}

// kernels_rates_farrow.hip.  Every function below takes either bank key: the ONE bank, or a bank per channel
// (mrhip_set_channel_taps_farrow / mrhip_set_channel_pnfb on a filter of mrhip_create_farrow_rates*; include/multirate_hip.h,
// "Per-channel taps with per-channel rates for FIRFarrow": FarrowArgs::pnfb holds nch banks, [nch][T][polyorder+1], and TypeKey::bank is
// set).  Records, slices, schedule kernel, RatesArgs and the tile of kFarrowRatesOPL runs serve both unchanged.  The key selects the
// reported name (farrow_rates_generic / farrow_rates_multi, farrow_rates_bank_generic / farrow_rates_bank_multi) and the switches
// (MRHIP_FARROW_RATES_MULTI / _GRID, MRHIP_FARROW_RATES_BANK_MULTI / _BANK_GRID).
hipError_t launch_farrow_rates_generic(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, hipStream_t s, const char **kname);
bool plan_farrow_rates_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, ArbTileArgs *out);      // (reads the key's MULTI switch)
// the multi kernel's persistent grid (occupancy query; the key's GRID switch): everything about its launch that can fail ahead of the launch
hipError_t prepare_farrow_rates_multi(const TypeKey &tk, bool fused, const ArbTileArgs &ta, int num_cus, long long *grid);
hipError_t launch_farrow_rates_multi(const TypeKey &tk, bool fused, const FarrowArgs &a, const RatesArgs &r, const ArbTileArgs &ta,
                                     long long grid, hipStream_t s, const char **kname);
// host_logic.cpp: the switch value passed in (0 never, 1 every call, -1 the default rule of the bank key), and the grid from what the
// chip holds (chip_grid), the tile count and a test's replacement (grid_fixed > 0: also more workgroups than tiles)
bool plan_farrow_rates_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, int mode, ArbTileArgs *out);
long long farrow_rates_multi_grid(long long total_tiles, long long chip_grid, int grid_fixed);

// ---- Device-resident updates (mrhip_set_channel_rates_device, mrhip_set_channel_taps_device, mrhip_set_channel_pnfb_device;
// include/multirate_hip.h, "Device-resident updates for the filters with per-channel rates") ---------------------------------------------
// The banks of one channel as create_pfb_banks (host_logic.cpp) builds them from the channel's row h (hLen taps, T = ceil(hLen / N𝜙)):
// element e = 𝜙*T + i of the bank (phase 𝜙, row i) holds h[j] with j = (T-1-i)*N𝜙 + 𝜙, zero for j >= hLen (taps2pfb); the dpfb bank holds
// dh[j] = h[j+1] - h[j], ONE subtraction rounded in the tap type, zero for j >= hLen-1 (arbitrary_dh: [diff(h), 0]).  The build kernel
// (kernels_rates_bank_build.hip) and tests/rates_device_updates_check.cpp run this text.
MRHIP_RATES_HD inline long long rates_bank_tap_index(long long e, long long T, long long Nphi)
{
    const long long phi = e / T, i = e - phi * T;
    return (T - 1 - i) * Nphi + phi;
}
template <typename TAP>
MRHIP_RATES_HD inline TAP rates_bank_pfb_value(const TAP *h, long long hLen, long long j) { return j < hLen ? h[j] : TAP(0); }
template <typename TAP>
MRHIP_RATES_HD inline TAP rates_bank_dpfb_value(const TAP *h, long long hLen, long long j) { return j + 1 < hLen ? TAP(h[j + 1] - h[j]) : TAP(0); }

struct BankBuildArgs {             // the bank build kernel: one workgroup per (channel, slab of kBankBuildSlab bank elements)
    const void *h;                 // DEVICE, [nch][hLen] in the tap type
    void *pfb, *dpfb;              // DEVICE, [nch][Nphi*T] in R
    long long hLen, T, Nphi;
    int nch;
    int row_in_lds;                // the channel's row is staged in LDS (hLen taps fit kBankBuildLdsBytes); else the kernel reads global memory
};
constexpr int kBankBuildThreads = 256;
constexpr int kBankBuildSlab = 4 * kBankBuildThreads;      // bank elements of one workgroup
constexpr long long kBankBuildLdsBytes = 32 * 1024;        // the room a channel's row may take in LDS

// kernels_rates_arb.hip: rates[c] into record c where it is finite and inside [lo, hi], else the refusal into the record's status
hipError_t launch_rates_set(RateChannel *rec, const double *rates, double lo, double hi, double N, int nch, hipStream_t st);
// kernels_rates_bank_build.hip (tap_f64 / r_f64: the tap type of h and R of the banks; Float64 taps imply Float64 R)
hipError_t launch_rates_bank_build(bool tap_f64, bool r_f64, const BankBuildArgs &b, hipStream_t st);
// ... and n Float64 coefficients into the filter's polynomial banks, rounded to Float32 and widened back for Float32 taps
hipError_t launch_rates_pnfb_install(bool tap_f32, const double *src, double *dst, long long n, hipStream_t st);

// ---- COMPLEX per-channel taps on the FIRArbitrary filter with per-channel rates (mrhip_set_channel_ctaps, mrhip_set_channel_ctaps_device;
// include/multirate_hip.h, "Complex per-channel taps with per-channel rates for FIRArbitrary") -------------------------------------------
// The filter holds nch pfb and nch dpfb banks of (re, im) pairs of R, [nch][Nphi][T], and TypeKey::complex_h and ::bank are both set.
// Records, slices, schedule kernel and RatesArgs serve it unchanged; the two filter kernels and the bank build kernel live in
// kernels_rates_arb_ctaps.hip (kernels_rates_arb.hip refuses a complex_h key), their plan in host_logic.cpp.  Reported names:
// arb_rates_ctaps_generic / arb_rates_ctaps_tiled; switches: MRHIP_ARB_RATES_CTAPS_TILED (-1 rule, 0, 1), MRHIP_ARB_RATES_CTAPS_GRID.
//
// The banks of one channel from its row of hLen (re, im) pairs, h[2j] and h[2j + 1]: the index map is rates_bank_tap_index, the values
// are those of the real banks component by component -- create_pfb_banks moves a pair as one element, arbitrary_dh subtracts the
// components each on their own, ONE subtraction rounded in the tap's scalar type.  The build kernel and tests/arb_rates_ctaps_check.cpp
// run this text.
template <typename TAP> struct RatesTapPair { TAP re, im; };
template <typename TAP>
MRHIP_RATES_HD inline RatesTapPair<TAP> rates_cbank_pfb_value(const TAP *h, long long hLen, long long j)
{
    return j < hLen ? RatesTapPair<TAP>{h[2 * j], h[2 * j + 1]} : RatesTapPair<TAP>{TAP(0), TAP(0)};
}
template <typename TAP>
MRHIP_RATES_HD inline RatesTapPair<TAP> rates_cbank_dpfb_value(const TAP *h, long long hLen, long long j)
{
    return j + 1 < hLen ? RatesTapPair<TAP>{TAP(h[2 * j + 2] - h[2 * j]), TAP(h[2 * j + 3] - h[2 * j + 1])} : RatesTapPair<TAP>{TAP(0), TAP(0)};
}

// kernels_rates_arb_ctaps.hip.  The key must have complex_h and bank set; fused is not an argument: complex taps have no FUSED form.
hipError_t launch_arb_rates_ctaps_generic(const TypeKey &tk, const ArbArgs &a, const RatesArgs &r, hipStream_t s, const char **kname);
bool plan_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, ArbTileArgs *out, size_t *lds);   // (reads MRHIP_ARB_RATES_CTAPS_TILED)
// the tiled kernel's persistent grid (occupancy query, LDS attribute; MRHIP_ARB_RATES_CTAPS_GRID): everything about its launch that can
// fail ahead of the launch
hipError_t prepare_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbTileArgs &ta, size_t lds, int num_cus, long long *grid);
hipError_t launch_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, const RatesArgs &r, const ArbTileArgs &ta, size_t lds, long long grid,
                                        hipStream_t s, const char **kname);
// BankBuildArgs over pairs: h is [nch][hLen] (re, im) pairs in the tap's scalar type, pfb / dpfb [nch][Nphi*T] pairs of R; the row is
// staged in LDS when its hLen pairs fit kBankBuildLdsBytes
hipError_t launch_rates_cbank_build(bool tap_f64, bool r_f64, const BankBuildArgs &b, hipStream_t st);
// host_logic.cpp: the switch value passed in (0 never, 1 wherever the plan fits, -1 the default rule)
bool plan_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, int mode, ArbTileArgs *out, size_t *lds);

// ---- COMPLEX per-channel taps on the FIRFarrow filter with per-channel rates (mrhip_set_channel_ctaps_farrow, mrhip_set_channel_pnfb_ctaps,
// mrhip_set_channel_pnfb_ctaps_device; include/multirate_hip.h, "Complex per-channel taps with per-channel rates for FIRFarrow") ---------
// The filter holds nch polynomial banks of (re, im) pairs of Float64, [nch][T][polyorder+1][2], and TypeKey::complex_h and ::bank are both
// set.  Records, slices, schedule kernel, RatesArgs and rates_pnfb_install_kernel (over twice as many doubles: the rounding is per
// component) serve it unchanged; the two filter kernels live in kernels_rates_farrow_ctaps.hip (kernels_rates_farrow.hip refuses a
// complex_h key), the multi kernel's plan in host_logic.cpp.  Reported names: farrow_rates_ctaps_generic / farrow_rates_ctaps_multi;
// switches: MRHIP_FARROW_RATES_CTAPS_MULTI (-1 rule, 0, 1), MRHIP_FARROW_RATES_CTAPS_GRID.
//
// farrow_rates_ctaps_multi_kernel: a lane owns kFarrowRatesCtapsOPL outputs of one channel, output `tid` of as many consecutive runs of
// kVariantThreads outputs; a tile is those runs (tile_out = kFarrowRatesCtapsOPL * kVariantThreads outputs of one channel).  4, not 2:
// a slot carries two Float64 Horner chains and a complex sum, and both counts compile without scratch for every instantiation (at 4: 77
// to 105 VGPRs); measured, 4 is ahead of the universal kernel at 4096 ch x 1e4 and 2 is not.
constexpr int kFarrowRatesCtapsOPL = 4;
// the live slots of lane `tid` in the tile that starts at output k0: farrow_rates_live_slots with this kernel's slot count
MRHIP_RATES_HD inline int farrow_rates_ctaps_live_slots(long long k0, int tid, long long count)
{
    const long long left = count - k0 - tid;                     // outputs from the lane's first slot to the count
    if (left <= 0) return 0;
    const long long slots = (left + kVariantThreads - 1) / kVariantThreads;
    return slots < kFarrowRatesCtapsOPL ? static_cast<int>(slots) : kFarrowRatesCtapsOPL;
}

// kernels_rates_farrow_ctaps.hip.  The key must have complex_h and bank set; fused is not an argument: complex taps have no FUSED form.
hipError_t launch_farrow_rates_ctaps_generic(const TypeKey &tk, const FarrowArgs &a, const RatesArgs &r, hipStream_t s, const char **kname);
bool plan_farrow_rates_ctaps_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, ArbTileArgs *out);      // (reads MRHIP_FARROW_RATES_CTAPS_MULTI)
// the multi kernel's persistent grid (occupancy query; MRHIP_FARROW_RATES_CTAPS_GRID): everything about its launch that can fail ahead of
// the launch
hipError_t prepare_farrow_rates_ctaps_multi(const TypeKey &tk, const ArbTileArgs &ta, int num_cus, long long *grid);
hipError_t launch_farrow_rates_ctaps_multi(const TypeKey &tk, const FarrowArgs &a, const RatesArgs &r, const ArbTileArgs &ta, long long grid,
                                           hipStream_t s, const char **kname);
// host_logic.cpp: the switch value passed in (0 never, 1 every call, -1 the default rule); the grid is farrow_rates_multi_grid's
bool plan_farrow_rates_ctaps_multi(const TypeKey &tk, const FarrowArgs &a, int num_cus, int mode, ArbTileArgs *out);

// ---- The FIRFarrow fit on the device (mrhip_set_channel_taps_farrow_device, mrhip_set_channel_ctaps_farrow_device; include/multirate_hip.h,
// "The FIRFarrow fit on the device for the filters with per-channel rates") ---------------------------------------------------------------
// polyfit_rows (host_logic.cpp) is a Householder QR of the Vandermonde matrix A[r][p] = (r+1)^p, n = N𝜙 rows and m = polyorder+1 columns.
// A depends on (N𝜙, polyorder) alone, and neither the reflectors v_c, their vnorm2_c nor the triangle R depend on the right-hand side b:
// polyfit_factor runs that side ONCE, on the host, polyfit_apply the b side and the back substitution per row -- together the statements
// of polyfit_rows in their order, so the coefficients are polyfit_rows' bit for bit (every multiply, add and subtract rounded on its
// own: -ffp-contract=off; the two divisions IEEE Float64).  The table, Float64, column c at c * polyfit_table_pitch(n, m):
//     [0, n)      v_c[r] by the ROW r of A it belongs to (rows r < c: 0, never read)
//     [n]         vnorm2_c (0: polyfit_rows skips the column's reflection, and so does polyfit_apply)
//     [n+1+cc]    R[c][cc], cc = 0 ... m-1: row c of A after every reflection (the back substitution reads cc >= c)
// m * (n + m + 1) = (polyorder+1) * (N𝜙 + polyorder + 2) values.
MRHIP_RATES_HD inline long long polyfit_table_pitch(long long n, int m) { return n + m + 1; }
inline size_t polyfit_table_size(long long n, int m) { return static_cast<size_t>(m) * static_cast<size_t>(polyfit_table_pitch(n, m)); }
// host_logic.cpp: the A side of polyfit_rows, statement for statement; `table` receives polyfit_table_size(Nphi, polyorder+1) values.
// false exactly where polyfit_rows answers false (it does so for every b or for none): n < m, a zero column norm, a zero pivot.
bool polyfit_factor(int64_t Nphi, int polyorder, std::vector<double> *table);
// The b side of polyfit_rows and its back substitution.  b: the n values of the row, element r at b[r * b_stride], OVERWRITTEN; coef:
// the m coefficients, element c at coef[c * coef_stride].  coef may be b itself (coef[c] is written after the last read of b[c]): the
// kernel keeps both in the lane's LDS column, the host program passes two arrays.  The table entries are indexed by loop counters only.
MRHIP_RATES_HD inline void polyfit_apply(const double *table, long long n, int m, double *b, long long b_stride, double *coef, long long coef_stride)
{
    const long long pitch = polyfit_table_pitch(n, m);
    for (int c = 0; c < m; ++c) {
        const double *v = table + c * pitch;
        const double vnorm2 = v[n];
        if (vnorm2 == 0.0) continue;
        double dot = 0.0;
        for (long long r = c; r < n; ++r) dot += v[r] * b[r * b_stride];
        const double f = 2.0 * dot / vnorm2;
        for (long long r = c; r < n; ++r) b[r * b_stride] -= f * v[r];
    }
    for (int c = m - 1; c >= 0; --c) {
        const double *R = table + c * pitch + n + 1;
        double sacc = b[c * b_stride];
        for (int cc = c + 1; cc < m; ++cc) sacc -= R[cc] * coef[cc * coef_stride];
        coef[c * coef_stride] = sacc / R[c];
    }
}

// Row i of channel c's polyphase bank, the n = N𝜙 values one fit takes: element 𝜙 is the tap h_c[j], j = (T-1-i)*N𝜙 + 𝜙, 0 for j >= hLen
// -- rates_bank_tap_index at e = 𝜙*T + i (taps2pfb) --, so the row is CONTIGUOUS in the channel's taps from j0 on:
MRHIP_RATES_HD inline long long farrow_fit_row_start(long long i, long long T, long long Nphi) { return (T - 1 - i) * Nphi; }
// A lane's item, 0 <= item < nch * T * nc (nc = 1, or 2: the components of a complex tap), is (channel, row, component) with the component
// fastest; its coefficient k goes to the filter's banks, [nch][T][m] scalars or (re, im) pairs, at farrow_fit_dst_index -- the place
// create_farrow_banks gives it on the host.  The kernel and tests/rates_farrow_fit_check.cpp (over a guard-padded buffer) run this text.
struct FarrowFitItem { long long c, i; int comp; };
MRHIP_RATES_HD inline FarrowFitItem farrow_fit_item(long long item, long long T, int nc)
{
    const long long rows = T * nc, c = item / rows, rem = item - c * rows, i = rem / nc;
    return FarrowFitItem{c, i, static_cast<int>(rem - i * nc)};
}
MRHIP_RATES_HD inline long long farrow_fit_dst_index(const FarrowFitItem &it, int k, long long T, int m, int nc)
{
    return ((it.c * T + it.i) * m + k) * nc + it.comp;
}

// The launch: one lane per (channel, row i, component), the lane's b in LDS as b[r][lane] (consecutive lanes on consecutive 8-byte
// words), one wave a workgroup.  LDS per workgroup is lanes * N𝜙 * 8 bytes and stays within kFarrowFitLdsBytes (two workgroups a CU):
// 64 lanes up to N𝜙 = 128, then the largest power of two that fits, down to kFarrowFitMinLanes at N𝜙 = kFarrowFitNphiMax; a larger N𝜙
// is refused (an eighth of a wave at work and less is not worth a launch: the host call takes those).
constexpr int kFarrowFitMaxLanes = 64;
constexpr int kFarrowFitMinLanes = 8;
constexpr long long kFarrowFitLdsBytes = 64 * 1024;
constexpr long long kFarrowFitNphiMax = kFarrowFitLdsBytes / (8 * kFarrowFitMinLanes);      // 1024
struct FarrowFitPlan { int lanes; size_t lds_bytes; };
// host_logic.cpp: false: N𝜙 is refused (< 1, or above kFarrowFitNphiMax)
bool plan_rates_fit(int64_t Nphi, FarrowFitPlan *out);

struct FarrowFitArgs {             // rates_farrow_fit_kernel
    const void *h;                 // DEVICE, [nch][hLen] taps (TAP), or (re, im) pairs of TAP
    double *pnfb;                  // DEVICE, the filter's banks: [nch][T][m], or [nch][T][m] pairs
    long long hLen, T, Nphi;
    long long items;               // nch * T * components: one lane each
    int m;                         // polyorder + 1
};
// kernels_rates_farrow_fit.hip (tap_f64: the scalar type of h; complex_h: pairs; table: DEVICE, polyfit_factor's -- a kernel parameter of
// its own, so that it carries __restrict__ and its loads stay scalar)
hipError_t launch_rates_fit(bool tap_f64, bool complex_h, const FarrowFitArgs &a, const double *table, const FarrowFitPlan &p, hipStream_t st);

}  // namespace mrhip
