// host_logic.cpp -- data-independent bookkeeping of the filt! hot path.
//
// Everything here depends only on lengths and on the (phase, deficit) state, never on sample
// values, so the host can size buffers, pick grids and advance the stream state without ever
// reading back from the device.  At the end: the host side of the constructors
// (create.h) -- their checks and the filter banks, which depend on the arguments and the taps alone.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <cstring>
#include <vector>

#include "mrhip_internal.h"
#include "create.h"
#include "rates_arb.h"

namespace mrhip {

// Polyphase decomposition of the prototype filter.
// Behaviour to match: src/Filters.jl:284-298 -- tapsPerPhi = ceil(hLen/Nphi); the matrix is
// tapsPerPhi x Nphi, column-major; column p holds h[p], h[p+Nphi], ... REVERSED (so that a dot
// with a forward-running sample window is a convolution), zero padded past hLen.
// Formulation here: element (row r, col c), 0-based, is h[(T-1-r)*Nphi + c].
int64_t taps2pfb(const void *h, int64_t hLen, int th, int64_t Nphi, void *out)
{
    const int64_t T = (hLen + Nphi - 1) / Nphi;
    if (!out) return T;
    const size_t es = dtype_size(th);                 // (complex taps: an (re, im) pair moves as one element)
    auto *dst = static_cast<unsigned char *>(out);
    const auto *src = static_cast<const unsigned char *>(h);
    for (int64_t c = 0; c < Nphi; ++c) {
        for (int64_t r = 0; r < T; ++r) {
            const int64_t hi = (T - 1 - r) * Nphi + c;
            unsigned char *d = dst + static_cast<size_t>(c * T + r) * es;
            if (hi < hLen) std::memcpy(d, src + static_cast<size_t>(hi) * es, es);
            else std::memset(d, 0, es);
        }
    }
    return T;
}

// dh = [diff(h), 0] (src/Filters.jl:106), in the tap type: one subtraction per scalar, the components of a complex tap each on
// their own (Julia's Complex - Complex).  `dh` receives hLen elements of `th`.
void arbitrary_dh(const void *h, int64_t hLen, int th, void *dh)
{
    const int64_t nc = dtype_is_complex(th) ? 2 : 1;        // scalars per tap: h[i + 1] is nc scalars behind h[i]
    const int64_t n = hLen * nc;
    auto diff = [&](auto *d, const auto *s) {
        for (int64_t j = 0; j < n; ++j) d[j] = j + nc < n ? s[j + nc] - s[j] : 0;
    };
    if (dtype_is_f64(th)) diff(static_cast<double *>(dh), static_cast<const double *>(h));
    else diff(static_cast<float *>(dh), static_cast<const float *>(h));
}

// src/Filters.jl:433-439
int64_t nextphase(int64_t phase, int64_t L, int64_t M)
{
    const int64_t next = phase + M % L;
    return next > L ? next - L : next;
}

// src/Filters.jl:352-357.  The reference divides in Float64 and takes iceil; for every length
// that fits a double exactly (< 2^53) that equals the integer ceiling computed here.
int64_t outputlength_ratio(int64_t inputlength, int64_t L, int64_t M, int64_t initialPhi)
{
    const int64_t a = inputlength * L - initialPhi + 1;
    return a >= 0 ? (a + M - 1) / M : -((-a) / M);
}

// src/Filters.jl:396-401
int64_t inputlength_ratio(int64_t outputlength, int64_t L, int64_t M, int64_t initialPhi)
{
    const int64_t a = outputlength * M + initialPhi - 1;
    return a >= 0 ? (a + L - 1) / L : -((-a) / L);
}

// Closed form of the rational loop (src/Filters.jl:558-571): with u_k = (phi0-1) + k*M,
// output k uses phase u_k mod L and input index d0 + u_k div L, and exists while that index
// is <= xLen.  STANDARD and DECIMATOR are L == 1; INTERPOLATOR restarts at (phi, idx) = (1, 1)
// on every call (src/Filters.jl:500-501) and never carries a deficit.
CallPlan plan_rational(int kind, int64_t L, int64_t M, int64_t phiIdx, int64_t inputDeficit, int64_t xLen)
{
    CallPlan p;
    switch (kind) {
    case MRHIP_FIR_STANDARD:
        p.phi0 = 1; p.d0 = 1; p.n_out = xLen; p.phi_end = 1; p.d_end = 1;
        return p;
    case MRHIP_FIR_INTERPOLATOR:
        p.phi0 = 1; p.d0 = 1; p.n_out = L * xLen; p.phi_end = 1; p.d_end = 1;
        return p;
    default:
        break;
    }
    p.phi0 = (kind == MRHIP_FIR_DECIMATOR) ? 1 : phiIdx;
    p.d0 = inputDeficit;
    if (xLen < inputDeficit) {  // not enough input for a single output
        p.short_input = true;
        p.n_out = 0;
        p.phi_end = phiIdx;
        p.d_end = inputDeficit - xLen;
        return p;
    }
    p.n_out = outputlength_ratio(xLen - inputDeficit + 1, L, M, p.phi0);
    const int64_t u_end = (p.phi0 - 1) + p.n_out * M;
    p.phi_end = u_end % L + 1;
    p.d_end = p.d0 + u_end / L - xLen;
    return p;
}

// Grid of a persistent kernel: as many workgroups as the chip holds, at most one per tile, at least one.  bpc > 0 (a launcher's
// MRHIP_*_BPC knob): workgroups per CU -- it replaces the occupancy figure (bpc_replaces: opair, fir_stream, phase-stationary)
// or only lowers it (the pipe and lane kernels).  *per_cu is updated to the figure the grid was sized with.
long long persistent_grid_size(int *per_cu, int num_cus, long long total_tiles, int bpc, bool bpc_replaces)
{
    if (*per_cu < 1) *per_cu = 1;
    if (bpc > 0 && (bpc_replaces || bpc < *per_cu)) *per_cu = bpc;
    long long g = static_cast<long long>(num_cus) * *per_cu;
    if (g > total_tiles) g = total_tiles;
    return g < 1 ? 1 : g;
}

// rational_opair_kernel in six-wave workgroups: the fourth never fits next to three running ones (see kernels_rational_opair.hip),
// so a launch of more tiles than three rounds of the chip is sized with three per CU.  The step in front of pair_grid() at the
// one opair call site (MRHIP_OPAIR_BPC, where set, replaces the result).
int opair_six_wave_cap(int per_cu, int num_cus, unsigned total_steps, int J, unsigned block_x)
{
    if (per_cu < 1) per_cu = 1;
    const long long tiles = (static_cast<long long>(total_steps) + J - 1) / J;
    return block_x == 6 * 64 && per_cu > 3 && tiles > 3LL * num_cus * per_cu ? 3 : per_cu;
}

// Launch of a pair kernel (rational_opair, fir_stream, fir_stream_rt) from the workgroups a CU holds: grid, scheduling groups
// (workgroup b draws grabs of J steps from group b % ngroups), and whether the grabs are dealt without atomics (at most three
// tiles a workgroup).  multi_n > 0: independent streams -- group = stream, its workgroups deal its tiles round-robin
// (total_steps: the longest stream's).  ring: the resident consumer takes every workgroup the chip holds at once (workgroup 0:
// the feeder), at most grid_cap where that is > 1; its steps_per_group is the ring's own (ring_api.inc) and reported as 0 here.
PairGrid pair_grid(int per_cu, int num_cus, unsigned total_steps, int J, int max_groups, int multi_n, bool ring, int grid_cap)
{
    PairGrid p{};
    const long long chip = static_cast<long long>(num_cus) * per_cu;
    const long long tiles = (static_cast<long long>(total_steps) + J - 1) / J;
    long long g = chip;
    if (ring) {
        if (grid_cap > 1 && g > grid_cap) g = grid_cap;
    } else {
        if (g > static_cast<long long>(total_steps)) g = total_steps;
        if (g < 1) g = 1;
    }
    p.ngroups = static_cast<int>(g < max_groups ? g : max_groups);
    p.steps_per_group = ring ? 0u : static_cast<unsigned>((total_steps + p.ngroups - 1) / p.ngroups);
    p.static_grabs = tiles <= 3 * g;
    if (multi_n > 0) {
        long long w = chip / multi_n;
        if (w > tiles) w = tiles;
        if (w < 1) w = 1;
        g = w * multi_n;
        p.ngroups = multi_n;
        p.static_grabs = 1;
    }
    p.grid = g;
    return p;
}

// ---- plans of the LDS-tiled variant kernels (complex taps, per-channel taps) ----------------------------------------------------
// Two shapes (plan_variant_poly_tiled, plan_variant_arb_tiled) and under each the families' own eligibility with the value of
// the family's switch passed in (the kernel units read it: MRHIP_*_TILED = 0 never, 1 wherever the LDS plan fits -- tests,
// measurements -- unset (-1) the family's measured default rule).

namespace {
size_t variant_sample_bytes(const TypeKey &tk) { return (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1); }
size_t variant_tap_bytes(const TypeKey &tk) { return (tk.r_f64 ? 8 : 4) * (tk.complex_h ? 2 : 1); }     // complex taps: an (re, im) pair
}  // namespace

// Rational shape: ONE tap bank (the shared one, or one channel's) with a column pitch of T + 1 taps, at most 96 KB, plus the sample
// window of a tile of cpl channels fit the LDS budget (at most 150 KB); the tile shrinks from 256 outputs to 64 -- and, where
// channels per lane are searched (search_cpl: the shared complex bank; 4 from 32 channels, 2 from 8), cpl first -- until they do.
// By default (not forced) the call must give every CU a tile: below that the universal kernel's one-lane-per-output grid spreads
// wider than the tiles do.
bool plan_variant_poly_tiled(size_t tap_bytes, bool search_cpl, int L, int M, int T, long long n_out, int nch, size_t sample_bytes,
                             int num_cus, bool forced, ArbTileArgs *out, size_t *lds)
{
    const int TP = T + 1;
    const size_t bank_elems = static_cast<size_t>(L) * TP;
    const size_t bank_bytes = (bank_elems * tap_bytes + 15) / 16 * 16;
    if (bank_bytes > 96 * 1024) return false;
    int cpl = !search_cpl ? 1 : nch >= 32 ? 4 : (nch >= 8 ? 2 : 1);
    long long tile_out = kVariantThreads;
    // samples a tile of `t` outputs can touch: floor((u_first + (t-1)*M)/L) - floor(u_first/L) + T
    auto span_of = [&](long long t) { return ((t - 1) * M + L - 1) / L + T + 1; };
    const size_t budget = std::max<size_t>(64 * 1024, std::min<size_t>(bank_bytes + 40 * 1024, 150 * 1024));
    for (;;) {
        const long long max_span = span_of(tile_out);
        const size_t total = bank_bytes + static_cast<size_t>(max_span) * sample_bytes * cpl;
        if (total <= budget || (cpl == 1 && tile_out == 64)) {
            if (total > 150 * 1024 || max_span > (1 << 30)) return false;
            const long long groups = (nch + cpl - 1) / cpl;
            ArbTileArgs ta{};
            ta.tap_pitch = TP;
            ta.bank_elems = static_cast<int>(bank_elems);
            ta.x_offset_bytes = static_cast<int>(bank_bytes);
            ta.max_span = static_cast<int>(max_span);
            ta.tile_out = tile_out;
            ta.tiles_per_channel = (n_out + tile_out - 1) / tile_out;
            ta.total_tiles = ta.tiles_per_channel * groups;
            ta.cpl = cpl;
            if (!forced && ta.total_tiles < static_cast<long long>(num_cus)) return false;
            *out = ta;
            *lds = total;
            return true;
        }
        if (cpl > 1) cpl /= 2;
        else tile_out /= 2;
    }
}

// poly_ctaps_tiled_kernel: the shared bank of pairs, CPL channels a lane
bool plan_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.complex_h || a.dyn || a.n_out < 1 || a.T < 1) return false;
    return plan_variant_poly_tiled(variant_tap_bytes(tk), true, a.L, a.M, a.T, a.n_out, a.nch, variant_sample_bytes(tk), num_cus, mode == 1, out, lds);
}
// poly_bank_tiled_kernel: ONE channel's bank.  The default rule is the measured plan: with at least one tile per CU the tiled kernel
// was 1.12 ... 3.6 times faster in every row measured (profiles/r07/bank.txt); smaller calls are unmeasured
// and stay on the universal kernel.
bool plan_bank_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.bank || tk.complex_h || a.dyn || a.n_out < 1 || a.T < 1) return false;
    return plan_variant_poly_tiled(variant_tap_bytes(tk), false, a.L, a.M, a.T, a.n_out, a.nch, variant_sample_bytes(tk), num_cus, mode == 1, out, lds);
}
// poly_bank_ctaps_tiled_kernel: ONE channel's bank of pairs; with at least one tile per CU 1.48 ... 4.1 times faster in every row
// measured (profiles/r07/bank_ctaps.txt)
bool plan_bank_ctaps_tiled(const TypeKey &tk, const PolyArgs &a, int num_cus, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.bank || !tk.complex_h || a.dyn || a.n_out < 1 || a.T < 1) return false;
    return plan_variant_poly_tiled(variant_tap_bytes(tk), false, a.L, a.M, a.T, a.n_out, a.nch, variant_sample_bytes(tk), num_cus, mode == 1, out, lds);
}

// Arbitrary-rate shape (FIRArbitrary, FIRFarrow).  A tile is 256 outputs (a lane each) of cpl channels; beside what the kernel
// keeps in LDS anyway (v.fixed_bytes, at most v.fixed_max) the samples may take 40 KiB or what v.total_max leaves.  The planned span
// follows from the rate -- consecutive outputs are 1/rate samples apart -- and is CUT to that room: tiles with a longer run read global
// memory, so a rate that makes EVERY full tile such a tile is left to the universal kernel unless the kernel is forced.
bool plan_variant_arb_tiled(const ArbVariantShape &v, int T, long long n_out, int nch, size_t sample_bytes, double rate, bool forced,
                            ArbTileArgs *out, size_t *lds)
{
    if (v.fixed_bytes > v.fixed_max) return false;
    constexpr size_t kSampleBytesMax = 40 * 1024;
    const size_t room = std::min(kSampleBytesMax, v.total_max - v.fixed_bytes) / 16 * 16;
    const long long tile_out = kVariantThreads;
    // samples the run of a tile can hold: n advances by at most ceil(1/rate) + 1 per output (update(), Filters.jl:663-673, 780-788)
    const double per_tile = std::ceil(static_cast<double>(tile_out - 1) / rate) + static_cast<double>(T) + 2.0;
    int cpl = v.cpl_start;
    while (cpl > 1 && per_tile * static_cast<double>(sample_bytes * cpl) > static_cast<double>(room)) cpl /= 2;
    long long max_span = static_cast<long long>(room / (sample_bytes * cpl));
    const bool cut = per_tile > static_cast<double>(max_span);
    if (!cut) max_span = static_cast<long long>(per_tile);
    if (max_span < T + 1) return false;                                               // not even one window
    if (cut && !forced) return false;
    ArbTileArgs ta{};
    ta.cpl = cpl;
    ta.tap_pitch = v.tap_pitch;
    ta.bank_elems = v.bank_elems;
    ta.x_offset_bytes = static_cast<int>(v.fixed_bytes);
    ta.max_span = static_cast<int>(max_span);
    ta.tile_out = tile_out;
    ta.tiles_per_channel = (n_out + tile_out - 1) / tile_out;
    ta.total_tiles = v.tile_all_channels ? ta.tiles_per_channel : ta.tiles_per_channel * ((nch + cpl - 1) / cpl);
    *out = ta;
    *lds = v.fixed_bytes + static_cast<size_t>(max_span) * sample_bytes * cpl;
    return true;
}

// arb_ctaps_tiled_kernel: both banks of pairs (column pitch T + 1, at most 96 KiB) beside 40 KiB of samples.  CPL = 1 or 2: with
// four channels a lane -- lo and up of four complex sums beside both banks' pairs -- the compiler spills to scratch in every type
// combination.  The default rule: a tile per CU at least, and min_work (MRHIP_CTAPS_ARB_TILED_MIN) outputs x channels -- by default
// never (negative): profiles/r07/ctaps_arb.txt has the measurements that comes from.
bool plan_ctaps_arb_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, int mode, int min_work, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.complex_h || a.n_out < 1 || a.T < 1 || !(rate > 0.0)) return false;
    const int TP = a.T + 1;
    const size_t bank_pairs = static_cast<size_t>(a.Nphi) * TP;
    const size_t banks_bytes = (2 * bank_pairs * variant_tap_bytes(tk) + 15) / 16 * 16;
    const ArbVariantShape v{banks_bytes, 96 * 1024, (96 + 40) * 1024, TP, static_cast<int>(bank_pairs), a.nch >= 8 ? 2 : 1, false};
    ArbTileArgs ta;
    size_t bytes;
    if (!plan_variant_arb_tiled(v, a.T, a.n_out, a.nch, variant_sample_bytes(tk), rate, mode == 1, &ta, &bytes)) return false;
    if (mode != 1) {
        if (ta.total_tiles < static_cast<long long>(num_cus)) return false;
        if (min_work < 0 || a.n_out * static_cast<long long>(a.nch) < min_work) return false;
    }
    *out = ta;
    *lds = bytes;
    return true;
}

// arb_bank_tiled_kernel: both banks of ONE channel plus the sample tile fit LDS at two workgroups a CU (160 KiB a CU: 78 KiB a
// workgroup, which leaves room for the epilogue's own word).  The default rule: the tiled kernel was faster than the universal one by
// far more than the spread of the repeats in every measured call of 5312 tiles or more (1.4 ... 10 times: DESIGN.md 9 item 12,
// profiles/r07/arb_bank.txt) and was not at 664 and 166 tiles (calls bound by their launches).  So: from kArbBankTiledTilesPerCu tiles
// per CU (5120 tiles on 256 CUs; 5312 is the smallest measured call it won); everything smaller stays on the universal kernel.
constexpr long long kArbBankTiledTilesPerCu = 20;
bool plan_arb_bank_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.bank || tk.complex_h || a.n_out < 1 || a.T < 1 || a.Nphi < 1 || !(rate > 0.0)) return false;
    const int TP = a.T + 1;
    const size_t bank_elems = static_cast<size_t>(a.Nphi) * TP;
    const size_t banks_bytes = (2 * bank_elems * variant_tap_bytes(tk) + 15) / 16 * 16;
    const ArbVariantShape v{banks_bytes, 78 * 1024, 78 * 1024, TP, static_cast<int>(bank_elems), 1, false};
    ArbTileArgs ta;
    size_t bytes;
    if (!plan_variant_arb_tiled(v, a.T, a.n_out, a.nch, variant_sample_bytes(tk), rate, mode == 1, &ta, &bytes)) return false;
    if (mode != 1 && ta.total_tiles < kArbBankTiledTilesPerCu * static_cast<long long>(num_cus)) return false;
    *out = ta;
    *lds = bytes;
    return true;
}

// arb_rates_tiled_kernel (per-channel RATES, kernels_rates_arb.hip; either bank key): ONE pfb and dpfb (column pitch T + 1) -- the pair
// all channels share, or with per-channel TAPS (tk.bank) one channel's, the LDS geometry of plan_arb_bank_tiled -- plus the sample tile
// fit LDS at two workgroups a CU (78 KiB a workgroup, as for plan_arb_bank_tiled); one channel a lane (cpl = 1).  n_out is the call's
// bound (the counts are on the device): the tiling goes by it and the kernel skips the tiles at or behind a channel's count.  The span is
// planned for the SLOWEST channel (rate_min: its tiles have the longest runs) and cut to the room only when the kernel is forced; in the
// kernel every tile's run comes from its own channel's schedule, so a faster channel stages less and a tile longer than the planned span
// reads global memory.  The default rule (mode -1) takes the calls the measured rows cover, from kArbRatesTiledRule[tk.bank].min_tiles
// tiles, up to .max_per_channel tiles a channel, and never with a cut span; every other call stays on the universal kernel unless
// MRHIP_ARB_RATES_TILED=1 (shared taps) or MRHIP_ARB_RATES_BANK_TILED=1 (per-channel taps) forces the tiled one.  The two entries came
// out equal and rest on different measured rows:
//
// Shared taps (profiles/r09/arb_rates.txt; the figures of the run DESIGN.md quotes): the tiled kernel beat the
// universal one by far more than the spread of the repeats at 4096 ch x 1e4 (360 448 tiles of 88 a channel: 3.125 against 3.449 ms,
// spreads 0.04 and 0.03) and at 256 ch x 1e5 (225 024 tiles of 879 a channel: 21.45 against 26.44 ms, spreads 0.11 and 0.10), and did
// not at 64 ch x 1e6 (8790 tiles a channel: 536.8 against 548.3 ms with spreads of 26 and 6 -- the serial walk is the call).  Both limits
// are GUARDS ON UNMEASURED GROUND, not causes: nothing about 880 tiles a channel makes the tiled kernel worse (at 8790 it still read
// 1.02x, inside the spread, because the walk hides the filter kernel), and 256 ch x 1.001e5 falls back to the universal kernel only
// because no row was measured beyond 879.  A measurement of the filter kernels alone at long channels (kernel trace, the walk set aside)
// is what would let the cap go.
//
// Per-channel taps (profiles/r12/arb_rates_bank.txt, both runs): the tiled kernel beat the universal one by far
// more than the spread of the repeats at 4096 ch x 1e4 (360 448 tiles of 88 a channel: 2.804 against 3.105 ms and 2.797 against 3.122,
// spreads <= 0.053) and at 256 ch x 1e5 (225 024 tiles of 879 a channel: 18.101 against 23.016 ms and 18.119 against 23.027, spreads
// <= 0.035), and did not at 64 ch x 1e6 (8790 tiles a channel: 464.8 against 459.2 ms and 431.4 against 479.8 with spreads of 29 to 55
// -- the serial walk is the call).  As for shared taps both limits are GUARDS ON UNMEASURED GROUND, not causes: nothing about 880 tiles
// a channel makes the tiled kernel worse (at 8790 the rows cannot tell the kernels apart because the walk hides them), and a call of
// fewer tiles falls back only because no smaller row was measured.
struct RatesTiledRule { long long min_tiles, max_per_channel; };      // (a limit < 0 would mean: never)
constexpr RatesTiledRule kArbRatesTiledRule[2] = {{225024, 879}, {225024, 879}};       // [tk.bank]: shared taps, per-channel taps
bool plan_arb_rates_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int /*num_cus*/, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || tk.complex_h || a.n_out < 1 || a.T < 1 || a.Nphi < 1 || !(rate_min > 0.0)) return false;
    const int TP = a.T + 1;
    const size_t bank_elems = static_cast<size_t>(a.Nphi) * TP;
    const size_t banks_bytes = (2 * bank_elems * variant_tap_bytes(tk) + 15) / 16 * 16;
    const ArbVariantShape v{banks_bytes, 78 * 1024, 78 * 1024, TP, static_cast<int>(bank_elems), 1, false};
    ArbTileArgs ta;
    size_t bytes;
    if (!plan_variant_arb_tiled(v, a.T, a.n_out, a.nch, variant_sample_bytes(tk), rate_min, mode == 1, &ta, &bytes)) return false;
    const RatesTiledRule rule = kArbRatesTiledRule[tk.bank ? 1 : 0];
    if (mode != 1 && (rule.min_tiles < 0 || ta.total_tiles < rule.min_tiles || ta.tiles_per_channel > rule.max_per_channel)) return false;
    *out = ta;
    *lds = bytes;
    return true;
}

// arb_rates_ctaps_tiled_kernel (per-channel RATES with COMPLEX per-channel taps, kernels_rates_arb_ctaps.hip): both banks of ONE channel
// as (re, im) pairs of R (column pitch T + 1 pairs) plus the sample tile fit LDS at two workgroups a CU (78 KiB a workgroup, as for
// plan_arb_rates_tiled and plan_arb_bank_ctaps_tiled); one channel a lane (cpl = 1).  n_out is the call's bound, the tiling goes by it;
// the span is planned for the SLOWEST channel (rate_min) and cut to the room only when the kernel is forced -- everything as
// plan_arb_rates_tiled states it, with a pair where that has a tap.
//
// The default rule (mode -1), written the way kArbRatesTiledRule is, takes the calls the measured rows cover, from .min_tiles tiles, up
// to .max_per_channel tiles a channel, and never with a cut span; every other call stays on the universal kernel unless
// MRHIP_ARB_RATES_CTAPS_TILED=1 forces the tiled one.  The rows (profiles/r15/arb_rates_ctaps.txt, Complex64 taps,
// both runs): the tiled kernel beat the universal one by more than the spread of the repeats at 4096 ch x 1e4 Float32 (360 448 tiles
// of 88 a channel: 2.866 against 3.424 ms and 2.918 against 3.443, spreads <= 0.304), at the same shape with ComplexF32 samples (2.712
// against 3.689 ms and 2.731 against 3.671, spreads <= 0.026) and at 256 ch x 1e5 (225 024 tiles of 879 a channel: 18.353 against
// 23.052 ms and 18.336 against 23.001, spreads <= 0.110 but for one repeat of the universal kernel at 24.128), and did not at 64 ch x
// 1e6 (8790 tiles a channel: 498.5 against 515.3 ms and 481.5 against 484.3 with spreads of 23 to 45 -- the serial walk is the call).
// As for the real-tap kernels, whose limits came out the same, both are GUARDS ON UNMEASURED GROUND, not causes: the kernel trace of
// the same file has the tiled kernel ALONE at 2.76 ms against the universal one's 14.07 in the longest row (and 1.06 against 5.75 at
// 256 ch x 1e5), beside a walk of 519 ms (17.3 ms) -- nothing about 880 tiles a channel makes it worse, the rows only cannot show it.
constexpr RatesTiledRule kArbRatesCtapsTiledRule = {225024, 879};
bool plan_arb_rates_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int /*num_cus*/, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.bank || !tk.complex_h || a.n_out < 1 || a.T < 1 || a.Nphi < 1 || !(rate_min > 0.0)) return false;
    const int TP = a.T + 1;
    const size_t bank_pairs = static_cast<size_t>(a.Nphi) * TP;
    const size_t banks_bytes = (2 * bank_pairs * variant_tap_bytes(tk) + 15) / 16 * 16;
    const ArbVariantShape v{banks_bytes, 78 * 1024, 78 * 1024, TP, static_cast<int>(bank_pairs), 1, false};
    ArbTileArgs ta;
    size_t bytes;
    if (!plan_variant_arb_tiled(v, a.T, a.n_out, a.nch, variant_sample_bytes(tk), rate_min, mode == 1, &ta, &bytes)) return false;
    const RatesTiledRule rule = kArbRatesCtapsTiledRule;
    if (mode != 1 && (rule.min_tiles < 0 || ta.total_tiles < rule.min_tiles || ta.tiles_per_channel > rule.max_per_channel)) return false;
    *out = ta;
    *lds = bytes;
    return true;
}

// farrow_rates_multi_kernel (FIRFarrow with per-channel RATES, kernels_rates_farrow.hip; either bank key): no LDS -- the polynomial bank
// (the one, or with tk.bank the tile's channel's) is read as scalar operands, the windows from global memory -- so the plan is the
// tiling alone: a tile is kFarrowRatesOPL consecutive runs of kVariantThreads outputs of ONE channel, so one polynomial bank, one channel
// a lane (cpl = 1), and the tiling goes by n_out, the call's bound (the counts are on the device; the kernel skips the tiles and the
// slots at or behind a channel's count).  The default rule (mode -1) takes the calls the measured rows cover, from
// kFarrowRatesMultiRule[tk.bank].min_tiles tiles, up to .max_per_channel tiles a channel; every other call stays on the universal kernel
// unless MRHIP_FARROW_RATES_MULTI=1 (the one bank) or MRHIP_FARROW_RATES_BANK_MULTI=1 (a bank per channel) selects the multi kernel.
// The two entries came out equal and rest on different measured rows:
//
// The one bank (profiles/r10/farrow_rates.txt): the multi kernel beat the universal one by more than the spread of
// the repeats in both runs at 4096 ch x 1e4 (90 112 tiles of 22 a channel: 2.722 against 2.856 ms and 2.703 against 2.843, spreads
// <= 0.05), and did not at 256 ch x 1e5 (56 320 tiles of 220 a channel: 21.86 against 21.83 ms and 21.85 against 21.81) nor at 64 ch x
// 1e6 (140 672 tiles of 2198 a channel: 508.5 against 519.0 ms with spreads of 33 and 38) -- there the serial walk is the call.  As for
// plan_arb_rates_tiled both limits are GUARDS ON UNMEASURED GROUND, not causes.  The kernel trace of the same file says where the gain
// is: alone, the multi kernel took 0.584 ms against the universal one's 0.745 in the first row (8 taps per phase) and was level with it
// in the other two (32 taps per phase: 2.94 against 2.80 ms in the longest launches), where the walk is 95 % and more of the call anyway.
//
// A bank per channel (profiles/r13/farrow_rates_bank.txt, both runs): the multi kernel beat the universal one by
// far more than the spread of the repeats at 4096 ch x 1e4 (90 112 tiles of 22 a channel: 2.349 against 2.561 ms and 2.364 against
// 2.563, spreads <= 0.019) and did not at 256 ch x 1e5 (56 320 tiles of 220 a channel: 18.460 against 18.473 ms and 18.422 against
// 18.525, spreads 0.06 to 0.17) nor at 64 ch x 1e6 (140 672 tiles of 2198 a channel: 464.5 against 464.6 ms and 462.6 against 477.4 with
// spreads of 5 to 45 -- the serial walk is the call).  As for the one bank, whose limits came out the same, both are GUARDS ON
// UNMEASURED GROUND, not causes.  (A limit < 0 would mean: never.)
constexpr RatesTiledRule kFarrowRatesMultiRule[2] = {{90112, 22}, {90112, 22}};        // [tk.bank]: the one bank, a bank per channel
bool plan_farrow_rates_multi(const TypeKey &tk, const FarrowArgs &a, int /*num_cus*/, int mode, ArbTileArgs *out)
{
    if (mode == 0 || tk.complex_h || a.n_out < 1 || a.T < 1 || a.polyorder < 0 || a.nch < 1) return false;
    ArbTileArgs ta{};
    ta.cpl = 1;
    ta.tile_out = static_cast<long long>(kFarrowRatesOPL) * kVariantThreads;
    ta.tiles_per_channel = (a.n_out + ta.tile_out - 1) / ta.tile_out;
    ta.total_tiles = ta.tiles_per_channel * a.nch;
    const RatesTiledRule rule = kFarrowRatesMultiRule[tk.bank ? 1 : 0];
    if (mode != 1 && (rule.min_tiles < 0 || ta.total_tiles < rule.min_tiles || ta.tiles_per_channel > rule.max_per_channel)) return false;
    *out = ta;
    return true;
}

// its persistent grid: what the chip holds, no more workgroups than tiles, at least one; a test's replacement (MRHIP_FARROW_RATES_GRID,
// MRHIP_FARROW_RATES_BANK_GRID) may also ask for more workgroups than tiles (their runs are empty)
long long farrow_rates_multi_grid(long long total_tiles, long long chip_grid, int grid_fixed)
{
    if (grid_fixed > 0) return std::min<long long>(grid_fixed, 65535);
    return std::max<long long>(std::min<long long>(chip_grid, total_tiles), 1);
}

// farrow_rates_ctaps_multi_kernel (FIRFarrow with per-channel RATES and COMPLEX per-channel taps, kernels_rates_farrow_ctaps.hip): as for
// plan_farrow_rates_multi there is no LDS, so the plan is the tiling alone: a tile is kFarrowRatesCtapsOPL consecutive runs of
// kVariantThreads outputs of ONE channel (one polynomial bank of pairs, one channel a lane: cpl = 1), and the tiling goes by n_out, the
// call's bound (the kernel skips the tiles and the slots at or behind a channel's count).  mode 0: never; 1: every call; -1: the default
// rule, written the way kFarrowRatesMultiRule is -- from .min_tiles tiles, up to .max_per_channel tiles a channel; a limit < 0 would
// mean NEVER.  The rule admits the multi kernel only in rows where it was measured ahead of the universal one on the MI355X (DESIGN.md
// 9 item 26, profiles/r16/farrow_rates_ctaps.txt, Complex64 taps, both runs, four outputs a lane): ahead by more than the spread of the
// repeats at 4096 ch x 1e4 Float32 (90 112 tiles of 22 a channel: 2.549 against 2.713 ms and 2.525 against 2.704, spreads <= 0.057) and
// at the same shape with ComplexF32 samples (2.665 against 2.781 ms and 2.667 against 2.769, spreads <= 0.058); NOT ahead at 256 ch x
// 1e5 (56 320 tiles of 220 a channel: 19.022 against 18.990 ms and 19.055 against 18.992; ComplexF32: 19.352 against 19.164 and 19.361
// against 19.132 -- behind by more than the spread) nor at 64 ch x 1e6 (140 672 tiles of 2198 a channel: 463 to 536 ms either way with
// spreads of 13 to 52 -- the serial walk is the call).  The limits came out as kFarrowRatesMultiRule's and, as there, both are GUARDS
// ON UNMEASURED GROUND, not causes.  (With two outputs a lane the kernel was ahead nowhere: 2.710 against 2.728 ms and 2.692 against
// 2.701 in the first row, inside the spread, and behind in the second and third.)
constexpr RatesTiledRule kFarrowRatesCtapsMultiRule = {90112, 22};
bool plan_farrow_rates_ctaps_multi(const TypeKey &tk, const FarrowArgs &a, int /*num_cus*/, int mode, ArbTileArgs *out)
{
    if (mode == 0 || !tk.bank || !tk.complex_h || a.n_out < 1 || a.T < 1 || a.polyorder < 0 || a.nch < 1) return false;
    ArbTileArgs ta{};
    ta.cpl = 1;
    ta.tile_out = static_cast<long long>(kFarrowRatesCtapsOPL) * kVariantThreads;
    ta.tiles_per_channel = (a.n_out + ta.tile_out - 1) / ta.tile_out;
    ta.total_tiles = ta.tiles_per_channel * a.nch;
    const RatesTiledRule rule = kFarrowRatesCtapsMultiRule;
    if (mode != 1 && (rule.min_tiles < 0 || ta.total_tiles < rule.min_tiles || ta.tiles_per_channel > rule.max_per_channel)) return false;
    *out = ta;
    return true;
}

// arb_bank_ctaps_tiled_kernel: both banks of ONE channel as (re, im) pairs of R (column pitch T + 1) plus the sample tile fit LDS at
// two workgroups a CU (78 KiB a workgroup, as for plan_arb_bank_tiled); one channel a lane (cpl = 1); the span follows from the rate
// and is cut only when the kernel is forced.  The default rule: the tiled kernel was faster than the universal one by far more than
// the spread of the repeats in every measured call of 5312 tiles or more (profiles/r08/arb_bank_ctaps.txt:
// 6.6, 5.1 and 6.0 times at 64 ch x 1e6 -- 2.27 against 14.92 ms, 0.71 against 3.65, 2.73 against 16.26, spreads <= 0.16 ms -- 2.1
// times at 4096 ch x 1e4, 1.29 times at 64 ch x 1e4 = 5312 tiles: 0.052 against 0.068 ms, spread 0.001) and was not at 664 tiles
// (0.050 against 0.048 ms: a call bound by its launches).  So: from kArbBankCtapsTiledTilesPerCu tiles per CU (5120 tiles on 256
// CUs; 5312 is the smallest measured call it won); everything smaller stays on the universal kernel.
constexpr long long kArbBankCtapsTiledTilesPerCu = 20;
bool plan_arb_bank_ctaps_tiled(const TypeKey &tk, const ArbArgs &a, double rate, int num_cus, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.bank || !tk.complex_h || a.n_out < 1 || a.T < 1 || a.Nphi < 1 || !(rate > 0.0)) return false;
    const int TP = a.T + 1;
    const size_t bank_pairs = static_cast<size_t>(a.Nphi) * TP;
    const size_t banks_bytes = (2 * bank_pairs * variant_tap_bytes(tk) + 15) / 16 * 16;
    const ArbVariantShape v{banks_bytes, 78 * 1024, 78 * 1024, TP, static_cast<int>(bank_pairs), 1, false};
    ArbTileArgs ta;
    size_t bytes;
    if (!plan_variant_arb_tiled(v, a.T, a.n_out, a.nch, variant_sample_bytes(tk), rate, mode == 1, &ta, &bytes)) return false;
    if (mode != 1 && ta.total_tiles < kArbBankCtapsTiledTilesPerCu * static_cast<long long>(num_cus)) return false;
    *out = ta;
    *lds = bytes;
    return true;
}

// farrow_bank_tiled_kernel: LDS holds the sample run only (a tap feeds one product; the coefficients are scalar loads), at most 40 KiB:
// two workgroups a CU.  The default rule is NEVER: the tiled kernel beat the universal one nowhere by more than the spread of the
// repeats (profiles/r07/farrow_bank.txt: 0.76 ... 0.98 times its speed at Float32 samples, 166 ... 530 752 tiles;
// at 64 ch x 1e7 Float64, 2 618 048 tiles, 16.27 against 16.67 ms in one run and 16.68 against 16.80 with a spread of 0.46 in the
// next), so it stays behind its switch.
bool plan_farrow_bank_tiled(const TypeKey &tk, const FarrowArgs &a, double rate, int /*num_cus*/, int mode, ArbTileArgs *out, size_t *lds)
{
    if (mode != 1 || !tk.bank || tk.complex_h || a.n_out < 1 || a.T < 1 || a.polyorder < 0 || !(rate > 0.0)) return false;
    const ArbVariantShape v{0, 0, 40 * 1024, 0, 0, 1, false};
    return plan_variant_arb_tiled(v, a.T, a.n_out, a.nch, variant_sample_bytes(tk), rate, true, out, lds);
}

// farrow_ctaps_tiled_kernel: the coefficient bank of pairs of Float64, 256 tap columns of pairs of R and the samples fit the 160 KiB
// of a CU less the kernel's static words (159 KiB); a tile is every channel of its 256 outputs, CPL (1 or 2, as in
// arb_ctaps_tiled_kernel) channels at a time.  The default rule: only where the tiled kernel was measured, and faster than the
// universal one in every run (profiles/r07/ctaps_farrow.txt): Float32 arithmetic, 32 taps per phase, 1 to 64 channels, 21 230
// outputs a channel and more (83 tiles: fewer than the chip has CUs, and still ahead) -- min_out (MRHIP_CTAPS_FARROW_TILED_MIN;
// negative: never) is the smallest call measured.  Float64 arithmetic and other banks are not measured yet and stay on the
// universal kernel.
constexpr int kCtapsFarrowMeasuredT = 32;
bool plan_ctaps_farrow_tiled(const TypeKey &tk, const FarrowArgs &a, double rate, int /*num_cus*/, int mode, int min_out, ArbTileArgs *out, size_t *lds)
{
    if (mode == 0 || !tk.complex_h || a.n_out < 1 || a.T < 1 || a.polyorder < 0 || !(rate > 0.0)) return false;
    const size_t bank_pairs = static_cast<size_t>(a.T) * (a.polyorder + 1);
    const size_t bank_bytes = bank_pairs * 2 * sizeof(double);                          // (whole 16-byte units)
    const size_t col_bytes = static_cast<size_t>(a.T) * kVariantThreads * variant_tap_bytes(tk);
    const ArbVariantShape v{bank_bytes + col_bytes, 159 * 1024, 159 * 1024, 0, static_cast<int>(bank_pairs), a.nch >= 2 ? 2 : 1, true};
    ArbTileArgs ta;
    size_t bytes;
    if (!plan_variant_arb_tiled(v, a.T, a.n_out, a.nch, variant_sample_bytes(tk), rate, mode == 1, &ta, &bytes)) return false;
    if (mode != 1) {
        if (tk.r_f64 || a.T != kCtapsFarrowMeasuredT) return false;
        if (min_out < 0 || a.n_out < min_out) return false;
    }
    *out = ta;
    *lds = bytes;
    return true;
}

// FIRArbitrary / FIRFarrow: the phase accumulator is a serial Float64 recurrence whose roundings the reference's
// outputs depend on (src/Filters.jl:663-673), so it is evaluated here, in order, once per call; every channel shares
// the result.  One step of update():  acc += delta; if acc > N: xIdx += ifloor((acc-1)/N); acc = mod(acc-1, N) + 1.
//
// The loop is bound by the LATENCY of that dependent Float64 chain (add, -1, -N, +1), so the chain is shortened
// without changing a bit: with a1 = fl(acc + delta) and k = floor((a1-1)/N),
//     fl(fl(fl(a1 - 1) - k*N) + 1) == a1 - k*N   exactly,
// because 1 and N are multiples of ulp(a1) (a1 < 2^53), every intermediate is a multiple of ulp(a1) no larger in
// magnitude than a1, hence representable, hence each of the three operations is exact; and k = #{j >= 1 : a1 >= j*N + 1}
// (a1 - 1 >= j*N  <=>  a1 >= j*N + 1, both sides exact).  So the new accumulator is ONE exact subtraction away from a1,
// selected among a1, a1-N, a1-2N, a1-3N by comparisons.  The index step keeps the reference's expression (quotient
// rounded before the floor; for a power-of-two N it is exactly k).  Rates so low that a step spans four periods or
// more take the reference's expressions one by one (slow_step), OUTSIDE the hot loop: a call in the loop body makes
// the compiler keep the loop constants (and, through reference parameters, the accumulator) in memory -- 3x slower.
// Checked: schedule-dependent outputs and end state == oracle (a plain restatement) bit for bit
// (tests/test_gpu_parity.py::test_arbitrary_phase_recurrence_many_rates; 8e6 steps of a Python model of both forms).
namespace {

struct ArbConsts {
    double delta, N, invN;
    bool n_pow2;
    bool old_mod;      // mrhip_set_mod_form(f, 1) on a N𝜙 that is not a power of two: the plain loop below with mod() as older Julia Base versions computed it
    ArbConsts(double delta_, int64_t Nphi, int mod_form = 0) : delta(delta_), N(static_cast<double>(Nphi)), invN(1.0 / static_cast<double>(Nphi)),
                                             n_pow2((Nphi & (Nphi - 1)) == 0), old_mod(mod_form != 0 && (Nphi & (Nphi - 1)) != 0) {}
};

// update() (src/Filters.jl:663-673) one expression at a time, with mod(x, y) = rem(y + rem(x, y), y): the form Julia's Base used for
// floats before 0.4 -- the reference is Julia-0.3 code and nothing in its tree says which Base it ran on.  Identical to the exact
// remainder whenever N𝜙 is a power of two, so only other N𝜙 come here.
int64_t arb_run_old_mod(const ArbConsts &c, double &acc, int64_t &xIdx, int64_t xLen, int32_t *n_idx, double *acc_out, int64_t max_outputs)
{
    int64_t count = 0;
    while (xIdx <= xLen && count < max_outputs) {          // :717
        if (n_idx) n_idx[count] = static_cast<int32_t>(xIdx);
        if (acc_out) acc_out[count] = acc;
        ++count;
        acc += c.delta;                                      // :664
        if (acc > c.N) {
            const double am1 = acc - 1.0;
            xIdx += static_cast<int64_t>(std::floor(am1 / c.N));              // :667
            acc = std::fmod(c.N + std::fmod(am1, c.N), c.N) + 1.0;           // :668, old Base
        }
    }
    return count;
}

struct SlowStep { double acc; int64_t dx; };
__attribute__((noinline)) SlowStep arb_slow_step(double a1, double N, double invN, bool n_pow2)
{
    const double am1 = a1 - 1.0;
    const double qd = n_pow2 ? am1 * invN : am1 / N;   // exact scaling for a power of two; else the reference's division
    return SlowStep{std::fmod(am1, N) + 1.0,             // exact remainder of positive operands = mod()
                    static_cast<int64_t>(std::floor(qd))};
}

// Runs until xIdx > xLen, `max_outputs` entries were written, or a step needs the slow path (returned in *slow_a1,
// with the accumulator NOT yet advanced).  n_idx / acc_out may be null (count only).
template <bool POW2>
inline int64_t arb_hot_loop(const ArbConsts &c, double &acc_io, int64_t &xIdx_io, int64_t xLen, int32_t *n_idx, double *acc_out,
                            int64_t max_outputs, bool *need_slow, double *slow_a1)
{
    const double delta = c.delta, N = c.N, N2 = 2.0 * N, N3 = 3.0 * N;
    const double Np1 = N + 1.0, N2p1 = N2 + 1.0, N3p1 = N3 + 1.0, fast_limit = 4.0 * N + 1.0;
    double acc = acc_io;
    int64_t xIdx = xIdx_io, count = 0;
    *need_slow = false;
    while (xIdx <= xLen && count < max_outputs) {          // :717
        if (n_idx) n_idx[count] = static_cast<int32_t>(xIdx);
        if (acc_out) acc_out[count] = acc;
        ++count;
        const double a1 = acc + delta;                       // update(), :664
        if (__builtin_expect(!(a1 < fast_limit), 0)) { *need_slow = true; *slow_a1 = a1; break; }
        const double s1 = a1 - N, s2 = a1 - N2, s3 = a1 - N3;
        const bool w1 = a1 >= Np1, w2 = a1 >= N2p1, w3 = a1 >= N3p1;
        double nacc = a1;
        nacc = w1 ? s1 : nacc;
        nacc = w2 ? s2 : nacc;
        nacc = w3 ? s3 : nacc;
        if constexpr (POW2) xIdx += static_cast<int64_t>(w1) + static_cast<int64_t>(w2) + static_cast<int64_t>(w3);
        else if (a1 > N) xIdx += static_cast<int64_t>((a1 - 1.0) / N);   // :667: quotient rounded first; positive, so the cast floors
        acc = nacc;
    }
    acc_io = acc;
    xIdx_io = xIdx;
    return count;
}

// up to max_outputs schedule entries from (acc, xIdx); returns the number written
int64_t arb_run(const ArbConsts &c, double &acc, int64_t &xIdx, int64_t xLen, int32_t *n_idx, double *acc_out, int64_t max_outputs)
{
    if (c.old_mod) return arb_run_old_mod(c, acc, xIdx, xLen, n_idx, acc_out, max_outputs);
    int64_t count = 0;
    while (xIdx <= xLen && count < max_outputs) {
        bool need_slow = false;
        double a1 = 0.0;
        int32_t *pn = n_idx ? n_idx + count : nullptr;
        double *pa = acc_out ? acc_out + count : nullptr;
        count += c.n_pow2 ? arb_hot_loop<true>(c, acc, xIdx, xLen, pn, pa, max_outputs - count, &need_slow, &a1)
                          : arb_hot_loop<false>(c, acc, xIdx, xLen, pn, pa, max_outputs - count, &need_slow, &a1);
        if (need_slow) {                                     // the entry was written; finish its update() the slow way
            const SlowStep r = arb_slow_step(a1, c.N, c.invN, c.n_pow2);
            acc = r.acc;
            xIdx += r.dx;
        }
    }
    return count;
}

}  // namespace

int64_t run_arbitrary_schedule(ArbState &st, double delta, int64_t Nphi, int64_t xLen,
                               std::vector<int32_t> *n_idx, std::vector<double> *acc_out, int mod_form)
{
    if (xLen < st.inputDeficit) {          // src/Filters.jl:705-709
        st.inputDeficit -= xLen;
        return 0;
    }
    const ArbConsts c(delta, Nphi, mod_form);
    double acc = st.acc;
    int64_t xIdx = st.inputDeficit;        // :715
    int64_t count = 0;
    if (n_idx) n_idx->clear();
    if (acc_out) acc_out->clear();
    const int64_t chunk = 1 << 16;
    while (xIdx <= xLen) {
        if (n_idx) n_idx->resize(static_cast<size_t>(count + chunk));
        if (acc_out) acc_out->resize(static_cast<size_t>(count + chunk));
        count += arb_run(c, acc, xIdx, xLen, n_idx ? n_idx->data() + count : nullptr, acc_out ? acc_out->data() + count : nullptr, chunk);
    }
    if (n_idx) n_idx->resize(static_cast<size_t>(count));
    if (acc_out) acc_out->resize(static_cast<size_t>(count));
    st.acc = acc;
    st.phiIdx = static_cast<int64_t>(std::floor(acc));   // :671
    st.alpha = acc - static_cast<double>(st.phiIdx);     // :672
    st.xIdx = xIdx;
    st.inputDeficit = xIdx - xLen;         // :734
    return count;
}

// The same recurrence, resumable: continues from (st.acc, st.xIdx) and writes at most `max_outputs` schedule
// entries into raw buffers (the caller's pinned staging memory); *done is set once xIdx has passed xLen, at which
// point st holds the call-end state exactly as run_arbitrary_schedule leaves it.  Lets filt! overlap the serial
// host recurrence of one long call with the kernels of the pieces already scheduled.
int64_t run_arbitrary_schedule_piece(ArbState &st, double delta, int64_t Nphi, int64_t xLen, int32_t *n_idx, double *acc_out,
                                     int64_t max_outputs, bool *done, int mod_form)
{
    const ArbConsts c(delta, Nphi, mod_form);
    double acc = st.acc;
    int64_t xIdx = st.xIdx;
    const int64_t count = arb_run(c, acc, xIdx, xLen, n_idx, acc_out, max_outputs);
    st.acc = acc;
    st.xIdx = xIdx;
    *done = xIdx > xLen;
    if (*done) {
        st.phiIdx = static_cast<int64_t>(std::floor(acc));
        st.alpha = acc - static_cast<double>(st.phiIdx);
        st.inputDeficit = xIdx - xLen;
    }
    return count;
}

// Un-rounded phase after k steps of the recurrence from acc_p (double-double product, folded onto [1, N+1)): what the
// device schedule (kernels_schedule.hip: sched_anchor) predicts segment starts with.  The host uses it to measure how far
// the true accumulator drifted from it over a run it evaluated itself.
double sched_anchor_host(const SchedPlan &c, double acc_p, double k)
{
    const double hi = k * c.delta;
    const double lo = std::fma(k, c.delta, -hi);
    const double w = std::floor(((acc_p - 1.0) + hi) / c.N);
    double r = ((acc_p - 1.0) + (hi - w * c.N)) + lo;
    if (r < 0.0) r += c.N;
    else if (r >= c.N) r -= c.N;
    return r + 1.0;
}

// polyfit(y, polyorder), src/support.jl:85-88: A = [x^p for x in 1:n, p = 0:polyorder]; coefficients = A \ y,
// i.e. the least-squares solution Julia computes by a QR factorisation of A in Float64.  Restated as a
// Householder QR (the reference pins no bits here: SURVEY.md 8c -- LAPACK's blocked QR and this one agree
// to rounding).  Returns false when the system is rank deficient (n < polyorder+1).
bool polyfit_rows(const double *y, int64_t n, int polyorder, double *coef)
{
    const int m = polyorder + 1;
    if (n < m || m < 1) return false;
    std::vector<double> A(static_cast<size_t>(n) * m), b(y, y + n);
    for (int64_t r = 0; r < n; ++r) {
        double v = 1.0;
        for (int c = 0; c < m; ++c) { A[static_cast<size_t>(r) * m + c] = v; v *= static_cast<double>(r + 1); }
    }
    for (int c = 0; c < m; ++c) {                     // Householder reflections, column by column
        double norm = 0.0;
        for (int64_t r = c; r < n; ++r) norm += A[static_cast<size_t>(r) * m + c] * A[static_cast<size_t>(r) * m + c];
        norm = std::sqrt(norm);
        if (norm == 0.0) return false;
        const double akk = A[static_cast<size_t>(c) * m + c];
        const double alpha = akk > 0 ? -norm : norm;
        std::vector<double> v(static_cast<size_t>(n - c));
        v[0] = akk - alpha;
        for (int64_t r = c + 1; r < n; ++r) v[static_cast<size_t>(r - c)] = A[static_cast<size_t>(r) * m + c];
        double vnorm2 = 0.0;
        for (double t : v) vnorm2 += t * t;
        if (vnorm2 == 0.0) continue;
        for (int cc = c; cc < m; ++cc) {
            double dot = 0.0;
            for (int64_t r = c; r < n; ++r) dot += v[static_cast<size_t>(r - c)] * A[static_cast<size_t>(r) * m + cc];
            const double f = 2.0 * dot / vnorm2;
            for (int64_t r = c; r < n; ++r) A[static_cast<size_t>(r) * m + cc] -= f * v[static_cast<size_t>(r - c)];
        }
        double dot = 0.0;
        for (int64_t r = c; r < n; ++r) dot += v[static_cast<size_t>(r - c)] * b[static_cast<size_t>(r)];
        const double f = 2.0 * dot / vnorm2;
        for (int64_t r = c; r < n; ++r) b[static_cast<size_t>(r)] -= f * v[static_cast<size_t>(r - c)];
    }
    for (int c = m - 1; c >= 0; --c) {                // back substitution on the upper-triangular R
        double sacc = b[static_cast<size_t>(c)];
        for (int cc = c + 1; cc < m; ++cc) sacc -= A[static_cast<size_t>(c) * m + cc] * coef[cc];
        const double d = A[static_cast<size_t>(c) * m + c];
        if (d == 0.0) return false;
        coef[c] = sacc / d;
    }
    return true;
}

// The A side of polyfit_rows above, statement for statement, without a right-hand side (rates_arb.h, "The FIRFarrow fit on the
// device"): the reflector of every column, its vnorm2 and, at the end, the triangle go into the table polyfit_apply reads.  A zero
// column norm and a zero pivot answer false here as they do there -- neither depends on b.
bool polyfit_factor(int64_t n, int polyorder, std::vector<double> *table)
{
    const int m = polyorder + 1;
    if (n < m || m < 1) return false;
    const size_t pitch = static_cast<size_t>(polyfit_table_pitch(n, m));
    table->assign(polyfit_table_size(n, m), 0.0);
    std::vector<double> A(static_cast<size_t>(n) * m);
    for (int64_t r = 0; r < n; ++r) {
        double v = 1.0;
        for (int c = 0; c < m; ++c) { A[static_cast<size_t>(r) * m + c] = v; v *= static_cast<double>(r + 1); }
    }
    for (int c = 0; c < m; ++c) {                     // Householder reflections, column by column
        double norm = 0.0;
        for (int64_t r = c; r < n; ++r) norm += A[static_cast<size_t>(r) * m + c] * A[static_cast<size_t>(r) * m + c];
        norm = std::sqrt(norm);
        if (norm == 0.0) return false;
        const double akk = A[static_cast<size_t>(c) * m + c];
        const double alpha = akk > 0 ? -norm : norm;
        std::vector<double> v(static_cast<size_t>(n - c));
        v[0] = akk - alpha;
        for (int64_t r = c + 1; r < n; ++r) v[static_cast<size_t>(r - c)] = A[static_cast<size_t>(r) * m + c];
        double vnorm2 = 0.0;
        for (double t : v) vnorm2 += t * t;
        if (vnorm2 == 0.0) continue;                  // (the table's vnorm2 stays 0: polyfit_apply skips the column as well)
        for (int cc = c; cc < m; ++cc) {
            double dot = 0.0;
            for (int64_t r = c; r < n; ++r) dot += v[static_cast<size_t>(r - c)] * A[static_cast<size_t>(r) * m + cc];
            const double f = 2.0 * dot / vnorm2;
            for (int64_t r = c; r < n; ++r) A[static_cast<size_t>(r) * m + cc] -= f * v[static_cast<size_t>(r - c)];
        }
        double *col = table->data() + static_cast<size_t>(c) * pitch;
        for (int64_t r = c; r < n; ++r) col[r] = v[static_cast<size_t>(r - c)];
        col[n] = vnorm2;
    }
    for (int c = m - 1; c >= 0; --c) {                // the upper-triangular R of the back substitution
        if (A[static_cast<size_t>(c) * m + c] == 0.0) return false;
        for (int cc = 0; cc < m; ++cc) (*table)[static_cast<size_t>(c) * pitch + static_cast<size_t>(n) + 1 + cc] = A[static_cast<size_t>(c) * m + cc];
    }
    return true;
}

// the fit kernel's launch (rates_arb.h, plan_rates_fit): the lanes of a workgroup whose b columns, N𝜙 Float64 each, fit kFarrowFitLdsBytes
bool plan_rates_fit(int64_t Nphi, FarrowFitPlan *out)
{
    if (Nphi < 1 || Nphi > kFarrowFitNphiMax) return false;
    int lanes = kFarrowFitMaxLanes;
    while (static_cast<long long>(lanes) * Nphi * 8 > kFarrowFitLdsBytes) lanes /= 2;
    out->lanes = lanes;
    out->lds_bytes = static_cast<size_t>(lanes) * static_cast<size_t>(Nphi) * 8;
    return true;
}

// ---- the constructors' host side (create.h; the device work is create.hip's) --------------------------------------------------------

Refusal create_check_args(const CreateEntry &e, const void *h, int64_t hLen, int th, int tx, int64_t nch, mrhip_filter **out)
{
    if (e.hint) {            // an entry point with a tap-class refusal of its own gives it first, whatever else is wrong
        if (out) *out = nullptr;
        if (e.taps == kTapsReal && (th == MRHIP_C64 || th == MRHIP_C128))
            return {MRHIP_ERR_UNSUPPORTED, std::string(e.name) + " takes Float32 / Float64 taps (" + e.hint + ")"};
        if (e.taps == kTapsComplex && (th == MRHIP_F32 || th == MRHIP_F64))
            return {MRHIP_ERR_INVALID_ARG, std::string(e.name) + " takes Complex64 / Complex128 taps; real taps: " + e.hint};
    }
    if (!out) return {MRHIP_ERR_INVALID_ARG, "out is NULL"};
    *out = nullptr;
    if (!h || hLen < 1) return {MRHIP_ERR_INVALID_ARG, "h must hold at least one tap"};
    if (th < MRHIP_F32 || th > MRHIP_C128) return {MRHIP_ERR_INVALID_ARG, "bad tap dtype"};
    if (dtype_is_complex(th) && e.taps == kTapsReal)     // (a text older than the *_ctaps constructors: DESIGN.md, known)
        return {MRHIP_ERR_UNSUPPORTED, "complex taps are supported by the rational family only (mrhip_create_rational: FIRStandard, FIRDecimator, "
                                       "FIRInterpolator, FIRRational); FIRArbitrary and FIRFarrow take Float32 or Float64 taps"};
    if (tx < MRHIP_F32 || tx > MRHIP_C128) return {MRHIP_ERR_INVALID_ARG, "bad sample dtype"};
    if (nch < 1) return {MRHIP_ERR_INVALID_ARG, "nchannels must be >= 1"};
    return {};
}

Refusal check_channel_rates(const double *rates, int64_t nch, double *rate_max)
{
    if (!rates) return {MRHIP_ERR_INVALID_ARG, "rates is NULL"};
    *rate_max = 0.0;
    for (int64_t c = 0; c < nch; ++c) {
        if (!(rates[c] > 0.0) || !std::isfinite(rates[c])) return {MRHIP_ERR_INVALID_ARG, "rate must be greater than 0 (every channel's, and finite)"};
        // (update() advances xIdx by about 1/rate a step; the walk carries that advance in 32 bits: sched_step.h)
        if (rates[c] < 1.0 / static_cast<double>(1LL << 30)) return {MRHIP_ERR_UNSUPPORTED, "a per-channel rate below 2^-30"};
        *rate_max = std::max(*rate_max, rates[c]);
    }
    return {};
}

// mrhip_set_channel_taps (the public header, "Per-channel taps with per-channel rates for FIRArbitrary"): what the call refuses
// before it touches the device, in its order -- the filter (is_rates: of a *_rates constructor; is_farrow), then h, hLen and the tap type
// against the filter's own (f_hLen, f_th)
Refusal check_channel_taps(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th)
{
    if (is_rates && is_farrow)
        return {MRHIP_ERR_UNSUPPORTED, "mrhip_set_channel_taps: FIRFarrow with per-channel taps and per-channel rates is not this call's (it needs the fit of "
                                       "every row): mrhip_set_channel_taps_farrow or mrhip_set_channel_pnfb; mrhip_create_arbitrary_rates filters take this call"};
    if (!is_rates) return {MRHIP_ERR_INVALID_ARG, "mrhip_set_channel_taps takes a filter of mrhip_create_arbitrary_rates"};
    if (!h) return {MRHIP_ERR_INVALID_ARG, "mrhip_set_channel_taps: h is NULL"};
    if (hLen != f_hLen)
        return {MRHIP_ERR_INVALID_ARG, "mrhip_set_channel_taps: hLen must be the filter's (" + std::to_string(f_hLen) + " taps a channel; got " +
                                       std::to_string(hLen) + "): tapsPerPhi, the history length and the history do not change"};
    if (th < MRHIP_F32 || th > MRHIP_C128) return {MRHIP_ERR_INVALID_ARG, "mrhip_set_channel_taps: bad tap dtype"};
    if (dtype_is_complex(th)) return {MRHIP_ERR_UNSUPPORTED, std::string("mrhip_set_channel_taps: ") + kRatesHint + " (the taps are Float32 / Float64)"};
    if (th != f_th) return {MRHIP_ERR_INVALID_ARG, "mrhip_set_channel_taps: the taps must have the filter's tap dtype"};
    return {};
}

// mrhip_set_channel_ctaps and mrhip_set_channel_ctaps_device (`who`; the public header, "Complex per-channel taps with per-channel rates
// for FIRArbitrary"): what the two calls refuse before they touch the device, in their order and each naming the function -- the filter
// (a FIRFarrow one with per-channel rates is status 5: left out), then h, hLen against the filter's, the tap type (out of range, real,
// the other complex precision: f_th is the filter's tap type, real or already complex -- its precision counts), and last the filter's
// numerics: complex taps have no FUSED form
Refusal check_channel_ctaps(const char *who_, bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th, bool fused)
{
    const std::string who = who_;
    if (is_rates && is_farrow) return {MRHIP_ERR_UNSUPPORTED, who + ": complex taps with per-channel rates for FIRFarrow are left out"};
    if (!is_rates) return {MRHIP_ERR_INVALID_ARG, who + " takes a filter of mrhip_create_arbitrary_rates"};
    if (!h) return {MRHIP_ERR_INVALID_ARG, who + ": h is NULL"};
    if (hLen != f_hLen)
        return {MRHIP_ERR_INVALID_ARG, who + ": hLen must be the filter's (" + std::to_string(f_hLen) + " taps a channel; got " + std::to_string(hLen) +
                                       "): tapsPerPhi, the history length and the history do not change"};
    if (th < MRHIP_F32 || th > MRHIP_C128) return {MRHIP_ERR_INVALID_ARG, who + ": bad tap dtype"};
    if (!dtype_is_complex(th))
        return {MRHIP_ERR_INVALID_ARG, who + ": the taps must be Complex64 or Complex128 (real taps go through mrhip_set_channel_taps" +
                                       (who.ends_with("_device") ? "_device)" : ")")};
    if (dtype_is_f64(th) != dtype_is_f64(f_th))
        return {MRHIP_ERR_INVALID_ARG, who + ": the taps must be the complex type of the filter's tap precision (Complex64 on Float32 taps, Complex128 on Float64 taps)"};
    if (fused) return {MRHIP_ERR_UNSUPPORTED, who + ": the filter is in FUSED numerics and no FUSED form is defined for complex taps (the public header: complex taps)"};
    return {};
}

// mrhip_set_channel_taps_farrow and mrhip_set_channel_pnfb (the public header, "Per-channel taps with per-channel rates for FIRFarrow"):
// what the two calls refuse before they touch the device, in their order and each naming the function -- the filter (a FIRArbitrary one
// with per-channel rates is pointed to its own call), then h / pnfb, then hLen or (tapsPerPhi, polyorder) against the filter's own, then
// (taps only) the tap type: out of range, complex, the other real one
namespace {
// (`who`: the function's name; arb_call: the call a filter of mrhip_create_arbitrary_rates is pointed to)
Refusal farrow_taps_checks(const std::string &who, const char *arb_call, bool pnfb_call, bool is_rates, bool is_farrow, const void *src, int64_t len,
                           int64_t polyorder, int th, int64_t f_len, int64_t f_polyorder, int f_th)
{
    if (is_rates && !is_farrow) return {MRHIP_ERR_INVALID_ARG, who + ": a filter of mrhip_create_arbitrary_rates takes " + arb_call};
    if (!is_rates || !is_farrow) return {MRHIP_ERR_INVALID_ARG, who + " takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb"};
    if (!src) return {MRHIP_ERR_INVALID_ARG, who + (pnfb_call ? ": pnfb is NULL" : ": h is NULL")};
    if (pnfb_call) {
        if (len != f_len || polyorder != f_polyorder)
            return {MRHIP_ERR_INVALID_ARG, who + ": tapsPerPhi and polyorder must be the filter's (" + std::to_string(f_len) + " polynomials of order " +
                                           std::to_string(f_polyorder) + " a channel; got " + std::to_string(len) + " of order " + std::to_string(polyorder) +
                                           "): the history length and the history do not change"};
        return {};
    }
    if (len != f_len)
        return {MRHIP_ERR_INVALID_ARG, who + ": hLen must be the filter's (" + std::to_string(f_len) + " taps a channel; got " + std::to_string(len) +
                                       "): tapsPerPhi, the history length and the history do not change"};
    if (th < MRHIP_F32 || th > MRHIP_C128) return {MRHIP_ERR_INVALID_ARG, who + ": bad tap dtype"};
    if (dtype_is_complex(th)) return {MRHIP_ERR_UNSUPPORTED, who + ": " + kRatesHint + " (the taps are Float32 / Float64)"};
    if (th != f_th) return {MRHIP_ERR_INVALID_ARG, who + ": the taps must have the filter's tap dtype"};
    return {};
}
}  // namespace

Refusal check_channel_taps_farrow(bool pnfb_call, bool is_rates, bool is_farrow, const void *src, int64_t len, int64_t polyorder, int th,
                                  int64_t f_len, int64_t f_polyorder, int f_th)
{
    return farrow_taps_checks(pnfb_call ? "mrhip_set_channel_pnfb" : "mrhip_set_channel_taps_farrow", "mrhip_set_channel_taps", pnfb_call, is_rates,
                              is_farrow, src, len, polyorder, th, f_len, f_polyorder, f_th);
}

// mrhip_set_channel_taps_farrow_device (the public header, "The FIRFarrow fit on the device for the filters with per-channel rates"): the
// checks of mrhip_set_channel_taps_farrow in their order, in the new function's name; a FIRArbitrary filter is pointed to
// mrhip_set_channel_taps_device
Refusal check_channel_taps_farrow_device(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th)
{
    return farrow_taps_checks("mrhip_set_channel_taps_farrow_device", "mrhip_set_channel_taps_device", false, is_rates, is_farrow, h, hLen, 0, th, f_hLen, 0, f_th);
}

// mrhip_set_channel_ctaps_farrow (pnfb_call false: src = h, len = hLen against the filter's hLen, th against the complex type of the
// filter's tap precision), mrhip_set_channel_pnfb_ctaps and mrhip_set_channel_pnfb_ctaps_device (pnfb_call true: src = pnfb, len =
// tapsPerPhi and polyorder against the filter's; th is not looked at) -- `who`; the public header, "Complex per-channel taps with
// per-channel rates for FIRFarrow": what the three calls refuse before they touch the device, in their order and each naming the
// function -- the filter (a FIRArbitrary one with per-channel rates is pointed to its own call), then h / pnfb, then hLen or
// (tapsPerPhi, polyorder) against the filter's own, then (taps only) the tap type (out of range, real, the other complex precision:
// f_th is the filter's tap type, real or already complex -- its precision counts), and last the filter's numerics: complex taps have no
// FUSED form
namespace {
// (arb_call: the call a filter of mrhip_create_arbitrary_rates is pointed to; real_call: the call real taps are pointed to)
Refusal farrow_ctaps_checks(const std::string &who, const char *arb_call, const char *real_call, bool pnfb_call, bool is_rates, bool is_farrow,
                            const void *src, int64_t len, int64_t polyorder, int th, int64_t f_len, int64_t f_polyorder, int f_th, bool fused)
{
    if (is_rates && !is_farrow) return {MRHIP_ERR_INVALID_ARG, who + ": a filter of mrhip_create_arbitrary_rates takes " + arb_call};
    if (!is_rates || !is_farrow) return {MRHIP_ERR_INVALID_ARG, who + " takes a filter of mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb"};
    if (!src) return {MRHIP_ERR_INVALID_ARG, who + (pnfb_call ? ": pnfb is NULL" : ": h is NULL")};
    if (pnfb_call) {
        if (len != f_len || polyorder != f_polyorder)
            return {MRHIP_ERR_INVALID_ARG, who + ": tapsPerPhi and polyorder must be the filter's (" + std::to_string(f_len) + " polynomials of order " +
                                           std::to_string(f_polyorder) + " a channel; got " + std::to_string(len) + " of order " + std::to_string(polyorder) +
                                           "): the history length and the history do not change"};
    } else {
        if (len != f_len)
            return {MRHIP_ERR_INVALID_ARG, who + ": hLen must be the filter's (" + std::to_string(f_len) + " taps a channel; got " + std::to_string(len) +
                                           "): tapsPerPhi, the history length and the history do not change"};
        if (th < MRHIP_F32 || th > MRHIP_C128) return {MRHIP_ERR_INVALID_ARG, who + ": bad tap dtype"};
        if (!dtype_is_complex(th))
            return {MRHIP_ERR_INVALID_ARG, who + ": the taps must be Complex64 or Complex128 (real taps go through " + real_call + ")"};
        if (dtype_is_f64(th) != dtype_is_f64(f_th))
            return {MRHIP_ERR_INVALID_ARG, who + ": the taps must be the complex type of the filter's tap precision (Complex64 on Float32 taps, Complex128 on Float64 taps)"};
    }
    if (fused) return {MRHIP_ERR_UNSUPPORTED, who + ": the filter is in FUSED numerics and no FUSED form is defined for complex taps (the public header: complex taps)"};
    return {};
}
}  // namespace

Refusal check_channel_ctaps_farrow(const char *who, bool pnfb_call, bool is_rates, bool is_farrow, const void *src, int64_t len, int64_t polyorder,
                                   int th, int64_t f_len, int64_t f_polyorder, int f_th, bool fused)
{
    return farrow_ctaps_checks(who, "mrhip_set_channel_ctaps", "mrhip_set_channel_taps_farrow", pnfb_call, is_rates, is_farrow, src, len, polyorder, th,
                               f_len, f_polyorder, f_th, fused);
}

// mrhip_set_channel_ctaps_farrow_device: the checks of mrhip_set_channel_ctaps_farrow in their order, in the new function's name; a
// FIRArbitrary filter is pointed to mrhip_set_channel_ctaps_device, real taps to mrhip_set_channel_taps_farrow_device
Refusal check_channel_ctaps_farrow_device(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th, bool fused)
{
    return farrow_ctaps_checks("mrhip_set_channel_ctaps_farrow_device", "mrhip_set_channel_ctaps_device", "mrhip_set_channel_taps_farrow_device", false,
                               is_rates, is_farrow, h, hLen, 0, th, f_hLen, 0, f_th, fused);
}

// mrhip_set_channel_rates_device: the host cannot see the rates, so the caller declares the range they lie in; the range is held to what
// check_channel_rates holds every rate to (finite, > 0, not below 2^-30), since the bound and the plans are sized for its two ends
Refusal check_channel_rates_device(bool is_rates, bool rates_is_null, double rate_lo, double rate_hi)
{
    const std::string who = "mrhip_set_channel_rates_device";
    if (!is_rates) return {MRHIP_ERR_INVALID_ARG, who + " takes a filter of mrhip_create_arbitrary_rates or mrhip_create_farrow_rates"};
    if (rates_is_null) return {MRHIP_ERR_INVALID_ARG, who + ": rates is NULL"};
    if (!std::isfinite(rate_lo) || !std::isfinite(rate_hi) || !(rate_lo > 0.0) || !(rate_hi > 0.0))
        return {MRHIP_ERR_INVALID_ARG, who + ": rate_lo and rate_hi must be finite and greater than 0"};
    if (rate_hi < rate_lo) return {MRHIP_ERR_INVALID_ARG, who + ": rate_hi < rate_lo"};
    if (rate_lo < 1.0 / static_cast<double>(1LL << 30)) return {MRHIP_ERR_UNSUPPORTED, who + ": a per-channel rate below 2^-30 (rate_lo)"};
    return {};
}

Refusal check_channel_taps_device(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th)
{
    if (is_rates && is_farrow)
        return {MRHIP_ERR_UNSUPPORTED, "mrhip_set_channel_taps_device: the fit of a FIRFarrow filter's rows on the device is left out: "
                                       "mrhip_set_channel_pnfb_device takes fitted banks; mrhip_create_arbitrary_rates filters take this call"};
    return check_channel_taps(is_rates, is_farrow, h, hLen, th, f_hLen, f_th);
}

Refusal check_channel_pnfb_device(bool is_rates, bool is_farrow, const void *pnfb, int64_t tapsPerPhi, int64_t polyorder, int64_t f_T,
                                  int64_t f_polyorder, int f_th)
{
    if (is_rates && !is_farrow)
        return {MRHIP_ERR_INVALID_ARG, "mrhip_set_channel_pnfb_device: a filter of mrhip_create_arbitrary_rates takes mrhip_set_channel_taps_device"};
    return check_channel_taps_farrow(true, is_rates, is_farrow, pnfb, tapsPerPhi, polyorder, f_th, f_T, f_polyorder, f_th);
}

Refusal check_ragged_lengths(const int64_t *x_lens, int64_t nch, bool x_is_null, int64_t x_stride, int64_t *len_max)
{
    if (!x_lens) return {MRHIP_ERR_INVALID_ARG, "mrhip_filt_device_rates_ragged: x_lens is NULL"};
    *len_max = 0;
    for (int64_t c = 0; c < nch; ++c) {
        if (x_lens[c] < 0) return {MRHIP_ERR_INVALID_ARG, "mrhip_filt_device_rates_ragged: negative length (every channel's must be >= 0)"};
        if (x_lens[c] >= 0x7fffffffLL)
            return {MRHIP_ERR_UNSUPPORTED, "mrhip_filt_device_rates_ragged: a call takes fewer than 2^31-1 samples per channel"};
        *len_max = std::max(*len_max, x_lens[c]);
    }
    if (*len_max > 0 && x_is_null) return {MRHIP_ERR_INVALID_ARG, "mrhip_filt_device_rates_ragged: x is NULL"};
    if (nch > 1 && x_stride < *len_max) return {MRHIP_ERR_INVALID_ARG, "mrhip_filt_device_rates_ragged: x_stride < the largest of x_lens"};
    return {};
}

Refusal check_device_lengths(const char *who, bool lens_is_null, int64_t len_max, bool x_is_null, int64_t nch, int64_t x_stride)
{
    const std::string w(who);
    const bool chained = w == "mrhip_filt_device_rates_chained";
    const char *name = chained ? "x_len_bound" : "x_len_max";
    if (lens_is_null) return {MRHIP_ERR_INVALID_ARG, w + ": x_lens is NULL"};
    if (len_max < 0) return {MRHIP_ERR_INVALID_ARG, w + ": negative " + name + " (the declared maximum of the lengths must be >= 0)"};
    if (len_max >= 0x7fffffffLL) return {MRHIP_ERR_UNSUPPORTED, w + ": a call takes fewer than 2^31-1 samples per channel"};
    if (len_max > 0 && x_is_null) return {MRHIP_ERR_INVALID_ARG, w + ": x is NULL"};
    if (nch > 1 && x_stride < len_max) return {MRHIP_ERR_INVALID_ARG, w + ": x_stride < " + name};
    return {};
}

Refusal check_rates_chain(bool f_is_rates, bool same_filter, bool prev_is_rates, int64_t f_nch, int64_t prev_nch, int f_device, int prev_device,
                          int f_tx, int prev_ty, bool prev_called, bool prev_dev_planned)
{
    const std::string w("mrhip_filt_device_rates_chained");
    if (!f_is_rates) return {MRHIP_ERR_INVALID_ARG, w + " takes a filter of mrhip_create_arbitrary_rates or mrhip_create_farrow_rates"};
    if (same_filter) return {MRHIP_ERR_INVALID_ARG, w + ": prev is the filter itself"};
    if (f_nch != prev_nch) return {MRHIP_ERR_INVALID_ARG, w + ": the two filters have different numbers of channels"};
    if (f_device != prev_device) return {MRHIP_ERR_INVALID_ARG, w + ": the two filters live on different devices"};
    if (f_tx != prev_ty) return {MRHIP_ERR_INVALID_ARG, w + ": the filter's sample dtype is not the previous filter's output dtype"};
    if (prev_is_rates && !prev_called)
        return {MRHIP_ERR_INVALID_ARG, w + ": the previous filter has not been called since its creation or mrhip_reset: its records hold no call's counts"};
    if (!prev_is_rates && !prev_dev_planned)
        return {MRHIP_ERR_INVALID_ARG, w + ": the previous filter's latest call was not planned on the device (mrhip_filt_device_async, or a call "
                                           "under capture): its count is not in its call record"};
    return {};
}

Refusal create_check_params(const CreateEntry &e, int64_t hLen, int64_t nch, CreateParams *p)
{
    if (e.family == kCreateRational) {
        if (p->num < 1 || p->den < 1) return {MRHIP_ERR_INVALID_ARG, "ratio must be positive"};
        int64_t g = p->num, r = p->den;                  // gcd
        while (r) { const int64_t t = g % r; g = r; r = t; }
        p->L = p->num / g; p->M = p->den / g;
        if (p->L > 0x7fffffff || p->M > 0x7fffffff || hLen > 0x7fffffff)
            return {MRHIP_ERR_INVALID_ARG, "L, M and hLen must fit in 31 bits"};
        return {};
    }
    if (e.rates) {
        if (Refusal r = check_channel_rates(p->rates, nch, &p->rate)) return r;
    } else if (!(p->rate > 0.0)) {
        return {MRHIP_ERR_INVALID_ARG, "rate must be greater than 0"};
    }
    if (p->Nphi < 1 || p->Nphi > 0x7fffffff || hLen > 0x7fffffff) return {MRHIP_ERR_INVALID_ARG, "bad Nphi"};
    if (e.family != kCreateFarrow) return {};
    if (e.pnfb) {            // a caller-fitted bank: nothing is fitted, so Nphi does not bound the order
        if (p->polyorder < 0 || p->polyorder > 32) return {MRHIP_ERR_INVALID_ARG, "polyorder must be in 0..32"};
    } else if (p->polyorder < 0 || p->polyorder > 32 || p->polyorder + 1 > p->Nphi) {
        return {MRHIP_ERR_INVALID_ARG, "polyorder must be in 0..min(32, Nphi-1)"};
    }
    return {};
}

int64_t create_pfb_banks(const void *h, int64_t hLen, int th, int64_t Nphi, size_t rows, std::vector<unsigned char> *pfb, std::vector<unsigned char> *dpfb)
{
    const size_t es = dtype_size(th);
    const int64_t T = taps2pfb(h, hLen, th, Nphi, nullptr);
    const size_t bank_bytes = static_cast<size_t>(T) * static_cast<size_t>(Nphi) * es;
    pfb->resize(bank_bytes * rows);
    if (dpfb) dpfb->resize(bank_bytes * rows);
    std::vector<unsigned char> dh(dpfb ? static_cast<size_t>(hLen) * es : 0);
    for (size_t r = 0; r < rows; ++r) {                  // (Nphi == 1: one column, reversed == flipud)
        const unsigned char *hr = static_cast<const unsigned char *>(h) + r * static_cast<size_t>(hLen) * es;
        taps2pfb(hr, hLen, th, Nphi, pfb->data() + r * bank_bytes);
        if (!dpfb) continue;
        arbitrary_dh(hr, hLen, th, dh.data());          // dh = [diff(h), 0] in the tap type (Filters.jl:106)
        taps2pfb(dh.data(), hLen, th, Nphi, dpfb->data() + r * bank_bytes);
    }
    return T;
}

// The Vandermonde matrix of the fit is real, so the least-squares fit of a complex row is the fit of its real parts and the fit of its
// imaginary parts: one loop over the nc components of a tap.
bool create_farrow_banks(const void *h, int64_t hLen, int th, int64_t Nphi, int64_t polyorder, size_t rows, std::vector<double> *pn)
{
    const size_t es = dtype_size(th), nc = dtype_is_complex(th) ? 2 : 1, np = static_cast<size_t>(polyorder + 1);
    const int64_t T = taps2pfb(h, hLen, th, Nphi, nullptr);
    pn->resize(rows * static_cast<size_t>(T) * np * nc);
    std::vector<unsigned char> pfb(static_cast<size_t>(T) * Nphi * es);
    std::vector<double> row(static_cast<size_t>(Nphi)), fit(np);
    for (size_t r = 0; r < rows; ++r) {
        taps2pfb(static_cast<const unsigned char *>(h) + r * static_cast<size_t>(hLen) * es, hLen, th, Nphi, pfb.data());   // column-major T x Nphi
        double *bank = pn->data() + r * static_cast<size_t>(T) * np * nc;
        for (int64_t i = 0; i < T; ++i)
            for (size_t comp = 0; comp < nc; ++comp) {
                for (int64_t c = 0; c < Nphi; ++c) {     // element (row i, column c) of the bank
                    const size_t s = static_cast<size_t>(c * T + i) * nc + comp;
                    row[static_cast<size_t>(c)] = dtype_is_f64(th) ? reinterpret_cast<const double *>(pfb.data())[s]
                                                                   : static_cast<double>(reinterpret_cast<const float *>(pfb.data())[s]);
                }
                if (!polyfit_rows(row.data(), Nphi, static_cast<int>(polyorder), fit.data())) return false;
                for (size_t j = 0; j < np; ++j) bank[(static_cast<size_t>(i) * np + j) * nc + comp] = fit[j];
            }
    }
    return true;
}

}  // namespace mrhip
