// rates_arb.h -- FIRArbitrary with PER-CHANNEL RATES (mrhip_create_arbitrary_rates; include/multirate_hip.h, "Per-channel rates for
// FIRArbitrary"): what api.hip, host_logic.cpp (the tiled kernel's plan) and kernels_rates_arb.hip (the three kernels) share.  Kept out
// of mrhip_internal.h so that only those units depend on it.
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
    long long pad;
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
};

struct RatesArgs {                 // beside ArbArgs (whose n_idx / acc are the bases of the slices, n_out the call's bound, dyn NULL)
    const RateChannel *rec;
    long long slice;
};

// kernels_rates_arb.hip
hipError_t launch_rates_schedule(const RatesSchedArgs &s, bool pow2, hipStream_t st);
hipError_t launch_rates_reset(RateChannel *rec, int nch, hipStream_t st);                  // constructor state, in stream order
hipError_t launch_arb_rates_generic(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, hipStream_t s, const char **kname);
bool plan_arb_rates_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, ArbTileArgs *out, size_t *lds);
// the tiled kernel's persistent grid (occupancy query, LDS attribute): everything about its launch that can fail ahead of the launch
hipError_t prepare_arb_rates_tiled(const TypeKey &tk, bool fused, const ArbTileArgs &ta, size_t lds, int num_cus, long long *grid);
hipError_t launch_arb_rates_tiled(const TypeKey &tk, bool fused, const ArbArgs &a, const RatesArgs &r, const ArbTileArgs &ta, size_t lds,
                                  long long grid, hipStream_t s, const char **kname);
// host_logic.cpp: the switch value passed in (MRHIP_ARB_RATES_TILED: 0 never, 1 wherever the plan fits, -1 the default rule)
bool plan_arb_rates_tiled(const TypeKey &tk, const ArbArgs &a, double rate_min, int num_cus, int mode, ArbTileArgs *out, size_t *lds);

}  // namespace mrhip
