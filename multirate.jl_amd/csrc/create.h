// create.h -- what the sixteen mrhip_create_* constructors (create.hip) are made of that makes no HIP call: the description of an entry
// point, its argument and parameter checks and the host-side bank building.  All of it is in host_logic.cpp, as pure functions, so the
// stand-alone check programs under tests/ run it on the CPU (tests/create_check.cpp).
#pragma once

#include <string_view>

#include "mrhip_internal.h"

namespace mrhip {

enum CreateFamily { kCreateRational, kCreateArbitrary, kCreateFarrow };
enum CreateTaps { kTapsReal, kTapsComplex, kTapsEither };

// One entry point, as data.  `hint` != NULL: the entry point has a tap-class refusal of its own, given BEFORE every other check (and
// *out is cleared first, where out is not NULL): real-only ones answer MRHIP_ERR_UNSUPPORTED with "<name> takes Float32 / Float64 taps
// (<hint>)", complex-only ones MRHIP_ERR_INVALID_ARG with "<name> takes Complex64 / Complex128 taps; real taps: <hint>" -- there the hint
// is the sibling's name.  hint == NULL: complex taps, where not accepted, get the generic text of create_check_args after the h / hLen
// and dtype checks.
struct CreateEntry {
    CreateFamily family;
    CreateTaps taps;             // tap class accepted
    bool bank, rates, pnfb;      // `h` holds nch rows / nch rates behind the one bank / `h` is a caller-fitted polynomial bank (no fit)
    const char *name, *hint;
};
inline constexpr const char *kRatesHint = "complex taps with per-channel rates are left out";
inline constexpr CreateEntry kCreateEntries[] = {
    //                                         bank   rates  pnfb
    {kCreateRational,  kTapsEither,  false, false, false, "mrhip_create_rational", nullptr},
    {kCreateRational,  kTapsReal,    true,  false, false, "mrhip_create_rational_bank", "complex taps in a bank are not supported"},
    {kCreateRational,  kTapsComplex, true,  false, false, "mrhip_create_rational_bank_ctaps", "mrhip_create_rational_bank"},
    {kCreateArbitrary, kTapsReal,    false, false, false, "mrhip_create_arbitrary", nullptr},
    {kCreateArbitrary, kTapsComplex, false, false, false, "mrhip_create_arbitrary_ctaps", "mrhip_create_arbitrary"},
    {kCreateArbitrary, kTapsReal,    true,  false, false, "mrhip_create_arbitrary_bank", "complex taps in a FIRArbitrary bank are left out"},
    {kCreateArbitrary, kTapsComplex, true,  false, false, "mrhip_create_arbitrary_bank_ctaps", "mrhip_create_arbitrary_bank"},
    {kCreateArbitrary, kTapsReal,    false, true,  false, "mrhip_create_arbitrary_rates", kRatesHint},
    {kCreateFarrow,    kTapsReal,    false, false, false, "mrhip_create_farrow", nullptr},
    {kCreateFarrow,    kTapsReal,    true,  false, false, "mrhip_create_farrow_bank",
     "complex taps in a FIRFarrow bank are left out of this entry point: mrhip_create_farrow_bank_ctaps"},
    {kCreateFarrow,    kTapsReal,    false, false, true,  "mrhip_create_farrow_pnfb", nullptr},
    {kCreateFarrow,    kTapsReal,    false, true,  false, "mrhip_create_farrow_rates", kRatesHint},
    {kCreateFarrow,    kTapsReal,    false, true,  true,  "mrhip_create_farrow_rates_pnfb", kRatesHint},
    {kCreateFarrow,    kTapsComplex, false, false, false, "mrhip_create_farrow_ctaps", "mrhip_create_farrow"},
    {kCreateFarrow,    kTapsComplex, true,  false, false, "mrhip_create_farrow_bank_ctaps", "mrhip_create_farrow_bank"},
    {kCreateFarrow,    kTapsComplex, false, false, true,  "mrhip_create_farrow_pnfb_ctaps", "mrhip_create_farrow_pnfb"},
};
// the row of an entry point; in a constant expression (as create.hip uses it) a name the table does not hold does not compile
constexpr const CreateEntry &create_entry(std::string_view name)
{
    for (const CreateEntry &e : kCreateEntries)
        if (name == e.name) return e;
    throw "no such entry point";
}

// What differs between the families' signatures.  In: num / den, or rate or rates, Nphi, polyorder.  create_check_params leaves the
// reduced ratio in L / M and, with per-channel rates, the largest rate in `rate`.
struct CreateParams {
    int64_t num = 1, den = 1;
    double rate = 0.0;
    const double *rates = nullptr;
    int64_t Nphi = 1, polyorder = 0;
    int64_t L = 1, M = 1;
};

// What a check answers: MRHIP_OK, or the status and the text of mrhip_last_error -- as a value, so that nothing here touches the
// library's error state (the caller hands it to fail()).
struct Refusal {
    int status = MRHIP_OK;
    std::string message;
    explicit operator bool() const { return status != MRHIP_OK; }
};

// (a) the checks in front of the device query: out, h / hLen, the dtypes, the tap class, nch
Refusal create_check_args(const CreateEntry &e, const void *h, int64_t hLen, int th, int tx, int64_t nch, mrhip_filter **out);
// (b) the checks behind the device checks: ratio and the 31-bit limits; rate or rates, then Nphi, then (FIRFarrow) polyorder
Refusal create_check_params(const CreateEntry &e, int64_t hLen, int64_t nch, CreateParams *p);
// the rate checks of the constructors with per-channel rates and of mrhip_set_channel_rates; *rate_max: the largest rate
Refusal check_channel_rates(const double *rates, int64_t nch, double *rate_max);
// the checks of mrhip_set_channel_taps that need no device: the filter's kind, h, hLen and the tap type against the filter's own
Refusal check_channel_taps(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th);
// the checks of mrhip_set_channel_ctaps and mrhip_set_channel_ctaps_device (`who`: the function's name) that need no device, in their
// order: the filter's kind, h, hLen, the tap type against the complex type of the filter's tap precision (f_th: real, or complex after
// an earlier call), and the filter's numerics (fused: complex taps have no FUSED form)
Refusal check_channel_ctaps(const char *who, bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th, bool fused);
// the checks of mrhip_set_channel_ctaps_farrow (pnfb_call false: src = h, len = hLen, th the tap type), mrhip_set_channel_pnfb_ctaps and
// mrhip_set_channel_pnfb_ctaps_device (pnfb_call true: src = pnfb, len = tapsPerPhi; th is not looked at) that need no device, in their
// order (`who`: the function's name): the filter's kind, src, the lengths against the filter's, the tap type against the complex type of
// the filter's tap precision (f_th: real, or complex after an earlier call), and the filter's numerics (fused: no FUSED form)
Refusal check_channel_ctaps_farrow(const char *who, bool pnfb_call, bool is_rates, bool is_farrow, const void *src, int64_t len, int64_t polyorder,
                                   int th, int64_t f_len, int64_t f_polyorder, int f_th, bool fused);
// the same for mrhip_set_channel_taps_farrow (pnfb_call false: src = h, len = hLen against the filter's hLen, th against its tap type)
// and mrhip_set_channel_pnfb (pnfb_call true: src = pnfb, len = tapsPerPhi and polyorder against the filter's; th is not looked at)
Refusal check_channel_taps_farrow(bool pnfb_call, bool is_rates, bool is_farrow, const void *src, int64_t len, int64_t polyorder, int th,
                                  int64_t f_len, int64_t f_polyorder, int f_th);
// the length checks of mrhip_filt_device_rates_ragged, in its order: x_lens itself, every length (negative, then 2^31-1 and above), x
// against the largest length, x_stride against it for nch > 1; *len_max: the largest length (what the call's bound is taken from)
Refusal check_ragged_lengths(const int64_t *x_lens, int64_t nch, bool x_is_null, int64_t x_stride, int64_t *len_max);
// Lengths the host never sees (the public header, "Input lengths from device memory, and chaining, for the filters with per-channel rates"):
// the checks of check_ragged_lengths with the declared maximum in the place of the largest length, in the same order and in the name of
// `who` (mrhip_filt_device_rates_lens_device: x_len_max; mrhip_filt_device_rates_chained: x_len_bound, and lens_is_null false): the
// lengths' pointer, the maximum (negative, then 2^31-1 and above), x against it, x_stride against it for nch > 1
Refusal check_device_lengths(const char *who, bool lens_is_null, int64_t len_max, bool x_is_null, int64_t nch, int64_t x_stride);
// what mrhip_filt_device_rates_chained refuses about the pair (f, prev) ahead of the length checks, in its order: f without per-channel
// rates, prev == f, the channel counts, the devices, f's sample dtype against prev's output dtype; then a prev with per-channel rates that
// no call has moved since creation or reset, or a one-state prev whose latest call was not planned on the device
Refusal check_rates_chain(bool f_is_rates, bool same_filter, bool prev_is_rates, int64_t f_nch, int64_t prev_nch, int f_device, int prev_device,
                          int f_tx, int prev_ty, bool prev_called, bool prev_dev_planned);
// The device-resident updates (the public header, "Device-resident updates for the filters with per-channel rates"): what the three calls
// refuse before they look at the stream, each in its own name.
// mrhip_set_channel_rates_device: f is a filter with per-channel rates, rates is there, and the declared range [rate_lo, rate_hi]
Refusal check_channel_rates_device(bool is_rates, bool rates_is_null, double rate_lo, double rate_hi);
// mrhip_set_channel_taps_device: a FIRFarrow filter is pointed to mrhip_set_channel_pnfb_device, then check_channel_taps unchanged
Refusal check_channel_taps_device(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th);
// mrhip_set_channel_pnfb_device: a FIRArbitrary filter is pointed to mrhip_set_channel_taps_device, then check_channel_taps_farrow(true, ...)
Refusal check_channel_pnfb_device(bool is_rates, bool is_farrow, const void *pnfb, int64_t tapsPerPhi, int64_t polyorder, int64_t f_T,
                                  int64_t f_polyorder, int f_th);
// The FIRFarrow fit on the device (the public header, "The FIRFarrow fit on the device for the filters with per-channel rates"): what the
// two calls refuse before they look at the plan, the fit's rank or the stream, each in its own name.
// mrhip_set_channel_taps_farrow_device: check_channel_taps_farrow(false, ...) with a FIRArbitrary filter pointed to mrhip_set_channel_taps_device
Refusal check_channel_taps_farrow_device(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th);
// mrhip_set_channel_ctaps_farrow_device: check_channel_ctaps_farrow(who, false, ...) with a FIRArbitrary filter pointed to
// mrhip_set_channel_ctaps_device and real taps to mrhip_set_channel_taps_farrow_device
Refusal check_channel_ctaps_farrow_device(bool is_rates, bool is_farrow, const void *h, int64_t hLen, int th, int64_t f_hLen, int f_th, bool fused);
// (c) the banks, `rows` tap vectors of hLen taps each, one bank per row, one after the other.  taps2pfb of every row into pfb and
// (dpfb != NULL: FIRArbitrary) of its dh = [diff(h), 0] into dpfb; returns tapsPerPhi
int64_t create_pfb_banks(const void *h, int64_t hLen, int th, int64_t Nphi, size_t rows, std::vector<unsigned char> *pfb, std::vector<unsigned char> *dpfb);
// FIRFarrow: pfb = taps2pfb(row, Nphi) and one polynomial per row of it (Filters.jl:139-140, :315-318), per component for complex taps,
// into pn, [rows][T][polyorder+1] scalars or (re, im) pairs.  false: a fit is rank deficient.
bool create_farrow_banks(const void *h, int64_t hLen, int th, int64_t Nphi, int64_t polyorder, size_t rows, std::vector<double> *pn);

}  // namespace mrhip
