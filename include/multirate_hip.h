/*
 * multirate_hip.h -- C ABI of libmultirate_hip.so, the MI355X (gfx950) engine behind
 * Multirate.jl's FIRFilter / filt / filt! hot path.
 *
 * The reference (JayKickliter/Multirate.jl) has no FFI boundary: its seam is Julia
 * multiple dispatch on
 *     filt!(buffer::Vector{Tb}, self::FIRFilter{K{Th}}, x::Vector{Tx})
 * (src/Filters.jl:450,489,536,598,693) reached through filt(self, x)
 * (src/Filters.jl:475,519,577,633,744) and filt(h, x, ratio|rate)
 * (src/Filters.jl:858,864).  Each entry point below names the reference
 * interface it replaces.  The Julia-side binding is in
 * multirate.jl_amd/julia/MultirateHIP.jl and described in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross the boundary
 *   - every function returns an mrhip_status (0 = ok) unless noted;
 *     mrhip_last_error() returns the message of the calling thread's last failure
 *     (the reference raises Julia error("...") in the same places)
 *   - complex samples are interleaved (re, im) pairs (Julia Complex{T} layout)
 *   - a filter object carries `nchannels` independent streams that share taps and
 *     the data-independent state (phase index, input deficit, phase accumulator)
 *     and own one history vector each: the batched form of the reference's
 *     one-Vector-per-FIRFilter model (SURVEY.md 8b "Batch")
 *   - channel c of a signal buffer starts at base + c * stride (stride in SAMPLES,
 *     not bytes): planar layout, the layout of a Julia Matrix with one channel per column
 *   - lengths are per channel, in samples
 *   - a handle is a mutable stream object exactly like the reference's FIRFilter:
 *     not to be used from two threads at once
 */
#ifndef MULTIRATE_HIP_H
#define MULTIRATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRHIP_ABI_VERSION 1

typedef enum {
    MRHIP_OK = 0,
    MRHIP_ERR_INVALID_ARG = 1,      /* reference: error("rate must be greater than 0") etc. */
    MRHIP_ERR_BUFFER_TOO_SMALL = 2, /* reference: error("buffer is too small"), Filters.jl:460,503,550 */
    MRHIP_ERR_HIP = 3,              /* a HIP runtime call failed; message holds hipGetErrorString */
    MRHIP_ERR_NO_DEVICE = 4,        /* no gfx950 device visible: the engine has no CPU fallback */
    MRHIP_ERR_UNSUPPORTED = 5       /* e.g. complex taps on mrhip_create_arbitrary / mrhip_create_farrow, FUSED numerics with complex taps */
} mrhip_status;

/* element types: Th in {F32,F64} for every kind, and {C64,C128} for the rational family (mrhip_create_rational, mrhip_create_rational_bank_ctaps) and
 * FIRArbitrary (mrhip_create_arbitrary_ctaps, mrhip_create_arbitrary_bank_ctaps) and FIRFarrow (mrhip_create_farrow_ctaps, mrhip_create_farrow_pnfb_ctaps, mrhip_create_farrow_bank_ctaps);
 * Tx in {F32,F64,C64,C128}; Tb = promote_type(Th,Tx) -- complex as soon as either side is */
typedef enum { MRHIP_F32 = 0, MRHIP_F64 = 1, MRHIP_C64 = 2, MRHIP_C128 = 3 } mrhip_dtype;

/* kernel kinds == the reference's FIRKernel subtypes, src/Filters.jl:15-117 */
typedef enum {
    MRHIP_FIR_STANDARD = 0,     /* FIRStandard     src/Filters.jl:15-24   */
    MRHIP_FIR_DECIMATOR = 1,    /* FIRDecimator    src/Filters.jl:45-58   */
    MRHIP_FIR_INTERPOLATOR = 2, /* FIRInterpolator src/Filters.jl:28-41   */
    MRHIP_FIR_RATIONAL = 3,     /* FIRRational     src/Filters.jl:62-80   */
    MRHIP_FIR_ARBITRARY = 4,    /* FIRArbitrary    src/Filters.jl:91-117  */
    MRHIP_FIR_FARROW = 5        /* FIRFarrow       src/Filters.jl:123-147 */
} mrhip_kind;

/* Arithmetic contract for the tap dot product (src/support.jl:5-55).
 *   STRICT: the order and roundings the reference source states -- oldest sample first,
 *           first product initialises the accumulator, separately rounded multiply and add
 *           in promote_type(Th,Tx) (no FMA; Julia 0.3 never fused).  Default.
 *   FUSED : same order, each step one fused multiply-add.  Faster where the kernel is
 *           VALU-bound; differs from STRICT by <= 1 rounding per tap. */
typedef enum { MRHIP_NUMERICS_STRICT = 0, MRHIP_NUMERICS_FUSED = 1 } mrhip_numerics;
/* Complex taps (Th in {C64,C128}; the rational family, FIRArbitrary through mrhip_create_arbitrary_ctaps and FIRFarrow through
 * mrhip_create_farrow_ctaps).  The reference is generic over the tap type: the unsafedot
 * methods (src/support.jl:5-55) only multiply and add, so the contract is the one above with Julia's complex products
 * written out.  Let R be the promoted real scalar (Float64 if either side is 64-bit, else Float32); every multiply, add
 * and subtract is rounded separately in R, a narrower operand is widened exactly before use:
 *   - the window is visited oldest sample first; the first product initialises the accumulator;
 *   - the start-from-zero seam of support.jl:46 applies as 0 + p on each component;
 *   - real sample x, tap (hr,hi):        p = (hr*x, hi*x)                          Complex*Real
 *   - complex sample (xr,xi):            p = (hr*xr - hi*xi, hr*xi + hi*xr)        Complex*Complex, operands in this order
 *   - acc = acc + p, component-wise.
 * The output is always complex (C128 if either side is 64-bit, else C64); the history stays in Tx (real for real
 * samples).  No FUSED form is defined: mrhip_set_numerics(f, FUSED) returns MRHIP_ERR_UNSUPPORTED on such a filter.
 * mrhip_create_arbitrary / mrhip_create_farrow with complex taps return MRHIP_ERR_UNSUPPORTED.
 * FIRArbitrary with complex taps (mrhip_create_arbitrary_ctaps; FIRArbitrary(h, rate, Nphi), src/Filters.jl:105-117, update,
 * tapsforphase! and filt!, :663-742, only take differences, multiply and add):
 *   - dh = [diff(h), 0] is taken per component in the tap type; pfb and dpfb are taps2pfb of h and dh;
 *   - yLower and yUpper are two complex dot products over ONE window, with pfb[:, phiIdx] and dpfb[:, phiIdx], each computed
 *     exactly as stated above (FIRArbitrary has no start-from-zero seam: its seam method is the Matrix one, support.jl:16-31);
 *   - buffer[k] = yLower + yUpper * alpha with alpha::Float64: both sides promote to Complex{Float64} and the store rounds to
 *     Complex{R}; per component c: y_c = R(double(lo_c) + double(up_c) * alpha), the product and the sum each rounded once in
 *     Float64 -- what the real-tap kernels do per real component;
 *   - the phase schedule, outputlength, set_state / reset and the mod form do not depend on the tap type;
 *   - no FUSED form either; the ring is not resident, mrhip_filt_device_multi issues single calls, mrhip_sharded_create refuses
 *     complex taps, and a cascade takes such a filter as a stage like any FIRArbitrary (the per-stage calls).
 * FIRFarrow with complex taps (mrhip_create_farrow_ctaps, mrhip_create_farrow_pnfb_ctaps; FIRFarrow(h, rate, Nphi, polyorder),
 * src/Filters.jl:138-147, pfb2pnfb :311-321, tapsforphase!, update and filt!, :764-839):
 *   - pnfb is one polynomial per ROW of taps2pfb(h, Nphi).  The least-squares fit is taken per component: polyfit on the real
 *     parts and on the imaginary parts of a row (the Vandermonde matrix is real, so a complex fit is these two; the reference
 *     pins no bits of the fit).  Coefficients are stored in the tap type per component -- for C64 each is rounded to Float32,
 *     as for F32 -- and held as Float64;
 *   - the taps of an output with the Float64 phase phi: for tap i and component c exactly the statement
 *     mrhip_farrow_tapsforphase makes for real taps -- Horner in Float64 from the highest power, t = phi*v; v = coef + t, the
 *     product and the sum each rounded once; the result rounded once to the tap's real scalar and widened exactly to R.  This is
 *     polyval(Poly{Complex{T}}, ::Float64) written out (y = p[i] + x*y; Real*Complex and Complex+Complex are by components),
 *     stored into currentTaps::Vector{Complex{T}} (:764-792).  (Polynomials.jl is not part of the reference tree this was
 *     written against; the statement is its documented Horner loop, as for real taps);
 *   - the dot is the Vector unsafedot (support.jl:33-55) with the products and sums stated above: oldest sample first, the
 *     first product initialises the accumulator; outputs with xIdx < tapsPerPhi that are not a continuation piece of a split
 *     call take the start-from-zero seam (support.jl:46) per component: acc_c = 0 + p_c;
 *   - the output is complex (C128 if either side is 64-bit, else C64), the history stays in Tx; the phase schedule,
 *     outputlength, set_state / reset and the mod form do not depend on the tap type;
 *   - no FUSED form; mrhip_sharded_create keeps refusing complex taps, mrhip_filt_device_multi issues single calls, a cascade
 *     takes such a filter as a stage through its per-stage calls. */
/* Per-channel taps (mrhip_create_rational_bank; the rational family, Th in {F32,F64}).  In the reference N channels are N
 * FIRFilter(h_c, ratio) objects and every h_c may differ; a filter built by mrhip_create_rational shares one h among its
 * channels.  A bank filter shares everything but the taps: ratio, state (phiIdx, inputDeficit) and call length.
 *   - for every channel c the outputs, the per-call counts, the end state and the history are bit for bit those of
 *     mrhip_create_rational(h_c, ..., nchannels = 1) fed x_c: every row goes through taps2pfb on its own, and the dot product
 *     is the one stated above (oldest sample first, first product initialises, the start-from-zero seam of support.jl:46);
 *   - STRICT is the default; under mrhip_set_numerics(f, FUSED) the results are those of that one-channel filter under FUSED;
 *   - everything that does not depend on the taps is unchanged: outputlength, inputlength, set_state, reset, set_history*,
 *     next_output_count, outputlength_bound; the mrhip_state layout is the same;
 *   - mrhip_get_taps(f, 0, out) returns the nchannels filter banks one after the other, each tapsPerPhi*Nphi elements laid
 *     out as mrhip_taps2pfb does;
 *   - complex taps return MRHIP_ERR_UNSUPPORTED here (they have a constructor of their own: "Per-channel complex taps" below); FIRArbitrary has a
 *     bank constructor of its own ("Per-channel taps for FIRArbitrary" below), and so has FIRFarrow ("Per-channel taps for FIRFarrow");
 *   - mrhip_filt_device_multi with a bank filter among its streams issues single calls; a ring on a bank filter is not
 *     resident (stream-ordered launches); mrhip_sharded_create has no bank constructor; a cascade takes a bank filter as a
 *     stage through its per-stage calls. */
/* Per-channel complex taps (mrhip_create_rational_bank_ctaps; the rational family, Th in {C64,C128}): one
 * FIRFilter(h_c::Vector{Complex}, ratio) per channel behind one handle -- a prototype rotated to every channel's own centre
 * frequency, per-channel Hilbert filters, per-antenna complex equalisers.  The contract is the conjunction of the two above:
 *   - for every channel c the outputs, the per-call counts, the end state and the history are bit for bit those of
 *     mrhip_create_rational(h_c complex, ..., nchannels = 1) fed x_c: the "Complex taps" arithmetic on bank c;
 *   - that arithmetic: every multiply, add and subtract is rounded separately in R; the window is visited oldest sample first,
 *     the first product initialises the accumulator, the start-from-zero seam of support.jl:46 applies as 0 + p per component,
 *     and the Complex*Real and Complex*Complex products are written out in the operand order stated under "Complex taps";
 *   - the output is always complex (C128 if either side is 64-bit, else C64); the history stays in Tx;
 *   - no FUSED form is defined: mrhip_set_numerics(f, FUSED) returns MRHIP_ERR_UNSUPPORTED;
 *   - mrhip_get_taps(f, 0, out) returns the nchannels filter banks one after the other, each tapsPerPhi*Nphi (re, im) pairs
 *     laid out as mrhip_taps2pfb does;
 *   - everything that does not depend on the taps is unchanged: outputlength, inputlength, set_state, reset, set_history*,
 *     next_output_count, outputlength_bound; the mrhip_state layout is the same and its tap_dtype reads 2 or 3;
 *   - mrhip_create_rational_bank keeps returning MRHIP_ERR_UNSUPPORTED for complex taps; a real tap_dtype here is
 *     MRHIP_ERR_INVALID_ARG;
 *   - as for both parents: mrhip_filt_device_multi with such a filter among its streams issues single calls; a ring on it is
 *     not resident (stream-ordered launches); mrhip_sharded_create has no such constructor; a cascade takes the filter as a
 *     stage through its per-stage calls. */

/* Per-channel taps for FIRArbitrary (mrhip_create_arbitrary_bank; Th in {F32,F64}): one FIRFilter(h_c, rate, Nphi) per channel
 * behind one handle -- per-antenna equalisers folded into the prototype of a clock-trim resampler, per-channel matched pulse
 * shapes, per-sensor calibration filters.  The phase schedule (update(), src/Filters.jl:663-673) does not depend on the taps, so
 * the channels share rate, Nphi, state and call length; only the two filter banks differ.
 *   - for every channel c the outputs, the per-call counts, the end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx)
 *     and the history are bit for bit those of mrhip_create_arbitrary(h_c, ..., nchannels = 1) fed x_c;
 *   - every row gets its own dh_c = [diff(h_c), 0] in the tap type, and both taps2pfb calls are made per row;
 *   - both dots are taken over ONE window, oldest sample first, the first product initialises the accumulator, no
 *     start-from-zero seam (FIRArbitrary's seam method is the Matrix one, support.jl:16-31); STRICT rounds every multiply and add
 *     separately in R, FUSED is one fma per tap; y = R(double(lo) + double(up) * alpha), the product and the sum each rounded
 *     once in Float64;
 *   - STRICT is the default; under mrhip_set_numerics(f, FUSED) the results are those of that one-channel filter under FUSED;
 *   - everything that does not depend on the taps is the shared code, unchanged: the phase schedule, mrhip_set_mod_form,
 *     outputlength, next_output_count, outputlength_bound, advance_state, set_state, reset, set_history*; the mrhip_state
 *     layout is the same;
 *   - mrhip_get_taps(f, 0, out) returns the nchannels pfb banks one after the other, which = 1 the dpfb banks; each bank is
 *     tapsPerPhi*Nphi elements laid out as mrhip_taps2pfb does;
 *   - mrhip_arbitrary_tapsforphase returns nchannels rows of tapsPerPhi taps, row c is the statement for real taps on bank c;
 *     the range errors are unchanged;
 *   - mrhip_create_arbitrary and mrhip_create_rational_bank* answer exactly as before; mrhip_filt_device_multi with such a
 *     filter among its streams issues single calls; a ring on it is not resident; mrhip_sharded_create has no such
 *     constructor; a cascade takes the filter as a stage through its per-stage calls;
 *   - complex taps return MRHIP_ERR_UNSUPPORTED here (left out of THIS constructor: they have one of their own, "Per-channel complex
 *     taps for FIRArbitrary" below); left out on purpose: sharded banks, and the hand-scheduled shared-taps FIRArbitrary kernels (such
 *     a filter runs on its own two kernels).  FIRFarrow banks have a constructor of their own (below). */

/* Per-channel complex taps for FIRArbitrary (mrhip_create_arbitrary_bank_ctaps; Th in {C64,C128}): one
 * FIRFilter(h_c::Vector{Complex}, rate, Nphi) per channel behind one handle -- a prototype rotated to every channel's own centre
 * frequency in front of a common clock-trim or arbitrary-rate change, per-antenna complex equalisers folded into the resampler's
 * prototype, per-channel Hilbert or single-sideband filters in front of a symbol-rate change.  The contract is the conjunction of
 * "Complex taps" (FIRArbitrary) and "Per-channel taps for FIRArbitrary":
 *   - for every channel c the outputs, the per-call counts, the end state (inputDeficit, phiAccumulator, phiIdx, alpha, xIdx)
 *     and the history are bit for bit those of mrhip_create_arbitrary_ctaps(h_c, ..., nchannels = 1) fed x_c;
 *   - every row gets its own dh_c = [diff(h_c), 0], taken per component in the tap type, and both taps2pfb calls are made per row;
 *   - both dots are taken over ONE window, oldest sample first, the first product initialises the accumulator, no
 *     start-from-zero seam; Complex*Real and Complex*Complex are written out in the operand order stated under "Complex taps",
 *     every multiply, add and subtract rounded separately in R; per component y_c = R(double(lo_c) + double(up_c) * alpha), the
 *     product and the sum each rounded once in Float64;
 *   - the output is always complex (C128 if either side is 64-bit, else C64); the history stays in Tx;
 *   - no FUSED form is defined: mrhip_set_numerics(f, FUSED) returns MRHIP_ERR_UNSUPPORTED;
 *   - everything that does not depend on the taps is the shared code, unchanged: the phase schedule, mrhip_set_mod_form,
 *     outputlength, next_output_count, outputlength_bound, advance_state, set_state, reset, set_history*; the mrhip_state
 *     layout is the same and its tap_dtype reads 2 or 3;
 *   - mrhip_get_taps(f, 0, out) returns the nchannels pfb banks one after the other, which = 1 the dpfb banks; each bank is
 *     tapsPerPhi*Nphi (re, im) pairs laid out as mrhip_taps2pfb does;
 *   - mrhip_arbitrary_tapsforphase returns nchannels rows of tapsPerPhi pairs, row c is the statement for complex taps (per
 *     component) on bank c; the range errors are unchanged;
 *   - mrhip_create_arbitrary_bank keeps returning MRHIP_ERR_UNSUPPORTED for complex taps; a real tap_dtype here is
 *     MRHIP_ERR_INVALID_ARG; mrhip_create_arbitrary_ctaps and mrhip_create_arbitrary answer exactly as before;
 *   - as for both parents: mrhip_filt_device_multi with such a filter among its streams issues single calls; a ring on it is
 *     not resident; mrhip_sharded_create has no such constructor; a cascade takes the filter as a stage through its per-stage
 *     calls;
 *   - left out on purpose: a FUSED form, sharded banks, a resident ring for banks.  FIRFarrow banks with complex taps have a
 *     constructor of their own ("Per-channel complex taps for FIRFarrow" below). */

/* Per-channel taps for FIRFarrow (mrhip_create_farrow_bank; Th in {F32,F64}): one FIRFilter(h_c, rate, Nphi, polyorder) per
 * channel behind one handle -- a per-antenna equaliser or a per-sensor calibration filter in front of a common, continuously
 * variable rate change.  The phase schedule (update(), src/Filters.jl:780-792) does not depend on the taps, so the channels
 * share rate, Nphi, polyorder, state and call length; only the polynomial banks differ.
 *   - for every channel c the outputs, the per-call counts, the end state (inputDeficit, phiAccumulator, phiIdx) and the history
 *     are bit for bit those of mrhip_create_farrow(h_c, ..., nchannels = 1) fed x_c;
 *   - every row goes through taps2pfb and the per-row polynomial fit on its own, exactly as mrhip_create_farrow treats one h;
 *     the coefficients are stored in the tap type;
 *   - per tap: Horner in Float64 from the highest power, t = phi*v; v = coef + t, the product and the sum each rounded once
 *     (never fused, under FUSED neither), the result rounded once to the tap type and widened exactly to R;
 *   - the dot: oldest sample first, the first product initialises the accumulator, outputs on the start-from-zero seam of
 *     support.jl:46 then take 0 + acc per component; the remaining taps are a separately rounded multiply and add under STRICT
 *     and one fma under FUSED;
 *   - STRICT is the default; under mrhip_set_numerics(f, FUSED) the results are those of that one-channel filter under FUSED;
 *   - everything that does not depend on the taps is the shared code, unchanged: the phase schedule, mrhip_set_mod_form,
 *     outputlength, next_output_count, outputlength_bound, advance_state, set_state, reset, set_history*; the mrhip_state
 *     layout is the same;
 *   - mrhip_get_pnfb returns the nchannels banks one after the other, [nchannels][tapsPerPhi][polyorder+1] Float64;
 *   - mrhip_farrow_tapsforphase returns nchannels rows of tapsPerPhi taps, row c is the statement for real taps on bank c; the
 *     range error is unchanged;
 *   - mrhip_create_farrow*, mrhip_create_arbitrary_bank and mrhip_create_rational_bank* answer exactly as before;
 *     mrhip_filt_device_multi with such a filter among its streams issues single calls; a ring on it is not resident;
 *     mrhip_sharded_create has no such constructor; a cascade takes the filter as a stage through its per-stage calls;
 *   - complex taps return MRHIP_ERR_UNSUPPORTED here (left out of THIS constructor: they have one of their own, "Per-channel complex
 *     taps for FIRFarrow" below); left out on purpose: a caller-fitted pnfb for banks, sharded banks, a resident ring for banks, and
 *     the shared-taps FIRFarrow kernels farrow_pipe_kernel / farrow_wave_kernel (such a filter runs on its own two kernels). */

/* Per-channel complex taps for FIRFarrow (mrhip_create_farrow_bank_ctaps; Th in {C64,C128}): one
 * FIRFilter(h_c::Vector{Complex}, rate, Nphi, polyorder) per channel behind one handle -- a prototype rotated to every channel's own
 * centre frequency, or a per-antenna complex equaliser, in front of a common, continuously variable rate change.  The contract is
 * the conjunction of "Complex taps" (FIRFarrow) and "Per-channel taps for FIRFarrow":
 *   - for every channel c the outputs, the per-call counts, the end state (inputDeficit, phiAccumulator, phiIdx) and the history
 *     are bit for bit those of mrhip_create_farrow_ctaps(h_c, ..., nchannels = 1) fed x_c;
 *   - every row goes through taps2pfb and the per-component polynomial fit on its own, exactly as mrhip_create_farrow_ctaps
 *     treats one h; the coefficients are stored in the tap type, per component;
 *   - per tap and component: Horner in Float64 from the highest power, t = phi*v; v = coef + t, the product and the sum each
 *     rounded once (never fused), the result rounded once to the tap's real scalar and widened exactly to R;
 *   - the dot: oldest sample first, the first product initialises the accumulator, Complex*Real and Complex*Complex written out
 *     in the operand order stated under "Complex taps", every multiply, add and subtract rounded separately in R; outputs on the
 *     start-from-zero seam of support.jl:46 then take 0 + acc per component;
 *   - the output is always complex (C128 if either side is 64-bit, else C64); the history stays in Tx;
 *   - STRICT only, no FUSED form is defined: mrhip_set_numerics(f, FUSED) returns MRHIP_ERR_UNSUPPORTED;
 *   - everything that does not depend on the taps is the shared code, unchanged: the phase schedule, mrhip_set_mod_form,
 *     outputlength, next_output_count, outputlength_bound, advance_state, set_state, reset, set_history*; the mrhip_state
 *     layout is the same and its tap_dtype reads 2 or 3;
 *   - mrhip_get_pnfb returns the nchannels banks one after the other, [nchannels][tapsPerPhi][polyorder+1] (re, im) pairs of
 *     Float64;
 *   - mrhip_farrow_tapsforphase returns nchannels rows of tapsPerPhi pairs, row c is the statement for complex taps (per
 *     component) on bank c; the range error is unchanged;
 *   - mrhip_create_farrow_bank keeps returning MRHIP_ERR_UNSUPPORTED for complex taps; a real tap_dtype here is
 *     MRHIP_ERR_INVALID_ARG; mrhip_create_farrow*, mrhip_create_arbitrary_bank* and mrhip_create_rational_bank* answer exactly as
 *     before;
 *   - as for both parents: mrhip_filt_device_multi with such a filter among its streams issues single calls; a ring on it is
 *     not resident; mrhip_sharded_create has no such constructor; a cascade takes the filter as a stage through its per-stage
 *     calls;
 *   - such a filter runs on ONE kernel (farrow_bank_ctaps_generic_kernel); MRHIP_FORCE_GENERIC has no effect on it;
 *   - left out on purpose: a caller-fitted pnfb for banks, a FUSED form, sharded banks, a resident ring for banks. */

/* Per-channel rates for FIRArbitrary (mrhip_create_arbitrary_rates; Th in {F32,F64}): one FIRFilter(h, rates[c], Nphi) per channel
 * behind one handle -- receivers or ADCs each off its own clock trimmed to a common rate, per-satellite or per-emitter Doppler
 * time-scale correction, and (with a per-channel start phase, mrhip_set_channel_states) per-channel fractional delay.  The channels
 * share h (so pfb and dpfb), Nphi, the call length and the history length; each channel has its own rate, delta, phiAccumulator,
 * phiIdx, alpha, xIdx, inputDeficit and per-call output count (mrhip_channel_state).
 *   - parity: for every channel c the outputs, the count of every call, the end state (inputDeficit, phiAccumulator, phiIdx, alpha,
 *     xIdx) and the history are bit for bit those of mrhip_create_arbitrary(h, rates[c], Nphi, nchannels = 1) fed x_c, under STRICT
 *     and under FUSED.  That includes the short-input path of filt! (src/Filters.jl:705-709): a channel whose inputDeficit exceeds
 *     x_len writes nothing and only has its deficit reduced, while its neighbours produce outputs in the same call;
 *   - arithmetic: that of "Per-channel taps for FIRArbitrary" -- two dot products over ONE window, oldest sample first, the first
 *     product initialises the accumulator, no start-from-zero seam, y = R(double(lo) + double(up) * alpha);
 *   - tap types F32 and F64 (complex taps: MRHIP_ERR_UNSUPPORTED, left out); all four sample types;
 *   - any rate <= 0 (or not finite) is MRHIP_ERR_INVALID_ARG; a rate below 2^-30 is MRHIP_ERR_UNSUPPORTED;
 *   - mrhip_set_mod_form(f, 1) is accepted when Nphi is a power of two, where the two forms agree in every bit; otherwise it
 *     returns MRHIP_ERR_UNSUPPORTED;
 *   - device-planned calls only: the host never learns a count before the kernels have run.  mrhip_filt_device_rates enqueues a
 *     schedule kernel (one lane per channel walks update() serially) and one filter kernel on the caller's stream and nothing else;
 *     the filter has no schedule stream and uses no stream of its own in a call;
 *   - these work on such a filter: mrhip_destroy, mrhip_reset, mrhip_set_numerics, mrhip_get_history, mrhip_set_history,
 *     mrhip_set_history_device, mrhip_get_taps, mrhip_arbitrary_tapsforphase, mrhip_outputlength_bound (the largest of the channels'
 *     bounds), mrhip_synchronize, mrhip_set_timing, mrhip_timing_read, mrhip_last_kernel_name;
 *   - every entry point that carries ONE state or ONE count returns MRHIP_ERR_UNSUPPORTED (-1 from the counting functions) with a
 *     message that names the calls below: mrhip_filt_device, _async, _chained, _chunked, mrhip_filt_host, mrhip_filt_device_multi,
 *     mrhip_ring_open, mrhip_cascade_create, mrhip_get_state, mrhip_set_state, mrhip_sync_state, mrhip_outputlength,
 *     mrhip_inputlength, mrhip_next_output_count, mrhip_advance_state; mrhip_sharded_create has no such constructor;
 *   - every other constructor and filter answers exactly as before;
 *   - the rates may change between calls: mrhip_set_channel_rates; mrhip_reset restores the constructor STATE of every channel and
 *     keeps the current rates;
 *   - the call length is shared through mrhip_filt_device_rates; mrhip_filt_device_rates_ragged feeds every channel its own number of
 *     samples (both filters with per-channel rates; the contract stands at its declaration);
 *   - per-channel taps on top of the per-channel rates: mrhip_set_channel_taps ("Per-channel taps with per-channel rates for
 *     FIRArbitrary", below);
 *   - complex taps on top of the per-channel rates: mrhip_set_channel_ctaps and mrhip_set_channel_ctaps_device ("Complex per-channel
 *     taps with per-channel rates for FIRArbitrary", below);
 *   - left out on purpose: evaluating
 *     a long channel's schedule with the parallel tables / chain / emit machinery instead of the serial walk (the next speed step
 *     for few long channels); graph capture, rings, cascades and sharding of such a filter; a mrhip_filt_device_multi that serves
 *     FIRArbitrary streams in one launch. */

/* Per-channel rates for FIRFarrow (mrhip_create_farrow_rates, mrhip_create_farrow_rates_pnfb; Th in {F32,F64}): one
 * FIRFilter(h, rates[c], Nphi, polyorder) per channel behind one handle -- FIRFarrow is the kernel the reference offers for a
 * continuously variable rate, so the users of per-channel rates named above are Farrow users first.  The channels share h -- so the ONE
 * polynomial bank pnfb, fitted once by the fit of mrhip_create_farrow (or handed over) -- Nphi, polyorder, the call length and the history
 * length; each channel has its own rate, delta, phiIdx (the Float64 phase: phiAccumulator of mrhip_channel_state), xIdx, inputDeficit
 * and per-call output count.
 *   - the constructor state of a channel is FIRFarrow's (src/Filters.jl:141-144: phiIdx = 1.0, inputDeficit = xIdx = 1), which is the
 *     state the records of the FIRArbitrary filter start from: both filters share the reset of their records, the schedule kernel
 *     (update(), :780-786, is the recurrence of :663-669 on the same Float64 quantity) and mrhip_filt_device_rates,
 *     mrhip_get_channel_states, mrhip_set_channel_states, mrhip_set_channel_rates;
 *   - parity: channel c is bit for bit mrhip_create_farrow(h, rates[c], Nphi, polyorder, nchannels = 1) (with a handed-over bank:
 *     mrhip_create_farrow_pnfb) fed x_c, under STRICT and under FUSED: the outputs, the count of every call, the end state and the
 *     history.  That includes the short-input path (:805-809) and the zero-start seam of outputs with xIdx < tapsPerPhi (:819-820) on
 *     EVERY call: a call of this filter always starts a filt!, it never continues one;
 *   - arithmetic: that of "Per-channel taps for FIRFarrow" on the one bank -- Horner in Float64 from the highest power, product and sum
 *     rounded separately and never fused, also under FUSED; the tap rounded once to the tap type; the dot oldest sample first, the first
 *     product initialises the accumulator;
 *   - mrhip_channel_state reports per channel what mrhip_get_state reports for a one-channel FIRFarrow filter: phiAccumulator is the
 *     Float64 phase, phiIdx = floor(phiAccumulator) and alpha the remainder;
 *   - tap types F32 and F64 (complex taps: MRHIP_ERR_UNSUPPORTED, left out); all four sample types; the rate checks are those of
 *     mrhip_create_arbitrary_rates, Nphi, polyorder and every other check those of mrhip_create_farrow (_pnfb);
 *   - mrhip_get_pnfb and mrhip_farrow_tapsforphase answer as on a one-channel FIRFarrow filter of h;
 *   - the call contract is the one stated for FIRArbitrary: two launches on the caller's stream, every host-side failure before the
 *     schedule kernel, no capture, at most 2^24 entries a channel, the same schedule buffers and their one reallocation wait, one timing
 *     bracket around both launches, and every entry point that carries ONE state or ONE count refuses the filter;
 *   - kernels: farrow_rates_generic (any shape) and farrow_rates_multi (four outputs a lane share each tap's scalar coefficient loads;
 *     MRHIP_FARROW_RATES_MULTI = 1 selects it, the default rule selects it nowhere until measurements say where);
 *   - per-channel taps on top of the per-channel rates: mrhip_set_channel_taps_farrow and mrhip_set_channel_pnfb ("Per-channel taps
 *     with per-channel rates for FIRFarrow", below);
 *   - complex taps on top of the per-channel rates: mrhip_set_channel_ctaps_farrow and mrhip_set_channel_pnfb_ctaps* ("Complex
 *     per-channel taps with per-channel rates for FIRFarrow", below);
 *   - left out on purpose: graph capture, rings,
 *     cascades and sharding of such a filter; the parallel schedule for long channels, which stays the named next speed step and is shared by both filters. */

typedef struct mrhip_filter mrhip_filter; /* opaque; replaces FIRFilter{Tk}, src/Filters.jl:151-155 */

/* Snapshot of the kernel fields of the reference structs (src/Filters.jl:15-117,151-155).
 * Indices are 1-based like the reference's. */
typedef struct {
    int32_t kind;            /* mrhip_kind */
    int32_t tap_dtype;       /* Th */
    int32_t sample_dtype;    /* Tx */
    int32_t output_dtype;    /* Tb = promote_type(Th,Tx) */
    int64_t nchannels;
    int64_t hLen;            /* length(h) as passed */
    int64_t interpolation;   /* L (reduced) ; Nphi for ARBITRARY */
    int64_t decimation;      /* M (reduced) */
    int64_t Nphi;            /* N𝜙 */
    int64_t tapsPerPhi;      /* tapsPer𝜙 (== hLen for STANDARD/DECIMATOR) */
    int64_t historyLen;
    int64_t phiIdx;          /* 𝜙Idx          FIRRational :68, FIRArbitrary :98 */
    int64_t inputDeficit;    /* inputDeficit  :49, :69, :101 */
    int64_t xIdx;            /* FIRArbitrary.xIdx :102 */
    double rate;             /* FIRArbitrary.rate :92 */
    double phiAccumulator;   /* 𝜙Accumulator :97 */
    double alpha;            /* α :99 */
    double delta;            /* Δ :100 */
} mrhip_state;

/* One channel of a filter with per-channel rates (mrhip_create_arbitrary_rates, mrhip_create_farrow_rates): the FIRArbitrary fields that differ from channel to
 * channel (src/Filters.jl:91-117), and the output count of the channel's latest call. */
typedef struct { double rate, delta, phiAccumulator, alpha;
                 int64_t phiIdx, inputDeficit, xIdx, last_count; } mrhip_channel_state;

/* ---- library ------------------------------------------------------------------------- */
int mrhip_abi_version(void);
const char *mrhip_last_error(void);
/* number of visible HIP devices whose arch is gfx950 (0 => every create fails with NO_DEVICE) */
int mrhip_device_count(void);

/* ---- host-only helpers (no GPU needed) ------------------------------------------------ */
/* replaces taps2pfb(h, Nphi), src/Filters.jl:284-298.  `pfb` receives tapsPerPhi*Nphi elements,
 * column-major (column = phase, contiguous); pass pfb = NULL to query.  Returns tapsPerPhi.  Any tap_dtype,
 * complex ones included. */
int64_t mrhip_taps2pfb(const void *h, int64_t hLen, int tap_dtype, int64_t Nphi, void *pfb);
/* replaces nextphase(currentphase, ratio), src/Filters.jl:433-439 */
int64_t mrhip_nextphase(int64_t currentphase, int64_t interpolation, int64_t decimation);
/* replaces outputlength(inputlength, ratio, initial𝜙), src/Filters.jl:352-357 */
int64_t mrhip_outputlength_ratio(int64_t inputlength, int64_t interpolation, int64_t decimation,
                                 int64_t initialPhi);
/* replaces inputlength(outputlength, ratio, initial𝜙), src/Filters.jl:396-401 */
int64_t mrhip_inputlength_ratio(int64_t outputlength, int64_t interpolation, int64_t decimation,
                                int64_t initialPhi);
/* replaces polyfit(y, polyorder), src/support.jl:85-88: least-squares polynomial through (x = 1..n, y[x]);
 * coef receives polyorder+1 coefficients, ascending powers (Poly.a).  Returns 0, or MRHIP_ERR_INVALID_ARG when
 * n < polyorder+1.  Float64 throughout (Julia's A \\ y promotes to Float64). */
int mrhip_polyfit(const double *y, int64_t n, int64_t polyorder, double *coef);
/* promote_type(Th, Tx) as used by every filt wrapper, e.g. src/Filters.jl:581 (complex if either argument is) */
int mrhip_output_dtype(int tap_dtype, int sample_dtype);

/* ---- FIR design, host only (src/FIRDesign.jl) ----------------------------------------------- */
/* replaces @enum(FIRResponse, LOWPASS, BANDPASS, HIGHPASS, BANDSTOP), src/FIRDesign.jl:7 (values 0..3, src/enum.jl) */
typedef enum { MRHIP_LOWPASS = 0, MRHIP_BANDPASS = 1, MRHIP_HIGHPASS = 2, MRHIP_BANDSTOP = 3 } mrhip_fir_response;
/* replaces kaiserlength(transition, attenuation = 60; samplerate = 1.0), src/FIRDesign.jl:18-33: (numtaps, beta) */
int mrhip_kaiserlength(double transition, double attenuation, double samplerate, int64_t *numtaps, double *beta);
/* the window firdes multiplies with when windowfunction == kaiser (src/FIRDesign.jl:82-83; DSP.jl's kaiser in the
 * reference, beta taken as is like src/Window.jl:53-58): out receives n Float64 samples */
int mrhip_kaiser(int64_t n, double beta, double *out);
/* replaces firprototype(numtaps, F; response), src/FIRDesign.jl:47-66.  F holds nF cutoffs in cycles/sample (two for
 * BANDPASS / BANDSTOP).  Returns the length of the prototype (numtaps, or numtaps+1 for HIGHPASS with an even
 * numtaps, :55) or -1 (mrhip_last_error: "Not a valid FIR_TYPE", :62); out = NULL only queries the length. */
int64_t mrhip_firprototype(int64_t numtaps, const double *F, int nF, int response, double *out);
/* replaces firdes(numtaps, cutoff, windowfunction; response, samplerate, beta), src/FIRDesign.jl:76-88.
 * `window` = NULL selects the Kaiser window with `beta` (windowfunction == kaiser, :82-83); otherwise it points to
 * the caller's window evaluated at the prototype length (:85) -- query that length first with out = NULL.
 * Returns the number of taps written (Float64), or -1. */
int64_t mrhip_firdes(int64_t numtaps, const double *cutoff, int ncutoff, int response, double samplerate, double beta,
                     const double *window, double *out);
/* replaces firdes(cutoff, transitionwidth, stopbandAttenuation = 60; response, samplerate), src/FIRDesign.jl:90-95
 * (kaiserlength, then the method above).  out = NULL queries the length. */
int64_t mrhip_firdes_kaiser(const double *cutoff, int ncutoff, double transitionwidth, double stopbandAttenuation, int response,
                            double samplerate, double *out);

/* ---- construction --------------------------------------------------------------------- */
/* replaces FIRFilter(h::Vector, resampleRatio::Rational = 1//1), src/Filters.jl:158-180.
 * num//den is reduced like a Julia Rational; the kernel kind is chosen exactly as :163-175
 * (ratio == 1 -> STANDARD, L == 1 -> DECIMATOR, M == 1 -> INTERPOLATOR, else RATIONAL).
 * `h` is a host pointer to hLen taps of tap_dtype (F32 | F64 | C64 | C128; complex taps are interleaved (re, im)
 * pairs and make the output complex: see "Complex taps" above).  `device` is a HIP ordinal. */
int mrhip_create_rational(const void *h, int64_t hLen, int tap_dtype, int64_t num, int64_t den,
                          int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* one FIRFilter(h_c, resampleRatio) per channel behind one handle (see "Per-channel taps" above): `h` holds nchannels rows of
 * hLen taps, row-major, row c is channel c's h.  tap_dtype F32 | F64 (complex: MRHIP_ERR_UNSUPPORTED).  Kind selection, L, M,
 * tapsPerPhi, historyLen and every error are those of mrhip_create_rational. */
int mrhip_create_rational_bank(const void *h, int64_t hLen, int tap_dtype, int64_t num, int64_t den,
                               int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* the same for COMPLEX taps (see "Per-channel complex taps" above): `h` holds nchannels rows of hLen interleaved (re, im) pairs,
 * row-major, row c is channel c's h.  tap_dtype C64 | C128; a real tap_dtype is MRHIP_ERR_INVALID_ARG: real taps use
 * mrhip_create_rational_bank (which keeps refusing complex ones).  Kind selection, L, M, tapsPerPhi, historyLen and every other
 * error are those of mrhip_create_rational. */
int mrhip_create_rational_bank_ctaps(const void *h, int64_t hLen, int tap_dtype, int64_t num, int64_t den,
                                     int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* replaces FIRFilter(h::Vector, rate::FloatingPoint, Nphi::Integer = 32), src/Filters.jl:183-189
 * (+ FIRArbitrary(h, rate, Nphi), :105-117: dh = [diff(h), 0], two PFBs).  rate <= 0 is
 * MRHIP_ERR_INVALID_ARG ("rate must be greater than 0", :184). */
int mrhip_create_arbitrary(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,
                           int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* the same constructor for COMPLEX taps (tap_dtype C64 | C128, interleaved (re, im) pairs; see "Complex taps" above): the
 * filter's kind is MRHIP_FIR_ARBITRARY and its output is complex for every sample type.  A real tap_dtype is
 * MRHIP_ERR_INVALID_ARG: real taps use mrhip_create_arbitrary (which keeps refusing complex ones). */
int mrhip_create_arbitrary_ctaps(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,
                                 int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* one FIRFilter(h_c, rate, Nphi) per channel behind one handle (see "Per-channel taps for FIRArbitrary" above): `h` holds nchannels
 * rows of hLen taps, row-major, row c is channel c's h.  tap_dtype F32 | F64 (complex: MRHIP_ERR_UNSUPPORTED, left out).  rate, Nphi
 * and every other argument check are those of mrhip_create_arbitrary; the filter's kind is MRHIP_FIR_ARBITRARY. */
int mrhip_create_arbitrary_bank(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,
                                int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* the same for COMPLEX taps (see "Per-channel complex taps for FIRArbitrary" above): `h` holds nchannels rows of hLen interleaved
 * (re, im) pairs, row-major, row c is channel c's h.  tap_dtype C64 | C128; a real tap_dtype is MRHIP_ERR_INVALID_ARG: real taps use
 * mrhip_create_arbitrary_bank (which keeps refusing complex ones).  rate, Nphi and every other argument check are those of
 * mrhip_create_arbitrary; the filter's kind is MRHIP_FIR_ARBITRARY and its output is complex for every sample type. */
int mrhip_create_arbitrary_bank_ctaps(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,
                                      int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* one FIRFilter(h, rates[c], Nphi) per channel behind one handle (see "Per-channel rates for FIRArbitrary" above): `h` is ONE tap
 * vector of hLen taps, `rates` holds nchannels rates.  tap_dtype F32 | F64 (complex: MRHIP_ERR_UNSUPPORTED, left out).  Every rate
 * must be greater than 0 (MRHIP_ERR_INVALID_ARG); Nphi and every other argument check are those of mrhip_create_arbitrary; the
 * filter's kind is MRHIP_FIR_ARBITRARY. */
int mrhip_create_arbitrary_rates(const void *h, int64_t hLen, int tap_dtype, const double *rates,
                                 int64_t Nphi, int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* one FIRFilter(h, rates[c], Nphi, polyorder) per channel behind one handle (see "Per-channel rates for FIRFarrow" above): `h` is ONE
 * tap vector of hLen taps, `rates` holds nchannels rates.  tap_dtype F32 | F64 (complex: MRHIP_ERR_UNSUPPORTED, left out).  The rate
 * checks are those of mrhip_create_arbitrary_rates; Nphi, polyorder and every other argument check are those of mrhip_create_farrow;
 * the filter's kind is MRHIP_FIR_FARROW.  _pnfb: the polynomial bank supplied by the caller, with the contract of
 * mrhip_create_farrow_pnfb. */
int mrhip_create_farrow_rates(const void *h, int64_t hLen, int tap_dtype, const double *rates, int64_t Nphi, int64_t polyorder,
                              int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
int mrhip_create_farrow_rates_pnfb(const double *pnfb, int64_t hLen, int tap_dtype, const double *rates, int64_t Nphi,
                                   int64_t polyorder, int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* replaces FIRFilter(h::Vector, rate::FloatingPoint, Nphi::Integer, polyorder::Integer),
 * src/Filters.jl:192-198 (+ FIRFarrow(h, rate, Nphi, polyorder), :138-147, pfb2pnfb :311-321 and
 * polyfit, src/support.jl:85-88): every ROW of the tapsPerPhi x Nphi filter bank is replaced by its
 * least-squares polynomial of degree polyorder over x = 1..Nphi, stored in the tap type; the taps of an
 * output are those polynomials evaluated at its Float64 phase.  The fit (Julia: A \ y, LAPACK QR) is
 * done on the host in Float64 by a Householder QR. */
int mrhip_create_farrow(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi, int64_t polyorder,
                        int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* one FIRFilter(h_c, rate, Nphi, polyorder) per channel behind one handle (see "Per-channel taps for FIRFarrow" above): `h` holds
 * nchannels rows of hLen taps, row-major, row c is channel c's h.  tap_dtype F32 | F64 (complex: MRHIP_ERR_UNSUPPORTED, left out of
 * this entry point: mrhip_create_farrow_bank_ctaps).
 * rate, Nphi, polyorder and every other argument check are those of mrhip_create_farrow; the filter's kind is MRHIP_FIR_FARROW. */
int mrhip_create_farrow_bank(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi, int64_t polyorder, int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* the same with COMPLEX taps (see "Per-channel complex taps for FIRFarrow" above): `h` holds nchannels rows of hLen interleaved
 * (re, im) taps, row-major.  tap_dtype C64 | C128 (real: MRHIP_ERR_INVALID_ARG, mrhip_create_farrow_bank takes those); every other
 * argument check is that of mrhip_create_farrow_ctaps; the output is complex for every sample type. */
int mrhip_create_farrow_bank_ctaps(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi, int64_t polyorder,
                                   int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* same, with the polynomial filter bank supplied by the caller: pnfb[tapsPerPhi][polyorder+1] Float64,
 * ascending powers (the layout of Poly.a), tapsPerPhi = ceil(hLen/Nphi); values are rounded to the tap type
 * as the reference's Poly{T} storage does.  Lets a caller fit with its own least-squares routine (the
 * reference pins no bits of the fit) and lets tests hand oracle and GPU the same coefficients. */
int mrhip_create_farrow_pnfb(const double *pnfb, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,
                             int64_t polyorder, int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* the two FIRFarrow constructors for COMPLEX taps (tap_dtype C64 | C128; see "Complex taps" above): the filter's kind is
 * MRHIP_FIR_FARROW and its output is complex for every sample type.  `h`: interleaved (re, im) pairs, the fit is taken per
 * component; `pnfb`: [tapsPerPhi][polyorder+1] (re, im) pairs of Float64, ascending powers.  A real tap_dtype is
 * MRHIP_ERR_INVALID_ARG: real taps use the two constructors above (which keep refusing complex ones); the other argument
 * checks are theirs. */
int mrhip_create_farrow_ctaps(const void *h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi, int64_t polyorder,
                              int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
int mrhip_create_farrow_pnfb_ctaps(const double *pnfb, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,
                                   int64_t polyorder, int sample_dtype, int64_t nchannels, int device, mrhip_filter **out);
/* the polynomial filter bank in use, [tapsPerPhi][polyorder+1] Float64 (pfb2pnfb's result); complex taps: (re, im) pairs of
 * Float64, twice as many values; per-channel taps (mrhip_create_farrow_bank, mrhip_create_farrow_bank_ctaps): the nchannels banks
 * one after the other */
int mrhip_get_pnfb(const mrhip_filter *f, double *host_out);
/* replaces tapsforphase(kernel::FIRFarrow, phase), src/Filters.jl:764-775: tapsPerPhi taps of tap_dtype
 * for a phase in [0, Nphi+1] (host evaluation; MRHIP_ERR_INVALID_ARG outside the range like :765); complex taps: tapsPerPhi
 * complex taps, the statement per component; per-channel taps (mrhip_create_farrow_bank, mrhip_create_farrow_bank_ctaps): nchannels
 * rows of tapsPerPhi taps */
int mrhip_farrow_tapsforphase(const mrhip_filter *f, double phase, void *host_out);
/* replaces tapsforphase(kernel::FIRArbitrary, phase), src/Filters.jl:677-690: (alpha, phiIdx) = modf(phase);
 * taps[i] = pfb[i, phiIdx] + alpha * dpfb[i, phiIdx], evaluated in Float64 (alpha is a Float64 there) and stored in
 * tap_dtype (complex taps: tapsPerPhi complex taps, the statement per component).  phase outside [0, Nphi+1] is
 * MRHIP_ERR_INVALID_ARG (:678); so is a phase whose integer part is not a column of the bank (0 or Nphi+1: a BoundsError in
 * the reference). */
int mrhip_arbitrary_tapsforphase(const mrhip_filter *f, double phase, void *host_out);
void mrhip_destroy(mrhip_filter *f);

/* ---- bookkeeping ---------------------------------------------------------------------- */
/* replaces outputlength(self::FIRFilter, inputlength), src/Filters.jl:359-385 (per channel).
 * For ARBITRARY this is the reference's ceil((n - deficit + 1) * rate) estimate (:375-377). */
int64_t mrhip_outputlength(const mrhip_filter *f, int64_t inputlength);
/* exact number of samples the next filt call with `inputlength` samples will write per channel
 * (== outputlength for the rational family when inputlength >= inputDeficit, else 0; for ARBITRARY it
 * runs the phase recurrence of update(), src/Filters.jl:663-673, without touching the state). */
int64_t mrhip_next_output_count(const mrhip_filter *f, int64_t inputlength);
/* Advance the stream state exactly as a filt! call over `inputlength` samples per channel would -- the state updates at
 * the end of every filt! (src/Filters.jl:472 Standard: none, :515-516 Interpolator, :571-572 Rational, :647-648 Decimator,
 * :731-735 Arbitrary, :836-838 Farrow) -- WITHOUT data and without touching the history: returns the number of outputs
 * that call would have written per channel, or -1.  The state machine is data independent, so a stream can be entered
 * at any sample: advance to it, mrhip_set_history with the tapsPerPhi-1 samples in front of it (support.jl:61-80 is
 * all a later call sees of the earlier ones), filt from there -- what sharding.py's TimeShardedFilter does per GPU. */
int64_t mrhip_advance_state(mrhip_filter *f, int64_t inputlength);
/* replaces inputlength(self::FIRFilter, outputlength), src/Filters.jl:403-422 */
int64_t mrhip_inputlength(const mrhip_filter *f, int64_t outputlength);
int mrhip_get_state(const mrhip_filter *f, mrhip_state *st);
/* restore a stream position (phiIdx, inputDeficit; phiAccumulator for ARBITRARY, from which
 * phiIdx and alpha are re-derived as update() does).  The reference has no such call; it is the
 * working counterpart of setphase/reset (src/Filters.jl:210-260, several of which are broken). */
int mrhip_set_state(mrhip_filter *f, int64_t phiIdx, int64_t inputDeficit, double phiAccumulator);
/* copy the history vectors (FIRFilter.history, src/Filters.jl:153) of all channels to / from a
 * host buffer laid out [nchannels][historyLen] in sample_dtype.  Synchronous. */
int mrhip_get_history(mrhip_filter *f, void *host_out);
int mrhip_set_history(mrhip_filter *f, const void *host_in);
/* the same from DEVICE memory on f's device, asynchronous on `stream` (ordered behind the filter's earlier calls and ahead of
 * its next one): a halo that arrived over RCCL goes into the filter without touching the host (sharding.py). */
int mrhip_set_history_device(mrhip_filter *f, const void *device_in, void *stream);
/* replaces reset(self::FIRFilter), src/Filters.jl:256-260: zero history; state back to the
 * constructor's (the reference resets 𝜙Idx only and is broken for FIRArbitrary, :247-253). */
int mrhip_reset(mrhip_filter *f);
int mrhip_set_numerics(mrhip_filter *f, int numerics);
/* FIRArbitrary / FIRFarrow: which floating-point mod() update() wraps the phase accumulator with (src/Filters.jl:668, :786).
 * form 0 (default): the exact remainder -- Julia >= 0.4.  form 1: rem(y + rem(x, y), y) -- how Julia's Base computed mod() for
 * floats before 0.4; the reference is Julia-0.3 code and nothing in its tree says which Base it ran on.  The two agree bit for bit
 * whenever Nphi is a power of two (BASELINE config 4: Nphi = 32); for other Nphi form 1 differs by one rounding of y + rem(x, y)
 * every few outputs (a random walk of ~1e-10 phase steps per 1e6 outputs).  With form 1 and such an Nphi the phase schedule is
 * evaluated by the host's serial loop (the device evaluation implements the exact remainder) and asynchronous / captured calls
 * are MRHIP_ERR_UNSUPPORTED.  The oracle has the same switch (oracle.set_mod_form). */
int mrhip_set_mod_form(mrhip_filter *f, int form);
/* the polyphase taps as stored on the device, converted back to tap_dtype (which = 0: h flipped or
 * pfb; which = 1: dpfb).  Column-major tapsPerPhi x Nphi.  For tests / tapsforphase. */
int mrhip_get_taps(mrhip_filter *f, int which, void *host_out);

/* ---- the hot path --------------------------------------------------------------------- */
/* replaces filt!(buffer, self, x) for all five kernels, src/Filters.jl:450,489,536,598,693,
 * on DEVICE memory: x and y are device pointers on f's device; channel c is read from
 * x + c*x_stride and written to y + c*y_stride (strides in samples).  y holds elements of
 * output_dtype.  y_capacity is the per-channel room in y; if it is smaller than the number of
 * samples the call will produce the call fails with MRHIP_ERR_BUFFER_TOO_SMALL and the filter
 * state is unchanged (reference: error() before the loop, :460,:503,:550).
 * *n_written receives the per-channel output count (the Int that the Rational/Decimator/
 * Arbitrary filt! return, :574,:630,:741; xLen resp. L*xLen for Standard/Interpolator).  It is a
 * pure function of (state, x_len) and is valid on return even though the kernels are only
 * enqueued: the call is asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * A short input (x_len < inputDeficit) is not an error: history is shifted, inputDeficit
 * reduced, *n_written = 0 (:543-547, :638-643, :705-709).
 * Only the outputs are written: like the reference's filt!, which writes buffer[1:n] and nothing else, every entry point
 * (mrhip_filt_device, _async, _chained, _chunked, _multi, mrhip_ring_push*, mrhip_cascade_filt_device*) leaves the elements of y
 * outside [0, count) of each channel row untouched -- whatever the alignment of y, whatever y_stride >= the required minimum
 * (count; mrhip_outputlength_bound(x_len) for a device-planned call), also between count and y_capacity, also where the launch is
 * sized for an estimate or a bound of the count, and also when the call fails with MRHIP_ERR_BUFFER_TOO_SMALL.  A caller may
 * filter into a slice of a larger buffer and lay the outputs of consecutive calls end to end (tests/test_gpu_output_bounds.py).
 * On a stream that is being captured into a HIP graph the call takes the device-planned path of mrhip_filt_device_async
 * (same buffer rule); *n_written then is the count of the FIRST replay (rational family) or -1 (FIRArbitrary / FIRFarrow:
 * read it with mrhip_sync_state after a replay). */
int mrhip_filt_device(mrhip_filter *f, const void *x, int64_t x_len, int64_t x_stride, void *y,
                      int64_t y_capacity, int64_t y_stride, int64_t *n_written, void *stream);
/* filt!(buffer, self, x) with NOTHING returned to the host: the call is planned ON THE DEVICE.  The reference mutates
 * 𝜙Idx / inputDeficit / 𝜙Accumulator at the end of every filt! (src/Filters.jl:571-572, 627-628, 734-735, update() :663-673);
 * here that state has a device-resident record per filter that every call keeps current in stream order.  This entry reads
 * the record in a one-lane plan kernel in front of the filter kernel (FIRArbitrary / FIRFarrow: in the kernels that evaluate
 * the phase schedule), advances it there, and never makes the host wait -- so a loop of such calls only enqueues, and the
 * same calls captured into a HIP graph replay correctly at ANY fixed chunk size and for every kind (mrhip_filt_device on a
 * capturing stream takes this path by itself).  The count is data independent but state dependent, so:
 *   - y_capacity (and y_stride for nchannels > 1) must be at least mrhip_outputlength_bound(x_len), else
 *     MRHIP_ERR_BUFFER_TOO_SMALL and nothing is enqueued (the reference's filt sizes its buffer from outputlength the same
 *     way, src/Filters.jl:744-751);
 *   - *count_out, if not NULL, must be DEVICE-ACCESSIBLE memory (hipMalloc or hipHostMalloc): the per-channel output count
 *     is stored there in stream order; mrhip_sync_state returns the last call's count as well;
 *   - the host-side view of the state (mrhip_get_state, outputlength, ...) re-reads the record when next asked, which
 *     waits for the filter's stream (after a capture: for the device).
 * A call longer than one launch (2^30 samples; 2^24 / rate for FIRArbitrary) is MRHIP_ERR_UNSUPPORTED here. */
int mrhip_filt_device_async(mrhip_filter *f, const void *x, int64_t x_len, int64_t x_stride, void *y,
                            int64_t y_capacity, int64_t y_stride, int64_t *count_out, void *stream);
/* The second stage of a device-resident chain (filt(f2, filt(f1, x)) in the reference's terms: the caller passes one filter's
 * output Vector to the next, src/Filters.jl:744-751): `f`'s input is what `prev`'s latest asynchronous or captured call --
 * earlier on the same stream -- wrote, and its LENGTH is that call's count, which only the device knows.  x_len_bound =
 * mrhip_outputlength_bound(prev, prev's input length): the launch is sized for it, and y_capacity / y_stride must cover
 * mrhip_outputlength_bound(f, x_len_bound).  `f` and `prev`: any kind (FIRArbitrary / FIRFarrow lay their phase
 * schedule out for the device-side length in the kernels that evaluate it); same count_out / state rules
 * as mrhip_filt_device_async.  With it a chain of filters runs, and replays from a HIP graph, at any chunk size without
 * the host learning a single count. */
int mrhip_filt_device_chained(mrhip_filter *f, const mrhip_filter *prev, const void *x, int64_t x_len_bound, int64_t x_stride,
                              void *y, int64_t y_capacity, int64_t y_stride, int64_t *count_out, void *stream);
/* filt!(buffer_i, self_i, x_i) for i = 0..n-1 -- n INDEPENDENT FIRFilter objects, each with its own phase, input deficit,
 * history and call length, the reference's one-FIRFilter-per-signal streaming usage (README.md:87-141) -- issued as ONE
 * launch when the filters agree in kind (the rational family: FIRStandard, FIRDecimator, FIRInterpolator, FIRRational), ratio,
 * tapsPerPhi, dtypes, numerics and device:
 * every workgroup of the launch works for one of the streams.  x[i] / y[i] are device pointers, channel c of filter i at
 * x[i] + c*x_len[i] and y[i] + c*y_capacity[i]; n_written[i] (optional) receives filter i's per-channel count.  Results,
 * states and histories are exactly those of n mrhip_filt_device calls, which is also what runs when the filters do not agree
 * (and inside a HIP-graph capture).  MRHIP_ERR_BUFFER_TOO_SMALL before anything is enqueued. */
int mrhip_filt_device_multi(mrhip_filter *const *filters, int n, const void *const *x, const int64_t *x_len, void *const *y,
                            const int64_t *y_capacity, int64_t *n_written, void *stream);
/* the largest per-channel output count a call of `inputlength` samples can have whatever the stream state: outputlength
 * (src/Filters.jl:352-385) evaluated for 𝜙Idx = inputDeficit = 1 (+ 2 for FIRArbitrary / FIRFarrow, whose outputlength is
 * an estimate, :375-381) */
int64_t mrhip_outputlength_bound(const mrhip_filter *f, int64_t inputlength);
/* filt! on every channel of a filter with per-channel rates (mrhip_create_arbitrary_rates, mrhip_create_farrow_rates), each channel from its own state, on
 * device memory; enqueued on `stream`.  Nothing waits, with one exception: the filter keeps two schedule buffers on the device that
 * hold nchannels slices of the call's bound -- 12 bytes per (channel, possible output), allocated a quarter larger than the largest call
 * so far needs: about 1.4 GB for 4096 channels x 1e4 samples at rates up to 2.25, about 2.2 GB for 64 x 1e6 -- and a call that needs
 * larger ones than the filter has waits on the host for the filter's stream, frees them and allocates anew.  Calls of one size pay
 * that once.
 *   - counts_out: NULL, or device-accessible memory for nchannels counts, stored in stream order;
 *   - y_capacity (and y_stride for nchannels > 1) must be at least mrhip_outputlength_bound(f, x_len) -- on this filter the largest of
 *     the channels' bounds -- else MRHIP_ERR_BUFFER_TOO_SMALL: nothing is enqueued and the state is unchanged;
 *   - row c of y receives elements [0, count_c) and nothing else;
 *   - with mrhip_set_timing, ONE bracket holds both launches of a call, the schedule kernel's walk and the filter kernel:
 *     mrhip_timing_read counts a call as one launch and its duration includes the walk;
 *   - a call whose bound exceeds 2^24 outputs per channel (the schedule-entry limit of a launch) returns MRHIP_ERR_UNSUPPORTED, and so
 *     does a call on a capturing stream. */
int mrhip_filt_device_rates(mrhip_filter *f, const void *x, int64_t x_len, int64_t x_stride,
                            void *y, int64_t y_capacity, int64_t y_stride, int64_t *counts_out, void *stream);
/* Per-channel input lengths for the filters with per-channel rates: mrhip_filt_device_rates with channel c fed x_c[0 : x_lens[c]) --
 * receivers off their own clocks deliver different numbers of samples per interval, and the caller feeds what arrived.  x_lens is a
 * HOST array of nchannels lengths; x holds the rows x_stride apart as before.
 *   - parity: channel c is bit for bit mrhip_create_arbitrary(h, rates[c], Nphi, nchannels = 1) -- mrhip_create_farrow(...) for the
 *     FIRFarrow filter -- fed x_c[0 : x_lens[c]): the outputs, the count of every call, the end state (inputDeficit, phiAccumulator,
 *     xIdx) and the history, under STRICT and under FUSED.  That includes the short-input path of filt! (src/Filters.jl:705-709,
 *     :805-809) per channel, and FIRFarrow's zero-start seam on every call;
 *   - a channel with x_lens[c] == 0 keeps its state and its history and files a count of 0, whatever its neighbours do;
 *   - when all lengths are equal the result is that of mrhip_filt_device_rates at that length;
 *   - the bound of a call is mrhip_outputlength_bound(f, the largest of x_lens): y_capacity (and y_stride for nchannels > 1) must
 *     reach it, else MRHIP_ERR_BUFFER_TOO_SMALL.  Row c of y receives elements [0, count_c) and nothing else; samples of row c of x
 *     at and behind x_lens[c] are not used;
 *   - refused before anything is enqueued or any state moves, each with a message that names this function: a NULL f or x_lens, a
 *     filter without per-channel rates, a negative length or y_capacity, x NULL with a length above 0, x_stride below the largest
 *     length for nchannels > 1 (all MRHIP_ERR_INVALID_ARG); a length of 2^31-1 or more, a capturing stream, a bound above 2^24
 *     (MRHIP_ERR_UNSUPPORTED); capacity or stride below the bound (MRHIP_ERR_BUFFER_TOO_SMALL);
 *   - x_lens may be reused or freed when the call returns: the library copies it into one of FOUR pinned staging slots it owns, used in
 *     turn, and from there, in stream order on `stream`, into the filter's one device array of lengths that the kernels read.  The
 *     call waits on the host where mrhip_filt_device_rates does (growth of the schedule buffers) and in one more place: for a staging
 *     slot whose upload, four ragged calls back, has not run yet;
 *   - the launches, the kernels (mrhip_last_kernel_name: the same four names), the timing bracket, mrhip_get_channel_states,
 *     mrhip_set_channel_states, mrhip_set_channel_rates and mrhip_reset are those of mrhip_filt_device_rates, and the two calls mix
 *     freely on one filter.  A ragged call sizes its grid by the longest channel and skips the tiles behind a channel's count;
 *   - left out on purpose: lengths that live on the device; compacting the tiles of channels that end early; graph capture,
 *     cascades, rings and sharding.  (Since added: lengths that live on the device, and such a filter behind another filter --
 *     mrhip_filt_device_rates_lens_device and mrhip_filt_device_rates_chained, "Input lengths from device memory, and chaining, for
 *     the filters with per-channel rates" below.) */
int mrhip_filt_device_rates_ragged(mrhip_filter *f, const void *x, const int64_t *x_lens /* HOST, [nchannels] */, int64_t x_stride,
                                   void *y, int64_t y_capacity, int64_t y_stride, int64_t *counts_out, void *stream);
/* the nchannels states of such a filter, after waiting for the filter's stream; MRHIP_ERR_BUFFER_TOO_SMALL if a channel's walk ever
 * overran the bound of its call (its outputs were clipped at the bound) */
int mrhip_get_channel_states(mrhip_filter *f, mrhip_channel_state *out /* [nchannels] */);
/* per-channel inputDeficit (>= 1) and phiAccumulator (in [1, Nphi+1)), behind the calls already enqueued; phiIdx and alpha are
 * re-derived as update() does (src/Filters.jl:671-672): floor(phiAccumulator) and the remainder */
int mrhip_set_channel_states(mrhip_filter *f, const int64_t *inputDeficit, const double *phiAccumulator);
/* new rates for a filter with per-channel rates (either constructor), behind the calls already enqueued (it waits for the filter's
 * stream as mrhip_set_channel_states does): rate and delta = Nphi / rate of every channel are rewritten; phiAccumulator, inputDeficit,
 * history and taps stay.  The checks are the constructors' (any rate <= 0 or not finite: MRHIP_ERR_INVALID_ARG, below 2^-30:
 * MRHIP_ERR_UNSUPPORTED; nothing is changed then).  mrhip_outputlength_bound follows the new largest rate, and a later call that
 * outgrows the schedule buffers reallocates them by the rule above.  After the call channel c continues bit for bit as the one-channel
 * filter constructed at the new rates[c] would, given channel c's (inputDeficit, phiAccumulator) through mrhip_set_state and its
 * history through mrhip_set_history.  mrhip_reset restores the constructor state and KEEPS the current rates.  A filter without
 * per-channel rates: MRHIP_ERR_INVALID_ARG. */
int mrhip_set_channel_rates(mrhip_filter *f, const double *rates /* [nchannels] */);
/* Per-channel taps with per-channel rates for FIRArbitrary (mrhip_set_channel_taps on a filter of mrhip_create_arbitrary_rates): one
 * FIRFilter(h_c, rates[c], Nphi) per channel behind one handle, taps AND rate differing per channel -- receivers each off its own clock
 * and each with its own front-end equaliser or calibration filter, per-emitter Doppler time-scale correction with the emitter's own
 * matched pulse; and taps that adapt at run time (a block-LMS equaliser) as the rates do through mrhip_set_channel_rates.  The feature
 * is a CALL on an existing filter, the twin of mrhip_set_channel_rates, not a constructor.
 *   - h holds nchannels rows of hLen taps, row-major, row c = h_c: the layout of mrhip_create_arbitrary_bank;
 *   - filter kinds: f must come from mrhip_create_arbitrary_rates.  A filter of mrhip_create_farrow_rates* answers MRHIP_ERR_UNSUPPORTED
 *     (not this call's: it needs the fit of every row; the message names mrhip_set_channel_taps_farrow and mrhip_set_channel_pnfb, which
 *     take such a filter -- "Per-channel taps with per-channel rates for FIRFarrow", below); any other filter
 *     answers MRHIP_ERR_INVALID_ARG, "mrhip_set_channel_taps takes a filter of mrhip_create_arbitrary_rates";
 *   - argument checks: h == NULL is MRHIP_ERR_INVALID_ARG; hLen other than the filter's hLen is MRHIP_ERR_INVALID_ARG (tapsPerPhi, the
 *     history length and the history do not change); a complex tap_dtype is MRHIP_ERR_UNSUPPORTED (complex taps with per-channel rates
 *     are left out); a real tap_dtype other than the filter's is MRHIP_ERR_INVALID_ARG;
 *   - effect: every row goes through dh_c = [diff(h_c), 0] in the tap type and the two taps2pfb calls, exactly as
 *     mrhip_create_arbitrary_bank builds and widens its banks; the call waits for the filter's stream (as mrhip_set_channel_rates
 *     does), then installs nchannels pfb and nchannels dpfb banks on the device: nchannels * 2 * Nphi * tapsPerPhi * sizeof(R) bytes,
 *     allocated by the first call and reused by every later one.  Everything that can fail -- the checks, the host banks, the first
 *     call's allocation -- happens BEFORE anything of the filter changes: a refused or failed call leaves the filter bit for bit as
 *     it was;
 *   - parity: from the next call on channel c is bit for bit mrhip_create_arbitrary(h_c, rates[c], Nphi, nchannels = 1) fed x_c, that
 *     filter given channel c's (inputDeficit, phiAccumulator) through mrhip_set_state and its history through mrhip_set_history:
 *     the outputs, the count of every call, the end state and the history, under STRICT and under FUSED, through
 *     mrhip_filt_device_rates and mrhip_filt_device_rates_ragged, including the short-input path of filt! (src/Filters.jl:705-709)
 *     and a channel of ragged length 0;
 *   - state: phiAccumulator, inputDeficit, rates and history stay untouched.  Called again the function replaces the taps: they may
 *     change between calls.  mrhip_reset keeps the current taps, as it keeps the current rates.  mrhip_set_channel_rates,
 *     mrhip_set_channel_states, mrhip_set_numerics, mrhip_set_history*, mrhip_outputlength_bound and mrhip_set_mod_form work as before;
 *   - tap queries: after a successful call mrhip_get_taps and mrhip_arbitrary_tapsforphase answer in the layout of "Per-channel taps
 *     for FIRArbitrary" -- nchannels banks or rows one after the other; before it they answer as on any filter of
 *     mrhip_create_arbitrary_rates;
 *   - kernels: arb_rates_bank_generic (any shape) and arb_rates_bank_tiled (ONE channel's two banks in LDS, reloaded when a
 *     workgroup's run crosses into another channel; MRHIP_ARB_RATES_BANK_TILED = 1 selects it wherever its plan fits);
 *     MRHIP_FORCE_GENERIC = 1 keeps the universal one;
 *   - a filter on which the function was never called runs the launches, kernels and messages it always ran; every entry point that
 *     refuses a filter with per-channel rates keeps refusing; the ABI version stays 1;
 *   - left out on purpose: FIRFarrow (it has its own two calls, below); complex taps; going back to shared taps; a stream-ordered update without the host wait (it
 *     needs double-buffered banks); graph capture, rings, cascades and sharding; the parallel schedule for long channels. */
int mrhip_set_channel_taps(mrhip_filter *f, const void *h /* [nchannels][hLen] */, int64_t hLen, int tap_dtype);
/* Per-channel taps with per-channel rates for FIRFarrow (mrhip_set_channel_taps_farrow and mrhip_set_channel_pnfb on a filter of
 * mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb): one FIRFilter(h_c, rates[c], Nphi, polyorder) per channel behind one
 * handle, taps AND rate differing per channel.  FIRFarrow is the kernel the reference offers for a continuously variable rate: Doppler
 * and clock trackers that call mrhip_set_channel_rates every chunk and carry a per-emitter matched pulse or a per-receiver equaliser.
 * Both are CALLS on an existing filter, the twins of mrhip_set_channel_taps / mrhip_set_channel_rates, not constructors.
 *   - mrhip_set_channel_taps_farrow: h holds nchannels rows of hLen taps, row-major, row c = h_c (the layout of
 *     mrhip_create_farrow_bank).  Every row goes through taps2pfb and one polynomial fit per row of it, then the rounding to the tap
 *     type, exactly as mrhip_create_farrow_bank builds its banks: bank c is bit for bit the bank of mrhip_create_farrow(h_c, ...).  A
 *     rank-deficient fit is MRHIP_ERR_INVALID_ARG;
 *   - mrhip_set_channel_pnfb: pnfb holds nchannels caller-fitted banks one after the other, [nchannels][tapsPerPhi][polyorder+1] Float64
 *     in ascending powers, rounded to the tap type as mrhip_create_farrow_pnfb rounds: the path of a block-adaptive user who updates
 *     coefficients directly, and of a test that hands an oracle and the device the same numbers;
 *   - refusals, each before anything changes, in this order, each message naming the function: f == NULL is MRHIP_ERR_INVALID_ARG; a
 *     filter of mrhip_create_arbitrary_rates is MRHIP_ERR_INVALID_ARG with a message that points to mrhip_set_channel_taps; any other
 *     filter is MRHIP_ERR_INVALID_ARG; then h / pnfb == NULL (MRHIP_ERR_INVALID_ARG); then hLen, or tapsPerPhi and polyorder, other
 *     than the filter's (MRHIP_ERR_INVALID_ARG: the history length and the history do not change); then (mrhip_set_channel_taps_farrow)
 *     the tap dtype: out of range MRHIP_ERR_INVALID_ARG, complex MRHIP_ERR_UNSUPPORTED (complex taps with per-channel rates are left
 *     out), a real type other than the filter's MRHIP_ERR_INVALID_ARG;
 *   - effect: the checks, the host banks (the fit included) and the first call's allocation come first; then the call waits for the
 *     filter's stream (as mrhip_set_channel_rates does) and uploads nchannels * tapsPerPhi * (polyorder+1) Float64, allocated by the
 *     first call of either function and reused by every later one; the one shared bank is freed.  A refused or failed call leaves the
 *     filter bit for bit as it was;
 *   - parity: from the next call on channel c is bit for bit mrhip_create_farrow_pnfb(bank_c, rates[c], Nphi, polyorder, nchannels = 1)
 *     fed x_c, that filter given channel c's (inputDeficit, phiAccumulator) through mrhip_set_state and its history through
 *     mrhip_set_history: the outputs, the count of every call, the end state and the history, under STRICT and under FUSED, through
 *     mrhip_filt_device_rates and mrhip_filt_device_rates_ragged, including the short-input path, a channel of ragged length 0 and
 *     FIRFarrow's zero-start seam on every call;
 *   - arithmetic: that of "Per-channel rates for FIRFarrow" on bank c -- Horner in Float64, never fused, also under FUSED; the tap
 *     rounded once to the tap type and widened exactly; the dot oldest sample first; STRICT a separate multiply and add per tap, FUSED
 *     one explicit fma per tap;
 *   - state: phiAccumulator, inputDeficit, rates and history stay untouched.  Either function may be called again, so the taps may
 *     change between calls.  mrhip_reset keeps the current taps, as it keeps the current rates.  mrhip_set_channel_rates,
 *     mrhip_set_channel_states, mrhip_get_channel_states, mrhip_set_numerics, mrhip_set_history*, mrhip_outputlength_bound and both
 *     mrhip_filt_device_rates* calls work as before;
 *   - tap queries: after a successful call mrhip_get_pnfb and mrhip_farrow_tapsforphase answer in the layout of "Per-channel taps for
 *     FIRFarrow" -- nchannels banks or rows one after the other; before it they answer as on any filter of mrhip_create_farrow_rates*;
 *   - kernels: farrow_rates_bank_generic (any shape) and farrow_rates_bank_multi (four outputs a lane share each tap's scalar
 *     coefficient loads, a tile is one channel and so one bank; MRHIP_FARROW_RATES_BANK_MULTI = 1 selects it wherever its plan fits, 0
 *     never, the default rule follows the measured rows); MRHIP_FORCE_GENERIC = 1 keeps the universal one;
 *   - mrhip_set_channel_taps keeps answering MRHIP_ERR_UNSUPPORTED for a FIRFarrow filter; a filter on which neither function was
 *     called runs the launches and kernels it always ran; the ABI version stays 1; there are still sixteen constructors;
 *   - complex banks: mrhip_set_channel_ctaps_farrow and mrhip_set_channel_pnfb_ctaps* (below);
 *   - left out on purpose: going back to shared taps; a stream-ordered update without the host
 *     wait (it needs double-buffered banks); the fit on the device; graph capture, rings, cascades and sharding; the parallel schedule
 *     for long channels.  (Since added: the fit on the device, mrhip_set_channel_taps_farrow_device below.) */
int mrhip_set_channel_taps_farrow(mrhip_filter *f, const void *h /* [nchannels][hLen] */, int64_t hLen, int tap_dtype);
int mrhip_set_channel_pnfb(mrhip_filter *f, const double *pnfb /* [nchannels][tapsPerPhi][polyorder+1] */, int64_t tapsPerPhi, int64_t polyorder);
/* Device-resident updates for the filters with per-channel rates (mrhip_create_arbitrary_rates, mrhip_create_farrow_rates*, with or
 * without per-channel taps).  A Doppler or clock tracker, or a block-LMS equaliser, computes the next rates and taps on the GPU from the
 * last chunk's outputs; mrhip_set_channel_rates, mrhip_set_channel_taps and mrhip_set_channel_pnfb take HOST arrays and wait for the
 * filter's stream, once per chunk.  The three calls below take DEVICE pointers and enqueue on `stream`: a loop of filter call, tracker,
 * update, filter call runs without the host learning anything or waiting for anything (what mrhip_filt_device_async is to the one-rate
 * filters).  They answer the "stream-ordered update without the host wait" the sections above list as left out; no double-buffered banks
 * are needed, since the update kernel runs in stream order between the filter kernels.
 *   - ordering: each call adopts `stream` as mrhip_filt_device_rates does (a filter whose last call ran on another stream: `stream` waits
 *     for it through an event) and takes effect behind the calls already enqueued and ahead of every later one.  The device arrays are
 *     read in stream order: they must hold their values by then and may be overwritten by work enqueued on `stream` afterwards.  A
 *     capturing stream is MRHIP_ERR_UNSUPPORTED.  Every refusal comes before anything is enqueued or changed, its message naming the
 *     function;
 *   - mrhip_set_channel_rates_device: the host cannot see the values, so the caller declares the range they lie in, [rate_lo, rate_hi].
 *     MRHIP_ERR_INVALID_ARG: f or rates NULL, a filter without per-channel rates, rate_lo or rate_hi not finite or not > 0, rate_hi <
 *     rate_lo; MRHIP_ERR_UNSUPPORTED: rate_lo < 2^-30, a capturing stream.  From then on mrhip_outputlength_bound and the buffer checks
 *     of later calls follow rate_hi, the tiled kernels' plans rate_lo; a later mrhip_set_channel_rates replaces both.  On the device
 *     (rates_set_kernel, one lane per channel) channel c reads r = rates[c]; r finite and rate_lo <= r <= rate_hi: rate = r and delta =
 *     Nphi / r, one Float64 division, the operation mrhip_set_channel_rates performs; any other value: the channel KEEPS its rate and
 *     delta, and its record receives the status MRHIP_ERR_INVALID_ARG unless it holds an earlier one.  phiAccumulator, inputDeficit,
 *     xIdx, the count, the history and the taps are not touched.  A refused value never reaches the walk, an accepted one is inside the
 *     range the bound and the plans were sized for, and the overrun clip of the schedule kernel stays as the last line (it is what
 *     catches a refused channel whose OLD rate lies above the new rate_hi: declare a range that holds the rates in force as well);
 *   - reporting: mrhip_get_channel_states returns MRHIP_ERR_INVALID_ARG while a record holds that status ("a device-resident rate was
 *     refused ... the channel kept its rate"; the states are filled in all the same); an overrun keeps answering
 *     MRHIP_ERR_BUFFER_TOO_SMALL with its message and goes first.  mrhip_set_channel_states and mrhip_reset clear the refusal as they
 *     clear an overrun;
 *   - parity (rates): from the next call on channel c continues bit for bit as after mrhip_set_channel_rates with the same values --
 *     outputs, counts, states and history, under STRICT and FUSED, FIRArbitrary and FIRFarrow, shared and per-channel taps, through
 *     both mrhip_filt_device_rates* calls;
 *   - mrhip_set_channel_taps_device (FIRArbitrary): h holds nchannels rows of hLen taps in the filter's tap dtype, the layout of
 *     mrhip_set_channel_taps, whose checks apply unchanged; a FIRFarrow filter is MRHIP_ERR_UNSUPPORTED with a message that points to
 *     mrhip_set_channel_pnfb_device.  One kernel (rates_bank_build_kernel) writes what mrhip_set_channel_taps uploads, bit for bit: bank
 *     c holds at c*Nphi*T + phi*T + i the tap h_c[j], j = (T-1-i)*Nphi + phi, 0 for j >= hLen; the dpfb bank h_c[j+1] - h_c[j], one
 *     subtraction rounded in the tap type, 0 for j >= hLen-1; both widened exactly to the arithmetic type.  From the next call on the
 *     filter is bit for bit the filter after mrhip_set_channel_taps with the same matrix, and runs the same two kernels
 *     (arb_rates_bank_generic, arb_rates_bank_tiled);
 *   - mrhip_set_channel_pnfb_device (FIRFarrow): pnfb holds [nchannels][tapsPerPhi][polyorder+1] Float64, the layout and the checks of
 *     mrhip_set_channel_pnfb; a filter of mrhip_create_arbitrary_rates is MRHIP_ERR_INVALID_ARG with a message that points to
 *     mrhip_set_channel_taps_device.  One kernel copies the coefficients, rounding each to Float32 and widening it back on a filter with
 *     Float32 taps, as mrhip_set_channel_pnfb rounds.  Parity is with mrhip_set_channel_pnfb given the same array;
 *   - allocation: the FIRST tap or bank call on a filter whose taps are still shared allocates the nchannels banks and waits once, on
 *     the host, for the filter's stream; the shared pair (the shared bank) is freed right after that one wait -- it is not kept until
 *     mrhip_destroy.  Every later call enqueues one kernel and returns without waiting.  A failed allocation leaves the filter bit for
 *     bit as it was;
 *   - host copies: after a device install the host no longer holds the taps.  mrhip_get_taps and mrhip_arbitrary_tapsforphase
 *     (mrhip_get_pnfb and mrhip_farrow_tapsforphase) then wait for the filter's stream and read the banks back -- narrowing the
 *     arithmetic type to the tap type is exact -- and answer in the per-channel layouts.  A later host install makes the host copy
 *     current again.  mrhip_get_channel_states reports the rates the records hold;
 *   - a filter on which none of the three was called runs the launches and kernels it always ran; the ABI version stays 1; there are
 *     still sixteen constructors;
 *   - left out on purpose: input lengths that live on the device; the FIRFarrow fit on the device (a mrhip_set_channel_taps_farrow
 *     twin); updates from a stream other than the one the filter's calls run on without ordering by the caller (the device arrays are
 *     read on `stream`); graph capture; complex taps; the parallel schedule for long channels.  (Since added: input lengths that
 *     live on the device, mrhip_filt_device_rates_lens_device below; complex taps, the two sections that follow; the FIRFarrow fit on
 *     the device, mrhip_set_channel_taps_farrow_device below.) */
int mrhip_set_channel_rates_device(mrhip_filter *f, const double *rates /* DEVICE, [nchannels] */, double rate_lo, double rate_hi, void *stream);
int mrhip_set_channel_taps_device(mrhip_filter *f, const void *h /* DEVICE, [nchannels][hLen] */, int64_t hLen, int tap_dtype, void *stream);
int mrhip_set_channel_pnfb_device(mrhip_filter *f, const double *pnfb /* DEVICE, [nchannels][tapsPerPhi][polyorder+1] */, int64_t tapsPerPhi,
                                  int64_t polyorder, void *stream);
/* Complex per-channel taps with per-channel rates for FIRArbitrary (mrhip_set_channel_ctaps and mrhip_set_channel_ctaps_device on a
 * filter of mrhip_create_arbitrary_rates): one FIRFilter(h_c::Vector{Complex}, rates[c], Nphi) per channel behind one handle.  Doppler
 * is both at once: a time scale, which is a rate per channel, and a carrier offset, which is a prototype rotated to the channel's own
 * frequency; a tracker moves both every chunk.  Both are CALLS on an existing filter, the twins of mrhip_set_channel_taps and
 * mrhip_set_channel_taps_device, not constructors: there are still sixteen constructors and the ABI version stays 1.
 *   - h holds nchannels rows of hLen (re, im) pairs, row-major, row c = h_c: the layout of mrhip_create_arbitrary_bank_ctaps;
 *   - filter kinds: f must come from mrhip_create_arbitrary_rates, with or without earlier mrhip_set_channel_taps* calls.  A filter of
 *     mrhip_create_farrow_rates* answers MRHIP_ERR_UNSUPPORTED, "complex taps with per-channel rates for FIRFarrow are left out"; any
 *     other filter answers MRHIP_ERR_INVALID_ARG;
 *   - checks, in this order, each before anything changes, each message naming the function: f == NULL (MRHIP_ERR_INVALID_ARG); the
 *     filter kind (above); h == NULL (MRHIP_ERR_INVALID_ARG); hLen other than the filter's (MRHIP_ERR_INVALID_ARG: tapsPerPhi, the
 *     history length and the history do not change); the tap dtype, which must be the complex type of the filter's real tap precision
 *     -- Complex64 on a filter with Float32 taps, Complex128 on one with Float64 taps: out of range is MRHIP_ERR_INVALID_ARG, a real
 *     type MRHIP_ERR_INVALID_ARG with a message that points to mrhip_set_channel_taps, the other complex precision
 *     MRHIP_ERR_INVALID_ARG; last, a filter in FUSED numerics is MRHIP_ERR_UNSUPPORTED: complex taps have no FUSED form, as everywhere
 *     in the library ("Complex taps");
 *   - effect (mrhip_set_channel_ctaps): every row goes through dh_c = [diff(h_c), 0], per component in the tap's scalar type, and the
 *     two taps2pfb calls, exactly as mrhip_create_arbitrary_bank_ctaps builds its banks, widened exactly to R.  The filter then holds
 *     nchannels pfb and nchannels dpfb banks of (re, im) pairs: nchannels * 2 * Nphi * tapsPerPhi * 2 * sizeof(R) bytes, allocated by
 *     the first call of either function and reused by every later one.  The order of steps is mrhip_set_channel_taps': the checks, the
 *     host banks and the allocation come first; then ONE wait for the filter's stream; then the upload and the swap; the shared pair or
 *     the real banks are freed after the wait.  A refused or failed call leaves the filter bit for bit as it was;
 *   - from the next call on the filter's tap type is the complex one and the output element type is mrhip_output_dtype(tap_dtype,
 *     sample_dtype): a filter over REAL samples now writes COMPLEX outputs, and the caller's y must be of that type (y_capacity and
 *     y_stride count such elements).  mrhip_set_numerics(FUSED) answers MRHIP_ERR_UNSUPPORTED as on
 *     every complex-tap filter.  phiAccumulator, inputDeficit, the rates (installed from the host or from the device, with their
 *     declared range), the history, the schedule buffers and mrhip_outputlength_bound are untouched.  mrhip_reset keeps the taps.  Either
 *     function may be called again: the taps may change between calls.  mrhip_set_channel_states, mrhip_set_channel_rates and
 *     mrhip_set_channel_rates_device work as before;
 *   - parity: channel c continues bit for bit as mrhip_create_arbitrary_ctaps(h_c, rates[c], Nphi, nchannels = 1) fed x_c, that filter
 *     given channel c's (inputDeficit, phiAccumulator) and its history: the outputs, the count of every call, the end state and the
 *     history, through mrhip_filt_device_rates and mrhip_filt_device_rates_ragged, including the short-input path of filt!
 *     (src/Filters.jl:705-709) and a channel of ragged length 0.  STRICT only.  Arithmetic: that of "Complex taps" -- both dots over one
 *     window, oldest sample first, every multiply, add and subtract rounded separately in R, the combine per component in Float64;
 *   - tap queries: mrhip_get_taps and mrhip_arbitrary_tapsforphase answer in the layout of "Per-channel complex taps for FIRArbitrary"
 *     -- nchannels banks or rows of (re, im) pairs one after the other;
 *   - going back: mrhip_set_channel_taps and mrhip_set_channel_taps_device on a filter that holds complex taps answer
 *     MRHIP_ERR_UNSUPPORTED, "going back to real taps is left out" (no filter could be in that state before);
 *   - mrhip_set_channel_ctaps_device: h is a DEVICE pointer of the same layout.  The same checks, then the stream rules of
 *     mrhip_set_channel_taps_device: the call adopts `stream`, a capturing stream is MRHIP_ERR_UNSUPPORTED.  One kernel
 *     (rates_cbank_build_kernel) builds both complex banks in stream order, bit for bit what mrhip_set_channel_ctaps uploads: bank c
 *     holds at c*Nphi*T + phi*T + i the pair h_c[j], j = (T-1-i)*Nphi + phi, (0, 0) for j >= hLen; the dpfb bank h_c[j+1] - h_c[j], one
 *     subtraction per component rounded in the tap's scalar type, (0, 0) for j >= hLen-1.  The first call on a filter that does not hold
 *     complex banks yet allocates them, waits once for the filter's stream and flips the type; every later call enqueues one kernel and
 *     returns.  Afterwards the host copy is stale and the tap queries wait for the stream and read the banks back;
 *   - kernels: arb_rates_ctaps_generic (any shape) and arb_rates_ctaps_tiled (ONE channel's two banks of pairs in LDS, reloaded when a
 *     workgroup's run crosses into another channel; MRHIP_ARB_RATES_CTAPS_TILED = 1 selects it wherever its plan fits, 0 never, the
 *     default rule follows the measured rows: from 225 024 tiles, up to 879 tiles a channel);
 *     MRHIP_FORCE_GENERIC = 1 keeps the universal one;
 *   - a filter on which neither function was called runs the launches, kernels and messages it always ran: mrhip_set_channel_taps,
 *     mrhip_set_channel_taps_farrow, mrhip_set_channel_taps_device and the constructors keep answering a complex tap dtype with
 *     MRHIP_ERR_UNSUPPORTED;
 *   - FIRFarrow with complex taps and per-channel rates: the three calls of the next section;
 *   - left out on purpose: one shared complex tap vector without a bank per channel
 *     (install the same row nchannels times); going back to real taps; a FUSED form; graph capture, rings, cascades and sharding;
 *     lengths on the device; the parallel schedule for long channels. */
int mrhip_set_channel_ctaps(mrhip_filter *f, const void *h /* [nchannels][hLen] (re, im) */, int64_t hLen, int tap_dtype);
int mrhip_set_channel_ctaps_device(mrhip_filter *f, const void *h /* DEVICE, same layout */, int64_t hLen, int tap_dtype, void *stream);
/* Complex per-channel taps with per-channel rates for FIRFarrow (mrhip_set_channel_ctaps_farrow, mrhip_set_channel_pnfb_ctaps and
 * mrhip_set_channel_pnfb_ctaps_device on a filter of mrhip_create_farrow_rates*): one FIRFilter(h_c::Vector{Complex}, rates[c], Nphi,
 * polyorder) per channel behind one handle.  FIRFarrow is the kernel the reference offers for a continuously variable rate, and Doppler
 * is a time scale AND a carrier offset: the matched pulse or equaliser of channel c is a complex prototype rotated to that channel's
 * frequency, and a tracker moves the rate every chunk.  The three are CALLS on an existing filter, the twins of
 * mrhip_set_channel_taps_farrow, mrhip_set_channel_pnfb and mrhip_set_channel_pnfb_device, not constructors: there are still sixteen
 * constructors and the ABI version stays 1.  This completes the table of the per-channel-rate filters.
 *   - layouts: h holds nchannels rows of hLen (re, im) pairs, row-major, row c = h_c (mrhip_create_farrow_bank_ctaps); pnfb holds
 *     [nchannels][tapsPerPhi][polyorder+1] (re, im) pairs of Float64, ascending powers ("Per-channel complex taps for FIRFarrow");
 *   - filter kinds: f must come from mrhip_create_farrow_rates or mrhip_create_farrow_rates_pnfb, with or without earlier
 *     mrhip_set_channel_taps_farrow / mrhip_set_channel_pnfb* calls.  A filter of mrhip_create_arbitrary_rates answers
 *     MRHIP_ERR_INVALID_ARG with a message that points to mrhip_set_channel_ctaps; any other filter answers MRHIP_ERR_INVALID_ARG;
 *   - checks, in this order, each before anything changes, each message naming the function: f == NULL (MRHIP_ERR_INVALID_ARG); the
 *     filter kind (above); h or pnfb == NULL (MRHIP_ERR_INVALID_ARG); hLen, or tapsPerPhi and polyorder, other than the filter's
 *     (MRHIP_ERR_INVALID_ARG: the history length and the history do not change); mrhip_set_channel_ctaps_farrow only, the tap dtype,
 *     which must be the complex type of the filter's tap precision -- out of range is MRHIP_ERR_INVALID_ARG, a real type
 *     MRHIP_ERR_INVALID_ARG with a message that points to mrhip_set_channel_taps_farrow, the other complex precision
 *     MRHIP_ERR_INVALID_ARG; last, a filter in FUSED numerics is MRHIP_ERR_UNSUPPORTED: complex taps have no FUSED form ("Complex
 *     taps").  The two pnfb calls take no dtype: the filter becomes Complex64 over Float32 taps and Complex128 over Float64 taps;
 *   - effect (mrhip_set_channel_ctaps_farrow): every row goes through taps2pfb and the fit per component, then the rounding to the
 *     tap's scalar, exactly as mrhip_create_farrow_bank_ctaps builds its banks: bank c is bit for bit the bank of
 *     mrhip_create_farrow_ctaps(h_c, ...).  A rank-deficient fit is MRHIP_ERR_INVALID_ARG.  mrhip_set_channel_pnfb_ctaps: every
 *     coefficient component is rounded as mrhip_create_farrow_pnfb_ctaps rounds.  The filter then holds nchannels * tapsPerPhi *
 *     (polyorder+1) pairs of Float64, allocated by the first of the three calls and reused by every later one.  The order of steps is
 *     mrhip_set_channel_pnfb's: the checks, the host banks and the allocation come first; then ONE wait for the filter's stream; then
 *     the upload and the swap; the one shared bank or the real banks are freed after the wait.  A refused or failed call leaves the
 *     filter bit for bit as it was;
 *   - mrhip_set_channel_pnfb_ctaps_device: pnfb is a DEVICE pointer of the same layout.  The same checks, then the stream rules of
 *     mrhip_set_channel_pnfb_device: the call adopts `stream`, a capturing stream is MRHIP_ERR_UNSUPPORTED.  The kernel is that of
 *     mrhip_set_channel_pnfb_device (rates_pnfb_install_kernel) over twice as many doubles -- the rounding is per component.  The first
 *     install on a filter that does not hold complex banks yet allocates them, waits once for the filter's stream and flips the type;
 *     every later call enqueues one kernel and returns.  Afterwards the host copy is stale and the tap queries wait for the stream and
 *     read the banks back.  Parity is with mrhip_set_channel_pnfb_ctaps given the same array;
 *   - from the next call on the filter's tap type is the complex one and the output element type is mrhip_output_dtype(tap, sample):
 *     a filter over REAL samples now writes COMPLEX outputs, and the caller's y must be of that type (y_capacity and y_stride count
 *     such elements).  mrhip_set_numerics(FUSED) answers MRHIP_ERR_UNSUPPORTED as on every complex-tap filter.  phiAccumulator,
 *     inputDeficit, the rates (installed from the host or from the device, with their declared range), the history, the schedule
 *     buffers and mrhip_outputlength_bound are untouched.  mrhip_reset keeps the taps.  Any of the three may be called again: the
 *     taps may change between calls;
 *   - parity: channel c continues bit for bit as mrhip_create_farrow_pnfb_ctaps(bank_c, rates[c], Nphi, polyorder, nchannels = 1) fed
 *     x_c, that filter given channel c's (inputDeficit, phiAccumulator) and its history: the outputs, the count of every call, the end
 *     state and the history, through mrhip_filt_device_rates and mrhip_filt_device_rates_ragged, including the short-input path, the
 *     zero-start seam on every call and a channel of ragged length 0.  STRICT only.  Arithmetic: that of "FIRFarrow with complex taps"
 *     on bank c -- Horner in Float64 per component, never fused; one rounding to the tap's scalar, widened exactly to R; the dot oldest
 *     sample first, every multiply, add and subtract rounded separately;
 *   - tap queries: mrhip_get_pnfb and mrhip_farrow_tapsforphase answer in the layout of "Per-channel complex taps for FIRFarrow" --
 *     nchannels banks or rows one after the other;
 *   - going back: mrhip_set_channel_taps_farrow, mrhip_set_channel_pnfb and mrhip_set_channel_pnfb_device on a filter that holds
 *     complex banks answer MRHIP_ERR_UNSUPPORTED, "going back to real taps is left out" (no filter could be in that state before);
 *   - kernels: farrow_rates_ctaps_generic (any shape) and farrow_rates_ctaps_multi (four outputs a lane share each tap's scalar
 *     coefficient loads, a tile is one channel and so one bank; MRHIP_FARROW_RATES_CTAPS_MULTI = 1 selects it for every call, 0 never,
 *     the default rule follows the measured rows: from 90 112 tiles, up to 22 tiles a channel); MRHIP_FARROW_RATES_CTAPS_GRID replaces
 *     its grid; MRHIP_FORCE_GENERIC = 1 keeps the universal one;
 *   - a filter on which none of the three was called runs the launches, kernels and messages it always ran: mrhip_set_channel_ctaps
 *     keeps answering a FIRFarrow filter as quoted above, mrhip_set_channel_taps_farrow and the constructors keep answering a complex
 *     tap dtype with MRHIP_ERR_UNSUPPORTED;
 *   - left out on purpose: the FIRFarrow fit on the device; one shared complex bank without a bank per channel (install the same bank
 *     nchannels times); going back to real taps; a FUSED form; lengths on the device; graph capture, rings, cascades and sharding;
 *     the parallel schedule for long channels.  (Since added: the FIRFarrow fit on the device, mrhip_set_channel_ctaps_farrow_device
 *     below.) */
int mrhip_set_channel_ctaps_farrow(mrhip_filter *f, const void *h /* [nchannels][hLen] (re, im) */, int64_t hLen, int tap_dtype);
int mrhip_set_channel_pnfb_ctaps(mrhip_filter *f, const double *pnfb /* [nchannels][tapsPerPhi][polyorder+1] (re, im) Float64 */, int64_t tapsPerPhi,
                                 int64_t polyorder);
int mrhip_set_channel_pnfb_ctaps_device(mrhip_filter *f, const double *pnfb /* DEVICE, same layout */, int64_t tapsPerPhi, int64_t polyorder,
                                        void *stream);
/* The FIRFarrow fit on the device for the filters with per-channel rates (mrhip_set_channel_taps_farrow_device and
 * mrhip_set_channel_ctaps_farrow_device on a filter of mrhip_create_farrow_rates*).  A block-LMS equaliser or a matched-pulse tracker
 * produces TAPS, not fitted polynomial banks; mrhip_set_channel_taps_farrow and mrhip_set_channel_ctaps_farrow take them from HOST memory,
 * wait for the filter's stream and fit every row on the host, which costs many chunks' worth of time.  The two calls below take the taps
 * from DEVICE memory and fit them there, in stream order: the cell the sections above list as left out ("the FIRFarrow fit on the
 * device").  They are CALLS on an existing filter, the twins of mrhip_set_channel_taps_farrow and mrhip_set_channel_ctaps_farrow, not
 * constructors: there are still sixteen constructors and the ABI version stays 1.
 *   - layouts and checks: mrhip_set_channel_taps_farrow_device takes the layout and the argument checks of mrhip_set_channel_taps_farrow
 *     (h: nchannels rows of hLen taps in the filter's tap dtype), mrhip_set_channel_ctaps_farrow_device those of
 *     mrhip_set_channel_ctaps_farrow (rows of (re, im) pairs in the complex type of the filter's tap precision; a FUSED filter is
 *     MRHIP_ERR_UNSUPPORTED), in the same order, each message naming the new function.  A filter of mrhip_create_arbitrary_rates is
 *     MRHIP_ERR_INVALID_ARG with a message that points to mrhip_set_channel_taps_device (mrhip_set_channel_ctaps_device); any other
 *     filter is MRHIP_ERR_INVALID_ARG.  The real call on a filter that holds complex banks is MRHIP_ERR_UNSUPPORTED, "going back to real
 *     taps is left out";
 *   - Nphi: a lane keeps its row of Nphi taps in LDS, so the calls serve Nphi up to 1024; a larger Nphi is MRHIP_ERR_UNSUPPORTED with a
 *     message that states the bound and points to the host call;
 *   - rank: whether the fit is rank deficient depends on (Nphi, polyorder) alone -- polyorder + 1 > Nphi, possible on a filter of
 *     mrhip_create_farrow_rates_pnfb -- and is decided on the host: MRHIP_ERR_INVALID_ARG, "polynomial fit is rank deficient";
 *   - stream: the rules of mrhip_set_channel_pnfb_device (mrhip_set_channel_pnfb_ctaps_device).  The call adopts `stream` and takes
 *     effect behind the calls already enqueued and ahead of every later one; h is read in stream order.  A capturing stream is
 *     MRHIP_ERR_UNSUPPORTED.  Every refusal comes before anything is enqueued or changed;
 *   - the fit: mrhip_polyfit's, a Householder QR of the Vandermonde matrix A[r][p] = (r+1)^p.  A is the same for every row of every
 *     channel, so its side of the factorisation -- the reflectors, their squared norms and the triangle R, (polyorder+1) * (Nphi +
 *     polyorder + 2) Float64 -- is computed once per filter on the host by the same statements, at the first of these calls, uploaded
 *     then and freed by mrhip_destroy.  One kernel (rates_farrow_fit_kernel, a lane per channel, row and component) applies the
 *     reflections to the row h_c[(tapsPerPhi-1-i)*Nphi + phi], phi = 0 ... Nphi-1 (0 past hLen), widened exactly to Float64, back-
 *     substitutes, and writes the polyorder+1 coefficients into the filter's bank, rounded to Float32 and widened back per component on a
 *     filter with Float32 taps.  Same order of operations, every multiply, add and subtract rounded on its own, IEEE Float64 division:
 *     the banks are BIT FOR BIT those of mrhip_set_channel_taps_farrow (mrhip_set_channel_ctaps_farrow) given the same matrix;
 *   - effect: from the next call on the filter is bit for bit the filter after the host call with the same matrix -- banks, outputs,
 *     counts, states and history, under STRICT and (real taps) FUSED, through mrhip_filt_device_rates, the ragged call, the
 *     device-lengths call and the chained call, on the universal and the multi kernels.  mrhip_set_channel_ctaps_farrow_device on a
 *     filter over real samples makes it write complex outputs from then on, as mrhip_set_channel_pnfb_ctaps_device does;
 *   - allocation and waits: a filter whose bank is still shared (for the complex call: that holds no complex banks yet) allocates the
 *     nchannels banks first, then waits ONCE for the filter's stream, and the bank it held is freed right after that wait; the first of
 *     these calls on a filter uploads the QR table during the same wait (a filter that already holds its banks waits for the table
 *     alone).  Every later call enqueues one kernel and returns without waiting.  A failed allocation leaves the filter bit for bit as
 *     it was;
 *   - host copies: afterwards the host copy is stale; mrhip_get_pnfb and mrhip_farrow_tapsforphase wait for the filter's stream and read
 *     the banks back.  mrhip_reset keeps the banks.  Host and device installs mix freely;
 *   - existing calls answer as before: mrhip_set_channel_taps_device on a FIRFarrow filter keeps its MRHIP_ERR_UNSUPPORTED and its
 *     message; a filter on which neither function was called runs the launches and kernels it always ran;
 *   - left out on purpose: the fit in the constructors and on the one-rate FIRFarrow filters; a faster host fit (mrhip_polyfit factors
 *     per row and stays the yardstick); graph capture; one shared complex bank; a FUSED form for complex taps; the parallel schedule
 *     for long channels. */
int mrhip_set_channel_taps_farrow_device(mrhip_filter *f, const void *h /* DEVICE, [nchannels][hLen] */, int64_t hLen, int tap_dtype, void *stream);
int mrhip_set_channel_ctaps_farrow_device(mrhip_filter *f, const void *h /* DEVICE, [nchannels][hLen] (re, im) */, int64_t hLen, int tap_dtype,
                                          void *stream);
/* Input lengths from device memory, and chaining, for the filters with per-channel rates (mrhip_create_arbitrary_rates,
 * mrhip_create_farrow_rates*, with shared, per-channel or complex per-channel taps).  Rates, taps and polynomial banks arrive from device
 * memory in stream order (above); the input LENGTHS of mrhip_filt_device_rates_ragged are a HOST array, so a length computed on the GPU
 * -- a burst detector's count, a jitter buffer's fill level, the output counts of an earlier filter -- had to travel to the host and be
 * waited for.  The two calls below fill the filter's device array of lengths by a kernel (rates_lens_set_kernel, one lane per channel)
 * in the place of the copy from the host; everything behind it is the ragged call.  They remove the last host round trip from the loop
 * of filter call, tracker, update, filter call.  No new constructor; the ABI version stays 1.
 *   - mrhip_filt_device_rates_lens_device is mrhip_filt_device_rates_ragged with x_lens in DEVICE memory, read in stream order: the
 *     array must hold its values by the time `stream` reaches the call and may be overwritten by work enqueued on `stream` afterwards.
 *     The host cannot see the values, so the caller declares their maximum, x_len_max, which takes the place of "the largest of
 *     x_lens" in every check of the ragged call -- fewer than 2^31-1 samples, x_stride >= x_len_max for nchannels > 1, the bound
 *     mrhip_outputlength_bound(f, x_len_max) <= 2^24, y_capacity and y_stride at least that bound -- and in the sizing of the launch
 *     and of the tiled kernels' plans;
 *   - on the device channel c reads l = x_lens[c]; 0 <= l <= x_len_max: the channel is fed x_c[0 : l).  Any other value -- negative,
 *     above the declared maximum -- feeds the channel NOTHING in this call, which is the ragged call's length 0: state and history are
 *     kept, the count is 0, and the channel's record receives a sticky "length refused" mark.  A refused value never reaches the walk,
 *     the history fold or a filter kernel;
 *   - after the import the call is the ragged call: the same launches, the same kernel names from mrhip_last_kernel_name, the same
 *     timing bracket (the import kernel runs in front of it).  Parity: channel c is bit for bit the one-channel filter fed
 *     x_c[0 : l_c) -- outputs, count, end state, history -- under STRICT and FUSED, for both families, for shared, per-channel and
 *     complex per-channel taps.  The call mixes freely with mrhip_filt_device_rates and mrhip_filt_device_rates_ragged on one filter;
 *   - host waits: only where mrhip_filt_device_rates waits (growth of the schedule buffers).  No pinned staging slot is used;
 *   - reporting: mrhip_get_channel_states returns MRHIP_ERR_INVALID_ARG while a record holds the mark ("a device-resident LENGTH was
 *     refused ... the channel was fed nothing"; the states are filled in all the same).  An overrun and a refused rate keep their
 *     answers and go first, in that order.  mrhip_set_channel_states and mrhip_reset clear the mark as they clear the others;
 *   - refused before anything is enqueued or any state moves, each with a message that names the function: a NULL f or x_lens, a filter
 *     without per-channel rates, a negative x_len_max or y_capacity, x NULL with x_len_max above 0, x_stride below x_len_max for
 *     nchannels > 1 (all MRHIP_ERR_INVALID_ARG); x_len_max of 2^31-1 or more, a capturing stream, a bound above 2^24
 *     (MRHIP_ERR_UNSUPPORTED); capacity or stride below the bound (MRHIP_ERR_BUFFER_TOO_SMALL);
 *   - mrhip_filt_device_rates_chained: f has per-channel rates; its input x is what prev's latest call wrote, earlier on the same
 *     stream, and its lengths are that call's counts, taken on the device.
 *       prev with per-channel rates: the same nchannels and device; the length of channel c is the `count` of prev's record c.  The
 *       records hold the counts of prev's LATEST call: the chained call must be enqueued between that call of prev and prev's next one
 *       on the stream.  A prev that has not been called since its creation or mrhip_reset is refused.
 *       prev a one-state filter: the same nchannels, and its latest call was planned on the device (mrhip_filt_device_async, a call
 *       under capture: the condition of mrhip_filt_device_chained); every channel is fed that call's one count.
 *     x_len_bound = mrhip_outputlength_bound(prev, prev's (largest) input length) plays x_len_max's part in every check above,
 *     including the refusal on the device of a count above it.  Refused on the host, ahead of any launch and in this function's name
 *     (MRHIP_ERR_INVALID_ARG): prev == f, different channel counts or devices, f's sample dtype other than prev's output dtype, the two
 *     cases of prev above; then the refusals of mrhip_filt_device_rates_lens_device.  Parity: channel c of f is bit for bit the
 *     one-channel filter fed the outputs of prev's channel c, call after call; prev is not touched.  mrhip_filt_device_chained and
 *     mrhip_cascade_create keep refusing filters with per-channel rates;
 *   - left out on purpose: graph capture of these filters; compacting the tiles of channels that end early; a one-state filter
 *     BEHIND a filter with per-channel rates (one length against many counts); mrhip_cascade_*, rings and sharding; the parallel
 *     schedule for long channels. */
int mrhip_filt_device_rates_lens_device(mrhip_filter *f, const void *x, const int64_t *x_lens /* DEVICE, [nchannels] */, int64_t x_len_max,
                                        int64_t x_stride, void *y, int64_t y_capacity, int64_t y_stride, int64_t *counts_out, void *stream);
int mrhip_filt_device_rates_chained(mrhip_filter *f, const mrhip_filter *prev, const void *x, int64_t x_len_bound, int64_t x_stride,
                                    void *y, int64_t y_capacity, int64_t y_stride, int64_t *counts_out, void *stream);
/* wait for everything the filter has enqueued (after a HIP-graph capture of one of its calls: for the device -- replays run
 * on streams the library never saw) and take the device-resident stream state over into the host object;
 * *last_n_written (optional) receives the per-channel count of the last call.  Returns the status of a device-planned call
 * that failed since the last mrhip_sync_state, once.  A device-wide wait invalidates a HIP-graph capture that is going on on
 * another stream: while a stream the library has been called on is still capturing, the wait of a filter whose calls were captured
 * once -- here and in every entry point that needs the host-side state (mrhip_next_output_count, mrhip_outputlength,
 * mrhip_get_state, a synchronous mrhip_filt_*) -- is refused with MRHIP_ERR_UNSUPPORTED (-1 from the counting functions). */
int mrhip_sync_state(mrhip_filter *f, int64_t *last_n_written);
/* Streaming helper: exactly the sequence of filt!(buffer, self, x[a:a+chunk]) calls a caller would make
 * over consecutive `chunk`-sample pieces of a device-resident signal, issued back to back by the library (one host
 * call instead of x_len/chunk).  Output k of piece i lands right after the outputs of piece i-1 in y; *n_written is the
 * total per channel.  State and history are carried from piece to piece on the device, bit-identical to the caller's own loop.
 * Like that loop, an error (e.g. MRHIP_ERR_BUFFER_TOO_SMALL for a later piece) leaves the pieces already issued applied:
 * *n_written then holds the outputs produced so far and the filter stands at the start of the failing piece. */
int mrhip_filt_device_chunked(mrhip_filter *f, const void *x, int64_t x_len, int64_t x_stride, int64_t chunk, void *y,
                              int64_t y_capacity, int64_t y_stride, int64_t *n_written, void *stream);
/* same contract with HOST pointers: copies x in, runs mrhip_filt_device, copies y out,
 * synchronises.  Replaces filt!(buffer, self, x) for a caller whose data lives in host memory. */
int mrhip_filt_host(mrhip_filter *f, const void *x, int64_t x_len, int64_t x_stride, void *y,
                    int64_t y_capacity, int64_t y_stride, int64_t *n_written);
/* block until everything enqueued on the filter's behalf on `stream` has finished */
int mrhip_synchronize(mrhip_filter *f, void *stream);

/* ---- cascades (the reference chains filt calls by hand) ------------------------ */
/* A chain of filters run back to back on one stream: y = filt(stage[n-1], ... filt(stage[0], x)).  The stages are
 * ordinary stateful filters (borrowed, not owned: destroy them after the cascade); stage i+1's sample dtype must be
 * stage i's output dtype, all stages share nchannels and the device.  Intermediate signals live in device buffers
 * owned by the cascade and never leave HBM; every count is closed-form on the host, so nothing is read back between
 * stages and chunked calls continue the stream exactly like calling the stages by hand. */
typedef struct mrhip_cascade mrhip_cascade;
int mrhip_cascade_create(mrhip_filter *const *stages, int nstages, mrhip_cascade **out);
void mrhip_cascade_destroy(mrhip_cascade *c);
/* outputlength of the chain (each stage's outputlength applied in turn: an estimate where a stage's is, :375) */
int64_t mrhip_cascade_outputlength(const mrhip_cascade *c, int64_t inputlength);
/* exact per-channel output count of the next mrhip_cascade_filt_device call with `inputlength` samples */
int64_t mrhip_cascade_next_output_count(const mrhip_cascade *c, int64_t inputlength);
/* same contract as mrhip_filt_device for the whole chain; MRHIP_ERR_BUFFER_TOO_SMALL leaves every stage untouched.
 * Under HIP-graph capture the lengths planned at capture time are what every replay runs with (a stage's input length is part
 * of the next stage's launch), so every stage must map its input length to the same count on every replay: rational-family
 * stages with inputlength * L a multiple of M; anything else (and FIRArbitrary / FIRFarrow stages) is MRHIP_ERR_UNSUPPORTED
 * before anything is launched.  y needs room for mrhip_outputlength_bound of the last stage, and one plain call of the same
 * size must have run before the capture (it allocates the buffers between the stages). */
int mrhip_cascade_filt_device(mrhip_cascade *c, const void *x, int64_t x_len, int64_t x_stride, void *y, int64_t y_capacity,
                              int64_t y_stride, int64_t *n_written, void *stream);
/* The chain with nothing returned to the host (asynchronous, or under HIP-graph capture at ANY chunk size): the first stage is
 * mrhip_filt_device_async, every later one mrhip_filt_device_chained on the previous stage's count.  y needs room for the
 * last stage's bound of the bounds; *count_out (device-accessible, may be NULL) receives the chain's per-channel output
 * count.  One plain call of the same size must have run before a capture (it allocates the buffers between the stages);
 * every kind of stage in every position. */
int mrhip_cascade_filt_device_async(mrhip_cascade *c, const void *x, int64_t x_len, int64_t x_stride, void *y, int64_t y_capacity,
                                    int64_t y_stride, int64_t *count_out, void *stream);
int mrhip_cascade_reset(mrhip_cascade *c);

/* ---- a ring of arriving chunks: ONE resident kernel instead of a launch per chunk ------------------------------ */
/* replaces the reference's streaming usage -- a loop of  y_i = filt(self, x_i)  over the chunks of a signal as they arrive, on one
 * stateful FIRFilter (README.md:87-141; the state carried from call to call: src/Filters.jl:571-572, history: support.jl:61-80).
 * mrhip_ring_open starts a kernel that stays resident on the filter's device and consumes chunk descriptors; mrhip_ring_push is
 * filt!(y, self, x) for the next chunk: it plans the call on the host (the state recurrence in closed form, so *n_written -- the
 * Int the reference's filt! returns -- is valid on return), writes one descriptor into pinned memory and returns; the kernel
 * filters the chunk beside the chunks before it (several are in flight at once, the history travels between them on the
 * device) and raises a flag in pinned memory when its outputs are complete: mrhip_ring_wait / mrhip_ring_drain.  Results, counts,
 * end state and history are bit for bit those of the same calls made through mrhip_filt_device.
 *   - x must be COMPLETE in device memory when it is pushed (the resident kernel is not ordered behind any stream: synchronise
 *     the producer of x first) and x and y must stay untouched until the chunk's flag is up;
 *   - at most 63 chunks are in flight; a push into a full ring waits for the oldest;
 *   - while a ring is open the filter's other entry points (filt, reset, set_state, ...) return MRHIP_ERR_INVALID_ARG, and no call
 *     that waits for the whole DEVICE (hipDeviceSynchronize, hipFree, ...) returns before mrhip_ring_close: the kernel leaves
 *     only when the ring is closed, or by itself after MRHIP_RING_IDLE_MS (default 2000) without a push -- the next push then
 *     starts a new one;
 *   - FIRRational / FIRInterpolator with 24 or 32 taps per phase and M < 2L (the BASELINE shapes; STRICT numerics) run on the
 *     resident kernel; every other filter takes the same interface as stream-ordered launches, one per chunk, on the ring's
 *     stream (mrhip_ring_info tells which);
 *   - a chunk is "complete" when a later kernel on any stream of the device, or a copy, reads its outputs: small chunks are stored
 *     write-through, chunks of at least MRHIP_RING_FLUSH_MIN_MB (32) of outputs plainly with one L2 write-back per XCD in front of the flag;
 *   - the resident kernel's launch is checked: if not all of its workgroups are on the chip within 3 ms (the dealing of the work needs
 *     every one of them) it is launched again with as many as were. */
typedef struct mrhip_ring mrhip_ring;
int mrhip_ring_open(mrhip_filter *f, mrhip_ring **out);
/* filt!(y, self, x) for the next arriving chunk (same argument meaning and errors as mrhip_filt_device); *seq (optional)
 * receives the chunk's number for mrhip_ring_wait */
int mrhip_ring_push(mrhip_ring *r, const void *x, int64_t x_len, int64_t x_stride, void *y, int64_t y_capacity, int64_t y_stride,
                    int64_t *n_written, uint64_t *seq);
/* the library's chunk loop over a device-resident signal (mrhip_filt_device_chunked's contract): one mrhip_ring_push per `chunk`
 * samples, outputs back to back in y; *n_written the total, *last_seq the last chunk's number */
int mrhip_ring_push_chunks(mrhip_ring *r, const void *x, int64_t x_len, int64_t x_stride, int64_t chunk, void *y, int64_t y_capacity,
                           int64_t y_stride, int64_t *n_written, uint64_t *last_seq);
/* block until chunk `seq` is complete (its outputs are in device memory); chunks may complete out of order */
int mrhip_ring_wait(mrhip_ring *r, uint64_t seq);
/* block until every pushed chunk is complete */
int mrhip_ring_drain(mrhip_ring *r);
/* drain, end the resident kernel, hand the stream (state behind the last chunk, history, device record) back to the filter,
 * free the ring.  (A filter destroyed while it still feeds a ring -- finalizers run in any order -- shuts the ring down itself;
 * the ring's entry points then fail and mrhip_ring_close only frees the handle.) */
int mrhip_ring_close(mrhip_ring *r);
/* info[0..n): [0] 1 = resident kernel, 0 = one launch per chunk; [1] ring depth; [2] chunks pushed; [3] kernels restarted after an
 * idle deadline; [4] steps per grab; [5] outputs per step; [6] launches repeated with fewer workgroups (not all started in time: a
 * co-tenant kernel held part of the chip); [7] workgroups of the resident kernel (0: as many as the chip holds); [8] XCDs of the
 * device (other than 8: every chunk completes by write-through stores) */
int mrhip_ring_info(const mrhip_ring *r, int64_t *info, int n);

/* ---- one FIRFilter whose channels are split over several GPUs (BASELINE.json config 5) ------------------------ */
/* replaces filt(self, x) (src/Filters.jl:577-587 and its siblings :475,519,633,744,841) for a multi-channel signal -- in the
 * reference: one FIRFilter per channel, nothing shared but the read-only taps -- split by CHANNEL over `ndevices` GPUs of one
 * process: shard i is an ordinary filter on devices[i] with channels [start_i, start_i + count_i) (contiguous; the first
 * nchannels % ndevices shards take one channel more), a stream of its own, and no exchange with the others during compute.  The
 * only traffic between devices is the final gather of the outputs (mrhip_sharded_gather: peer copies over xGMI on the shards'
 * streams).  The same device may be named more than once (two shards on one GPU).
 * ctor selects the reference constructor: 0 = FIRFilter(h, num//den) (:158), 1 = FIRFilter(h, rate, Nphi) (:183),
 * 2 = FIRFilter(h, rate, Nphi, polyorder) (:192); arguments a constructor does not take are ignored. */
typedef struct mrhip_sharded mrhip_sharded;
int mrhip_sharded_create(int ctor, const void *h, int64_t hLen, int tap_dtype, int64_t num, int64_t den, double rate, int64_t Nphi,
                         int64_t polyorder, int sample_dtype, int64_t nchannels, const int *devices, int ndevices, mrhip_sharded **out);
void mrhip_sharded_destroy(mrhip_sharded *s);
int mrhip_sharded_nshards(const mrhip_sharded *s);
/* shard i: first channel, channel count, device, and the shard's filter itself (borrowed: state, history, timing ... through the
 * ordinary entry points; NULL for a shard without channels); any of the four may be NULL */
int mrhip_sharded_shard(const mrhip_sharded *s, int i, int64_t *start, int64_t *count, int *device, mrhip_filter **filter);
/* outputlength / the exact count of the next call (the state machine is data independent: every shard agrees) / reset */
int64_t mrhip_sharded_outputlength(const mrhip_sharded *s, int64_t inputlength);
int64_t mrhip_sharded_next_output_count(const mrhip_sharded *s, int64_t inputlength);
int mrhip_sharded_reset(mrhip_sharded *s);
/* filt!(buffer, self, x) with device-resident data: x[i] / y[i] are device pointers ON SHARD i's DEVICE holding its count_i channels
 * (channel c at + c * stride[i]; NULL strides: x_len / y_capacity); same contract as mrhip_filt_device per shard, each on the
 * shard's own stream (asynchronous: mrhip_sharded_synchronize waits for all); *n_written = the per-channel count. */
int mrhip_sharded_filt_device(mrhip_sharded *s, const void *const *x, int64_t x_len, const int64_t *x_stride, void *const *y, int64_t y_capacity,
                              const int64_t *y_stride, int64_t *n_written);
/* filt!(buffer, self, X) for a HOST matrix with one channel per column (Julia's layout; x_stride / y_stride in samples): the columns
 * are split over the shards, one host thread per shard runs its copies and kernels (mrhip_filt_host), all devices at once; blocks
 * until y holds every channel's outputs.  What the Julia shim's filt(::ShardedFIRFilter, X::Matrix) calls. */
int mrhip_sharded_filt_host(mrhip_sharded *s, const void *x, int64_t x_len, int64_t x_stride, void *y, int64_t y_capacity, int64_t y_stride,
                            int64_t *n_written);
/* the final gather: rows [start_i, start_i + count_i) of a (nchannels x n_out) result at `dst` on `dst_device` (row stride dst_stride
 * samples) from y[i] on shard i's device, asynchronous on the shards' streams behind their filter kernels */
int mrhip_sharded_gather(mrhip_sharded *s, const void *const *y, int64_t n_out, const int64_t *y_stride, void *dst, int64_t dst_stride, int dst_device);
/* ordering against a CALLER's stream on shard i's device (the shards run on private streams): _wait_stream puts the shard's stream
 * behind what `stream` holds so far (inputs the caller's kernels still write, buffers its allocator handed out in stream order),
 * _signal_stream puts `stream` behind what the shard's stream holds so far (the caller's later kernels see the outputs).  No
 * reference counterpart: the reference is synchronous (src/Filters.jl:577-587). */
int mrhip_sharded_wait_stream(mrhip_sharded *s, int shard, void *stream);
int mrhip_sharded_signal_stream(mrhip_sharded *s, int shard, void *stream);
int mrhip_sharded_synchronize(mrhip_sharded *s);

/* replaces the stateless filt(h, x, ratio), src/Filters.jl:858-861, and
 * filt(h, x, rate, Nphi), :864-867, for host data, one channel: construct, filter once,
 * destroy.  rate <= 0 selects the rational form with num//den; rate > 0 the arbitrary form. */
int mrhip_filt_once(const void *h, int64_t hLen, int tap_dtype, int64_t num, int64_t den, double rate,
                    int64_t Nphi, const void *x, int64_t x_len, int sample_dtype, void *y,
                    int64_t y_capacity, int64_t *n_written, int device);

/* ---- measurement ---------------------------------------------------------------------- */
/* With timing enabled every compute-kernel launch made by mrhip_filt_device on this filter is
 * bracketed by a pair of HIP events recorded on the launch stream (the history-shift kernel and
 * the copies are outside the bracket).  Nothing synchronises until mrhip_timing_read, which waits
 * for the recorded events, returns how many launches were bracketed since the last read and the sum
 * of their durations in milliseconds, and clears the log.  bench.py uses it for roofline.achieved.
 * enabled = n > 1 brackets every n-th compute launch only (the two event records cost a few microseconds of
 * stream time per launch, which a throughput measurement of back-to-back launches would otherwise include).
 * enabled = -n < -1 puts ONE bracket around every n consecutive compute launches: mrhip_timing_read then returns the
 * launches covered by complete groups and the groups' total duration, gaps between the launches included. */
int mrhip_set_timing(mrhip_filter *f, int enabled);
int mrhip_timing_read(mrhip_filter *f, int64_t *n_launches, double *total_ms);
/* name of the device kernel the last filt call dispatched (for profiles / logs).  The two filter kernels of a filter with
 * per-channel rates are reported as arb_rates_generic and arb_rates_tiled, without the suffix the other names carry: the table of
 * write-only-own-outputs cases (tests/output_bounds_cases.py) is keyed by the suffixed names in the sources, and these two kernels'
 * cases live in tests/test_gpu_rates_arb.py until they move into that table.  The same holds for farrow_rates_generic and
 * farrow_rates_multi (FIRFarrow with per-channel rates; their cases: tests/test_gpu_rates_farrow.py), and for arb_rates_bank_generic
 * and arb_rates_bank_tiled (per-channel taps with per-channel rates; their cases: tests/test_gpu_rates_bank_arb.py), and for
 * farrow_rates_bank_generic and farrow_rates_bank_multi (the same for FIRFarrow; their cases: tests/test_gpu_rates_bank_farrow.py), and
 * for arb_rates_ctaps_generic and arb_rates_ctaps_tiled (complex per-channel taps with per-channel rates; their cases:
 * tests/test_gpu_rates_arb_ctaps.py), and for farrow_rates_ctaps_generic and farrow_rates_ctaps_multi (the same for FIRFarrow; their
 * cases: tests/test_gpu_rates_farrow_ctaps.py). */
const char *mrhip_last_kernel_name(const mrhip_filter *f);
/* How the phase schedule of a FIRArbitrary / FIRFarrow filter -- update(), src/Filters.jl:663-673 and :780-792 -- has
 * been evaluated so far.  info[0..n) receives, as far as n reaches:
 *   [0] 1 if the device evaluation covers this (rate, Nphi), else 0 (the host's serial loop runs)
 *   [1] candidate values per congruence class G/Umin   [2] candidates per segment
 *   [3] period of the accumulator's cycle, 0 if none was found (a cycle makes the schedule a closed form)
 *   [4] outputs scheduled by the host loop             [5] outputs scheduled by the closed form of a cycle
 *   [6] pieces scheduled and verified on the device    [7] pieces whose verification failed (redone by the host loop)
 *   [8] calls that reused the schedule of an identical earlier call (same accumulator, inputDeficit and length)
 * (diagnostics and tests; results never depend on the path taken) */
int mrhip_schedule_info(const mrhip_filter *f, int64_t *info, int n);

#ifdef __cplusplus
}
#endif
#endif /* MULTIRATE_HIP_H */
