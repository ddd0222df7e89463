// create.hip -- the sixteen mrhip_create_* constructors of include/multirate_hip.h.
//
// An entry point is a value (CreateEntry, create.h: family, tap class, bank / rates / pnfb, its name and the hint of its refusal) and one
// call of create_filter.  Everything there that makes no HIP call -- the argument checks in front of the device query, the parameter
// checks behind it, the banks -- is host_logic.cpp's (create_check_args, create_check_params, create_pfb_banks, create_farrow_banks);
// this unit keeps the device work: the device checks, the guard, the uploads, the common allocations, the per-channel records.
#include <algorithm>
#include <cstdlib>

#include "mrhip_filter.h"
#include "create.h"
#include "rates_arb.h"

using namespace mrhip;

namespace {

int check_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MRHIP_ERR_NO_DEVICE, "no HIP device visible; libmultirate_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(MRHIP_ERR_INVALID_ARG, "device ordinal out of range");
    if (!device_is_gfx950(device))
        return fail(MRHIP_ERR_NO_DEVICE, "device is not gfx950 (MI355X); kernels are built for gfx950 only");
    return MRHIP_OK;
}

size_t r_size(const mrhip_filter *f) { return f->r_f64 ? 8 : 4; }

// upload taps (tap dtype on the host) as R-typed device array; f32 -> f64 widening is exact and is
// what Julia's promotion does on every multiply (Real*Real / Real*Complex methods).  Complex taps are
// interleaved (re, im) pairs: the same array of scalars, widened the same way.
// The vector sits between two runs of kTapPad zero elements: fir_stream_rt_kernel reads whole blocks of taps around the
// ends of a window (it discards what the out-of-window ones produce) without a clamp per tap.
int upload_taps(mrhip_filter *f, const std::vector<unsigned char> &src, void **dptr, void **alloc)
{
    const size_t n = src.size() / dtype_scalar_size(f->th);
    const size_t pad = static_cast<size_t>(mrhip::kTapPad) * r_size(f);
    const size_t bytes = std::max<size_t>(n * r_size(f), 16) + 2 * pad;
    MRHIP_CHECK_HIP(hipMalloc(alloc, bytes));
    MRHIP_CHECK_HIP(hipMemset(*alloc, 0, bytes));
    *dptr = static_cast<unsigned char *>(*alloc) + pad;
    if (f->r_f64 && !dtype_is_f64(f->th)) {
        std::vector<double> w(n);
        const float *s = reinterpret_cast<const float *>(src.data());
        for (size_t i = 0; i < n; ++i) w[i] = static_cast<double>(s[i]);
        MRHIP_CHECK_HIP(hipMemcpy(*dptr, w.data(), n * 8, hipMemcpyHostToDevice));
    } else {
        MRHIP_CHECK_HIP(hipMemcpy(*dptr, src.data(), src.size(), hipMemcpyHostToDevice));
    }
    return MRHIP_OK;
}

// FIRFarrow: the polynomial bank(s), [T][polyorder+1] coefficients in ascending powers -- scalars for real taps, (re, im) pairs for complex
// ones; a bank per channel one after the other with per-channel taps.  The same bank degree-major, padded to 32 taps with zeros, is what
// farrow_wave_kernel reads: built only where that kernel can run (real taps, T <= 32, one bank, one rate).
int upload_pnfb(mrhip_filter *f)
{
    if (hipMalloc(reinterpret_cast<void **>(&f->d_pnfb), f->h_pnfb.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(f->d_pnfb, f->h_pnfb.data(), f->h_pnfb.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MRHIP_ERR_HIP, "uploading the polynomial filter bank failed");
    if (f->T > 32 || dtype_is_complex(f->th) || f->bank || f->rates) return MRHIP_OK;
    const int64_t P = f->polyorder;
    std::vector<double> t(static_cast<size_t>(P + 1) * 32, 0.0);
    for (int64_t i = 0; i < f->T; ++i)
        for (int64_t j = 0; j <= P; ++j) t[static_cast<size_t>(j) * 32 + i] = f->h_pnfb[static_cast<size_t>(i) * (P + 1) + j];
    if (hipMalloc(reinterpret_cast<void **>(&f->d_pnfb_t), t.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(f->d_pnfb_t, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(MRHIP_ERR_HIP, "uploading the polynomial filter bank failed");
    return MRHIP_OK;
}

int alloc_common(mrhip_filter *f)
{
    const size_t hbytes = std::max<size_t>(static_cast<size_t>(f->nch) * f->H * dtype_size(f->tx), 16);
    // Every later launch goes to a non-blocking stream, which the null stream's memsets are not ordered with: zero
    // on the filter's own stream and wait for it here (construction may block; nothing else in the library does).
    MRHIP_CHECK_HIP(hipStreamCreateWithFlags(&f->own_stream, hipStreamNonBlocking));
    for (int i = 0; i < 3; ++i) {
        MRHIP_CHECK_HIP(hipMalloc(&f->d_hist[i], hbytes));
        MRHIP_CHECK_HIP(hipMemsetAsync(f->d_hist[i], 0, hbytes, f->own_stream));   // history = zeros(historyLen), Filters.jl:177
    }
    MRHIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(&f->d_counters), mrhip::kCounterBytes));
    MRHIP_CHECK_HIP(hipMemsetAsync(f->d_counters, 0, mrhip::kCounterBytes, f->own_stream));
    MRHIP_CHECK_HIP(hipStreamSynchronize(f->own_stream));
    {
        hipDeviceProp_t prop;
        MRHIP_CHECK_HIP(hipGetDeviceProperties(&prop, f->device));
        f->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        const char *fg = std::getenv("MRHIP_FORCE_GENERIC");
        f->force_generic = fg && fg[0] == '1';
    }
    MRHIP_CHECK_HIP(hipEventCreateWithFlags(&f->sched_copied, hipEventDisableTiming));
    MRHIP_CHECK_HIP(hipEventCreateWithFlags(&f->xs_event, hipEventDisableTiming));
    return rec_alloc(f);              // the stream state on the device (stream_state.hip), constructor state
}

// Per-channel rates: the channels share the banks; each has a record on the device (RateChannel, rates_arb.h) in its constructor state
// (Filters.jl:110-115, :141-144: the state rates_reset_kernel writes).
int rates_alloc(mrhip_filter *f)
{
    std::vector<RateChannel> v(static_cast<size_t>(f->nch));
    for (int64_t c = 0; c < f->nch; ++c) {
        RateChannel &r = v[static_cast<size_t>(c)];
        r = RateChannel{};
        r.rate = f->h_rates[static_cast<size_t>(c)];
        r.delta = static_cast<double>(f->Nphi) / r.rate;           // Δ = N𝜙/rate, Filters.jl:113
        r.acc = 1.0; r.inputDeficit = 1; r.xIdx = 1;
    }
    MRHIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(&f->d_rrec), v.size() * sizeof(RateChannel)));
    MRHIP_CHECK_HIP(hipMemcpy(f->d_rrec, v.data(), v.size() * sizeof(RateChannel), hipMemcpyHostToDevice));
    return MRHIP_OK;
}

// The one path of every constructor.  FIRFilter(h, ratio), src/Filters.jl:158-180; FIRArbitrary(h, rate, N𝜙), :105-117; FIRFarrow(h, rate,
// N𝜙, polyorder), :138-147.  The banks are held in the tap type on the host and upload_taps widens them exactly to R (complex taps: as
// the interleaved (re, im) scalars they are); FIRFarrow's coefficients are Float64 that hold values of the tap type.  e.bank: `h` holds
// nch rows and the device nch banks one after the other, [nch][Nphi][T] or [nch][T][polyorder+1].  e.rates: nch rates behind the one
// bank; the filter's `rate` is the largest of them.  e.pnfb: `h` is the caller's polynomial bank.
int create_filter(const CreateEntry &e, const void *h, int64_t hLen, int th, CreateParams p, int tx, int64_t nch, int device, mrhip_filter **out)
{
    if (Refusal r = create_check_args(e, h, hLen, th, tx, nch, out)) return fail(r.status, r.message);
    if (int rc = check_device(device)) return rc;
    if (Refusal r = create_check_params(e, hLen, nch, &p)) return fail(r.status, r.message);
    const size_t rows = e.bank ? static_cast<size_t>(nch) : 1;      // tap vectors in `h`, each hLen long
    std::vector<double> pn;
    if (e.pnfb) {
        const double *src = static_cast<const double *>(h);
        pn.assign(src, src + static_cast<size_t>((hLen + p.Nphi - 1) / p.Nphi) * (p.polyorder + 1) * (dtype_is_complex(th) ? 2 : 1));
    } else if (e.family == kCreateFarrow && !create_farrow_banks(h, hLen, th, p.Nphi, p.polyorder, rows, &pn)) {
        return fail(MRHIP_ERR_INVALID_ARG, "polynomial fit is rank deficient");
    }

    DeviceGuard guard(device);
    if (!guard.ok) return fail(MRHIP_ERR_HIP, "hipSetDevice failed");
    auto *f = new mrhip_filter();
    f->th = th; f->tx = tx; f->ty = mrhip_output_dtype(th, tx);
    f->nc = dtype_is_complex(tx) ? 2 : 1;
    f->r_f64 = dtype_is_f64(f->ty);
    f->nch = nch; f->hLen = hLen; f->device = device;
    f->bank = e.bank;
    int rc = MRHIP_OK;
    if (e.family == kCreateRational) {
        // STANDARD (Filters.jl:163-165) / DECIMATOR (:166-168): h = flipud(h); INTERPOLATOR (:169-171) / RATIONAL (:172-174): the bank
        f->kind = p.L == 1 ? (p.M == 1 ? MRHIP_FIR_STANDARD : MRHIP_FIR_DECIMATOR) : (p.M == 1 ? MRHIP_FIR_INTERPOLATOR : MRHIP_FIR_RATIONAL);
        f->L = p.L; f->M = p.M; f->Nphi = p.L;
    } else {
        f->kind = e.family == kCreateArbitrary ? MRHIP_FIR_ARBITRARY : MRHIP_FIR_FARROW;
        f->L = p.Nphi; f->M = 1; f->Nphi = p.Nphi;
        f->rate = p.rate;
        f->delta = static_cast<double>(p.Nphi) / p.rate;   // Δ = N𝜙/rate, Filters.jl:113, :143
        if (e.rates) { f->rates = true; f->h_rates.assign(p.rates, p.rates + nch); }
    }
    if (e.family == kCreateFarrow) {
        f->polyorder = p.polyorder;
        f->T = (hLen + p.Nphi - 1) / p.Nphi;
        f->H = f->T - 1;
        f->h_pnfb = pn;
        // Poly{T} storage: coefficients live in the tap type (Filters.jl:313 Array(Poly{T}, ...)), complex ones per component
        if (!dtype_is_f64(th)) for (double &c : f->h_pnfb) c = static_cast<double>(static_cast<float>(c));
        rc = upload_pnfb(f);
    } else {
        f->T = create_pfb_banks(h, hLen, th, f->Nphi, rows, &f->h_taps, e.family == kCreateArbitrary ? &f->h_dtaps : nullptr);
        f->H = f->T - 1;
        rc = upload_taps(f, f->h_taps, &f->d_taps, &f->d_taps_alloc);
        if (!rc && e.family == kCreateArbitrary) rc = upload_taps(f, f->h_dtaps, &f->d_dtaps, &f->d_dtaps_alloc);
    }
    if (!rc) rc = alloc_common(f);
    if (!rc && f->rates) rc = rates_alloc(f);
    if (rc) { mrhip_destroy(f); return rc; }
    // (per-channel rates: the serial walk of kernels_rates_arb.hip, none of the schedule machinery)
    if (e.family != kCreateRational && !f->rates) sched_configure(f);
    *out = f;
    return MRHIP_OK;
}

}  // namespace

extern "C" {

// ---- the rational family: one bank; one per channel (include/multirate_hip.h, "Per-channel taps"); that with complex taps -------------
int mrhip_create_rational(const void *h, int64_t hLen, int th, int64_t num, int64_t den, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_rational");
    return create_filter(e, h, hLen, th, {.num = num, .den = den}, tx, nch, device, out);
}
int mrhip_create_rational_bank(const void *h, int64_t hLen, int th, int64_t num, int64_t den, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_rational_bank");
    return create_filter(e, h, hLen, th, {.num = num, .den = den}, tx, nch, device, out);
}
int mrhip_create_rational_bank_ctaps(const void *h, int64_t hLen, int th, int64_t num, int64_t den, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_rational_bank_ctaps");
    return create_filter(e, h, hLen, th, {.num = num, .den = den}, tx, nch, device, out);
}

// ---- FIRArbitrary: real and complex taps, a bank per channel of either ("Per-channel taps for FIRArbitrary"), per-channel rates ---------
int mrhip_create_arbitrary(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_arbitrary");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi}, tx, nch, device, out);
}
int mrhip_create_arbitrary_ctaps(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_arbitrary_ctaps");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi}, tx, nch, device, out);
}
int mrhip_create_arbitrary_bank(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_arbitrary_bank");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi}, tx, nch, device, out);
}
int mrhip_create_arbitrary_bank_ctaps(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_arbitrary_bank_ctaps");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi}, tx, nch, device, out);
}
int mrhip_create_arbitrary_rates(const void *h, int64_t hLen, int th, const double *rates, int64_t Nphi, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_arbitrary_rates");
    return create_filter(e, h, hLen, th, {.rates = rates, .Nphi = Nphi}, tx, nch, device, out);
}

// ---- FIRFarrow: the same five, and the three forms that take a caller-fitted bank in place of the taps ---------------------------------
int mrhip_create_farrow(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}
int mrhip_create_farrow_bank(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow_bank");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}
int mrhip_create_farrow_pnfb(const double *pnfb, int64_t hLen, int th, double rate, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow_pnfb");
    return create_filter(e, pnfb, hLen, th, {.rate = rate, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}
int mrhip_create_farrow_rates(const void *h, int64_t hLen, int th, const double *rates, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow_rates");
    return create_filter(e, h, hLen, th, {.rates = rates, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}
int mrhip_create_farrow_rates_pnfb(const double *pnfb, int64_t hLen, int th, const double *rates, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow_rates_pnfb");
    return create_filter(e, pnfb, hLen, th, {.rates = rates, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}
int mrhip_create_farrow_ctaps(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow_ctaps");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}
int mrhip_create_farrow_bank_ctaps(const void *h, int64_t hLen, int th, double rate, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow_bank_ctaps");
    return create_filter(e, h, hLen, th, {.rate = rate, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}
int mrhip_create_farrow_pnfb_ctaps(const double *pnfb, int64_t hLen, int th, double rate, int64_t Nphi, int64_t polyorder, int tx, int64_t nch, int device, mrhip_filter **out)
{
    constexpr const CreateEntry &e = create_entry("mrhip_create_farrow_pnfb_ctaps");
    return create_filter(e, pnfb, hLen, th, {.rate = rate, .Nphi = Nphi, .polyorder = polyorder}, tx, nch, device, out);
}

}  // extern "C"
