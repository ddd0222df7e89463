// kernels_bank_farrow.hip -- FIRFarrow (src/Filters.jl:123-147, 764-839) with PER-CHANNEL taps.
//
// In the reference N channels are N FIRFilter(h_c, rate, N𝜙, polyorder) objects and every h_c may differ (a per-antenna equaliser or a
// per-sensor calibration filter in front of a common, continuously variable rate change).  The phase schedule (update(), :780-792;
// arb_schedule.hip evaluates it) does not depend on the taps, so mrhip_create_farrow_bank builds ONE filter whose channels share rate,
// N𝜙, polyorder, state and call length -- everything but the polynomial bank: channel c reads bank c of a.pnfb, [nch][T][polyorder+1]
// Float64, ascending powers, values representable in the tap type.  These kernels are the only ones such a filter ever reaches (api.hip:
// launch_range tests TypeKey::bank first).  Per output k the schedule supplies the input index n_k and the Float64 phase 𝜙_k:
//
//     taps_c[i] = Th(polyval(pnfb_c[i], 𝜙_k))                  i = 1 .. tapsPer𝜙
//     y_c,k     = sum_i taps_c[i] * ext_c[n_k - T + i]         ext = [history ; x]
//
// Arithmetic (include/multirate_hip.h, "Per-channel taps for FIRFarrow"): that of farrow_kernel (kernels_generic.hip) on bank c -- Horner
// in Float64 from the highest power (t = 𝜙*v; v = coef + t, the product and the sum each rounded once, NEVER fused: farrow_kernel does not
// fuse them under FUSED either), the tap rounded once to the tap type and widened exactly to R; the dot oldest sample first, the first
// product initialises the accumulator, outputs on the seam (n < seam_below) then take R(0) + acc per component (support.jl:46); STRICT: a
// separately rounded multiply and add per tap, FUSED: one explicit fma per tap -- so channel c is bit for bit
// mrhip_create_farrow(h_c, ..., nch = 1) fed x_c.  This file is compiled with -ffp-contract=off; FUSED calls fma explicitly (RealTaps,
// variant_device.h: mac of pipe_stage.h).
//
// What sets these kernels apart from the shared-taps ones: there a lane evaluates its output's taps ONCE and reuses them for every channel;
// here a tap belongs to one (channel, output) and feeds exactly one product, so it is evaluated in the inner loop, used and dropped -- no tap
// column in LDS.  The coefficient address pnfb + (ch*T + i)*(P+1) + j is the same for every lane of a wave (the channel is uniform per
// block / tile, i and j are loop counters): the bank is read through the constant address space, so the loads are scalar loads and the
// coefficients reach the Float64 adds as scalar operands -- no LDS read and no vector register per coefficient.
//
// Both kernels take the count from the call record when a.dyn is set and the ShiftFold epilogue (shiftin! by the workgroup that leaves
// last), with no early return in front of it.
// Shared with the other variant units: variant_device.h (algebra, staging, tile hand-out, launch shapes); the tiled plan: host_logic.cpp.
#include "variant_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

// the polynomial bank is never written while a filter exists: through the constant address space the compiler uses scalar loads for the
// wave-uniform coefficient indices (it cannot prove that for a global pointer next to the y stores)
typedef const __attribute__((address_space(4))) double *farrow_coef_t;

// One tap of one (channel, output): polyval(pnfb_c[i], 𝜙) by Horner in Float64 (Polynomials.jl: y = p[end]; y = p[i] + x*y), stored into
// currentTaps::Vector{Th} (one rounding to the tap type), widened exactly to R.  `c`: the polynomial's P+1 coefficients, wave-uniform.
// PP >= 0: the polyorder at compile time -- the P+1 scalar loads of a tap are issued together and waited for once; PP < 0: any polyorder,
// one load and one wait per Horner step.  The arithmetic is the same statement either way.
template <typename R, int PP>
__device__ __forceinline__ R farrow_bank_tap(farrow_coef_t c, const int P, const double phase, const bool tap_f32)
{
    double v;
    if constexpr (PP >= 0) {
        double cj[PP + 1];
#pragma unroll
        for (int j = 0; j <= PP; ++j) cj[j] = c[j];
        v = cj[PP];
#pragma unroll
        for (int j = PP - 1; j >= 0; --j) {
            const double t = phase * v;
            v = cj[j] + t;
        }
    } else {
        v = c[P];
        for (int j = P - 1; j >= 0; --j) {
            const double t = phase * v;
            v = c[j] + t;
        }
    }
    return tap_f32 ? static_cast<R>(static_cast<float>(v)) : static_cast<R>(v);
}

// polyorder 4 is the default of every constructor above this library and the one every measurement was taken at: its Horner chain is
// unrolled (kFarrowBankUnrolledP); every other polyorder takes the runtime loop.  The branch is on a kernel argument: uniform.
constexpr int kFarrowBankUnrolledP = 4;

// One thread per output, any (T, polyorder, rate): farrow_kernel with pnfb + ch*T*(P+1), the taps evaluated per (channel, output).
// blockIdx.y strides the channels.  Serves every path: device-planned calls (a.dyn), host-scheduled calls, the pieces of a split call
// (seam_below == 0 on continuation pieces) and captured calls.  No dynamic LDS.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void farrow_bank_generic_kernel(FarrowArgs a)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = CSample<TX, NCX>;
    const long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a.dyn) a.n_out = a.dyn->n_out;              // a device-planned call: the count the schedule's FINISH kernel left
    if (k < a.n_out) {                               // (no early return: every thread takes part in the history epilogue below)
        const long long n = a.n_idx[k];
        const double phase = a.acc[k];
        const int P = a.polyorder, T = a.T;
        const bool tap_f32 = a.tap_f32 != 0;
        const long long base = n - T;               // 0-based index of the oldest sample (>= -H: n >= 1)
        const bool seam = n < a.seam_below;         // kernel.xIdx < kernel.tapsPer𝜙, Filters.jl:818 (never in a piece that continues a call)
        auto channels = [&]<int PP>() {
            for (int ch = blockIdx.y; ch < a.nch; ch += gridDim.y) {
                farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + static_cast<long long>(ch) * T * (P + 1);
                const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
                const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;
                R *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
                auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
                const Sample v0 = sample(base);
                typename A::Sum acc = A::first(farrow_bank_tap<R, PP>(pc, P, phase, tap_f32), v0);
                if (seam) acc = A::zero_start(acc);
                for (int i = 1; i < T; ++i) {
                    const Sample v = sample(base + i);
                    acc = A::step(acc, farrow_bank_tap<R, PP>(pc + i * (P + 1), P, phase, tap_f32), v);
                }
                A::store(yc, k, acc);
            }
        };
        if (P == kFarrowBankUnrolledP) channels.template operator()<kFarrowBankUnrolledP>();
        else channels.template operator()<-1>();
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// Persistent workgroups in the channel-major tile order (tile_run, variant_device.h), computed here from the device-side count
// (tiles_take_dyn with nch groups).  A tile is (channel, run of tile_out = 256 outputs); its run of samples is staged into LDS by plain
// loads (tile_span).  LDS holds the sample run ONLY: a tap feeds one product, and the coefficients are scalar loads (the channel of a
// tile is uniform over the workgroup).  No workgroup communicates with or waits for another.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kVariantThreads) void farrow_bank_tiled_kernel(FarrowArgs a, ArbTileArgs ta)
{
    using A = RealTaps<TX, R, NCX, FUSED>;
    using Sample = CSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_farrow_smem[];
    Sample *const lx = reinterpret_cast<Sample *>(bank_farrow_smem);

    const int tid = threadIdx.x;
    const int T = a.T, P = a.polyorder;
    const bool tap_f32 = a.tap_f32 != 0;
    long long ngroups;                                              // (== nch: a tile covers one channel)
    tiles_take_dyn(a.n_out, ta, ngroups, a.dyn);                    // (a device-planned call: the count from the call record)
    const TileRun run = tile_run(ta.total_tiles);

    for (long long tile = run.begin; tile < run.end; ++tile) {
        const BankTile t = bank_tile<true>(tile, ta, a.n_out);      // (the channel is uniform: said so to the compiler)
        const int ch = t.ch;
        const TileSpan w = tile_span(a.n_idx, t.k0, t.klast, T, ta.max_span);
        farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + static_cast<long long>(ch) * T * (P + 1);
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;

        __syncthreads();   // the previous tile's reads of the window are done
        if (w.staged) stage_window(lx, xc, hc, w.o, static_cast<int>(w.span), a.x_len, a.H, tid);
        __syncthreads();

        R *__restrict__ yc = A::channel_out(a.y, ch, a.y_stride);
        auto outputs = [&]<int PP>() {
            for (long long k = t.k0 + tid; k <= t.klast; k += kVariantThreads) {
                const long long n = a.n_idx[k];
                const double phase = a.acc[k];
                const bool seam = n < a.seam_below;
                auto dot = [&](auto window) {                       // window(i): sample i of this output's window, oldest first
                    const Sample v0 = window(0);
                    typename A::Sum acc = A::first(farrow_bank_tap<R, PP>(pc, P, phase, tap_f32), v0);
                    if (seam) acc = A::zero_start(acc);
                    for (int i = 1; i < T; ++i) {
                        const Sample v = window(i);
                        acc = A::step(acc, farrow_bank_tap<R, PP>(pc + i * (P + 1), P, phase, tap_f32), v);
                    }
                    A::store(yc, k, acc);
                };
                const long long base = n - T;
                const Sample *wp = lx + (n - w.n_lo), *__restrict__ he = hc + a.H;
                if (w.staged) dot([&](int i) { return wp[i]; });
                else dot([&](int i) { const long long xi = base + i; return xi >= 0 ? xc[xi] : he[xi]; });   // the window from global memory
            }
        };
        if (P == kFarrowBankUnrolledP) outputs.template operator()<kFarrowBankUnrolledP>();
        else outputs.template operator()<-1>();
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

}  // namespace

hipError_t launch_farrow_bank_generic(const TypeKey &tk, bool fused, const FarrowArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    return launch_lane_per_output(tk, a, s, "farrow_bank_generic_kernel", kname, [&]<typename TX, typename R, int NCX>() {
        return fused ? farrow_bank_generic_kernel<TX, R, NCX, true> : farrow_bank_generic_kernel<TX, R, NCX, false>;
    });
}

bool plan_farrow_bank_tiled(const TypeKey &tk, const FarrowArgs &a, double rate, int num_cus, ArbTileArgs *out, size_t *lds)
{
    return plan_farrow_bank_tiled(tk, a, rate, num_cus, MRHIP_ENV_INT("MRHIP_FARROW_BANK_TILED", -1), out, lds);
}

hipError_t launch_farrow_bank_tiled(const TypeKey &tk, bool fused, const FarrowArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                    const char **kname, int num_cus)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    *kname = "farrow_bank_tiled_kernel";
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_FARROW_BANK_GRID", 0);
    return dispatch_variant(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        return launch_persistent(fused ? farrow_bank_tiled_kernel<TX, R, NCX, true> : farrow_bank_tiled_kernel<TX, R, NCX, false>, a, ta, lds, s,
                                 num_cus, GridOverride::replace, grid_fixed);
    });
}

}  // namespace mrhip
