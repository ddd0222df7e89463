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
// mrhip_create_farrow(h_c, ..., nch = 1) fed x_c.  This file is compiled with -ffp-contract=off; FUSED calls fma explicitly.
//
// What sets these kernels apart from the shared-taps ones: there a lane evaluates its output's taps ONCE and reuses them for every channel;
// here a tap belongs to one (channel, output) and feeds exactly one product, so it is evaluated in the inner loop, used and dropped -- no tap
// column in LDS.  The coefficient address pnfb + (ch*T + i)*(P+1) + j is the same for every lane of a wave (the channel is uniform per
// block / tile, i and j are loop counters): the bank is read through the constant address space, so the loads are scalar loads and the
// coefficients reach the Float64 adds as scalar operands -- no LDS read and no vector register per coefficient.
//
// Both kernels take the count from the call record when a.dyn is set and the ShiftFold epilogue (shiftin! by the workgroup that leaves
// last), with no early return in front of it.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "mrhip_internal.h"
#include "pair_device.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

constexpr int kFarrowBankThreads = 256;

// the polynomial bank is never written while a filter exists: through the constant address space the compiler uses scalar loads for the
// wave-uniform coefficient indices (it cannot prove that for a global pointer next to the y stores)
typedef const __attribute__((address_space(4))) double *farrow_coef_t;

template <typename R, bool FUSED>
__device__ __forceinline__ R mac(R t, R x, R acc)
{
    if constexpr (FUSED) {
        if constexpr (sizeof(R) == 4) return __builtin_fmaf(t, x, acc);
        else return __builtin_fma(t, x, acc);
    } else {
        R p = t * x;
        return acc + p;
    }
}

template <typename TX, int NCX>
struct alignas(sizeof(TX) * NCX) BankSample { TX c[NCX]; };

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
__global__ __launch_bounds__(kFarrowBankThreads) void farrow_bank_generic_kernel(FarrowArgs a)
{
    using Sample = BankSample<TX, NCX>;
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
                R *__restrict__ yc = static_cast<R *>(a.y) + static_cast<long long>(ch) * a.y_stride * NCX;
                auto sample = [&](long long xi) -> Sample { return xi >= 0 ? xc[xi] : hc[static_cast<long long>(a.H) + xi]; };
                R acc[NCX];
                {
                    const Sample v = sample(base);
                    const R t = farrow_bank_tap<R, PP>(pc, P, phase, tap_f32);
#pragma unroll
                    for (int c = 0; c < NCX; ++c) acc[c] = t * static_cast<R>(v.c[c]);
                }
                if (seam) {
#pragma unroll
                    for (int c = 0; c < NCX; ++c) acc[c] = static_cast<R>(0) + acc[c];
                }
                for (int i = 1; i < T; ++i) {
                    const Sample v = sample(base + i);
                    const R t = farrow_bank_tap<R, PP>(pc + i * (P + 1), P, phase, tap_f32);
#pragma unroll
                    for (int c = 0; c < NCX; ++c) acc[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), acc[c]);
                }
#pragma unroll
                for (int c = 0; c < NCX; ++c) yc[k * NCX + c] = acc[c];
            }
        };
        if (P == kFarrowBankUnrolledP) channels.template operator()<kFarrowBankUnrolledP>();
        else channels.template operator()<-1>();
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// Persistent workgroups: tile order and ownership are arb_bank_tiled_kernel's.  A tile is (channel, run of tile_out = 256 outputs); the
// tiles are ordered channel-major and workgroup b owns ONE contiguous run of that order, computed here from the device-side count
// (tiles_take_dyn with nch groups).  The contiguous [history ; x] run between the tile's first and last n_idx (the schedule is
// non-decreasing in k: x[n_idx[k0] - T ... n_idx[klast])) is read from the schedule HERE and staged into LDS by plain loads; a tile whose
// run is longer than the planned span (ta.max_span: a heavily decimating rate) reads its windows from global memory.  LDS holds the sample
// run ONLY: a tap feeds one product, and the coefficients are scalar loads (the channel of a tile is uniform over the workgroup).  No
// workgroup communicates with or waits for another.
template <typename TX, typename R, int NCX, bool FUSED>
__global__ __launch_bounds__(kFarrowBankThreads) void farrow_bank_tiled_kernel(FarrowArgs a, ArbTileArgs ta)
{
    using Sample = BankSample<TX, NCX>;
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_farrow_smem[];
    Sample *const lx = reinterpret_cast<Sample *>(bank_farrow_smem);

    const int tid = threadIdx.x;
    const int T = a.T, P = a.polyorder;
    const bool tap_f32 = a.tap_f32 != 0;
    long long ngroups;                                              // (== nch: a tile covers one channel)
    tiles_take_dyn(a.n_out, ta, ngroups, a.dyn);                    // (a device-planned call: the count from the call record)

    // this workgroup's run of the channel-major tile order: [t_begin, t_end)
    const long long per = ta.total_tiles / gridDim.x, extra = ta.total_tiles - per * gridDim.x;
    const long long b = blockIdx.x;
    const long long t_begin = b * per + (b < extra ? b : extra);
    const long long t_end = t_begin + per + (b < extra ? 1 : 0);

    for (long long tile = t_begin; tile < t_end; ++tile) {
        const int ch = __builtin_amdgcn_readfirstlane(static_cast<int>(tile / ta.tiles_per_channel));   // (uniform: said so to the compiler)
        const long long tau = tile - static_cast<long long>(ch) * ta.tiles_per_channel;
        const long long k0 = tau * ta.tile_out;
        const long long klast = (k0 + ta.tile_out < a.n_out ? k0 + ta.tile_out : a.n_out) - 1;
        const long long n_lo = a.n_idx[k0], n_hi = a.n_idx[klast];
        const long long o = n_lo - T;                                                   // 0-based x index of LDS sample 0 (>= -H)
        const long long span = n_hi - n_lo + T;
        const bool staged = span <= ta.max_span;                                        // (uniform over the workgroup)
        farrow_coef_t pc = reinterpret_cast<farrow_coef_t>(reinterpret_cast<uintptr_t>(a.pnfb)) + static_cast<long long>(ch) * T * (P + 1);
        const Sample *__restrict__ xc = static_cast<const Sample *>(a.x) + static_cast<long long>(ch) * a.x_stride;
        const Sample *__restrict__ hc = static_cast<const Sample *>(a.hist) + static_cast<long long>(ch) * a.H;

        __syncthreads();   // the previous tile's reads of the window are done
        if (staged) {
            for (int s = tid; s < static_cast<int>(span); s += kFarrowBankThreads) {
                const long long gi = o + s;
                Sample v;
#pragma unroll
                for (int c = 0; c < NCX; ++c) v.c[c] = static_cast<TX>(0);
                if (gi >= 0) { if (gi < a.x_len) v = xc[gi]; }
                else if (gi >= -static_cast<long long>(a.H)) v = hc[a.H + gi];
                lx[s] = v;
            }
        }
        __syncthreads();

        R *__restrict__ yc = static_cast<R *>(a.y) + static_cast<long long>(ch) * a.y_stride * NCX;
        auto outputs = [&]<int PP>() {
            for (long long k = k0 + tid; k <= klast; k += kFarrowBankThreads) {
                const long long n = a.n_idx[k];
                const double phase = a.acc[k];
                const bool seam = n < a.seam_below;
                R acc[NCX];
                if (staged) {
                    const Sample *wp = lx + (n - n_lo);             // oldest sample of this output's window
                    {
                        const Sample v = wp[0];
                        const R t = farrow_bank_tap<R, PP>(pc, P, phase, tap_f32);
#pragma unroll
                        for (int c = 0; c < NCX; ++c) acc[c] = t * static_cast<R>(v.c[c]);
                    }
                    if (seam) {
#pragma unroll
                        for (int c = 0; c < NCX; ++c) acc[c] = static_cast<R>(0) + acc[c];
                    }
                    for (int i = 1; i < T; ++i) {
                        const Sample v = wp[i];
                        const R t = farrow_bank_tap<R, PP>(pc + i * (P + 1), P, phase, tap_f32);
#pragma unroll
                        for (int c = 0; c < NCX; ++c) acc[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), acc[c]);
                    }
                } else {
                    // the window from global memory
                    const long long base = n - T;
                    const Sample *__restrict__ he = hc + a.H;
                    {
                        const Sample v = base >= 0 ? xc[base] : he[base];
                        const R t = farrow_bank_tap<R, PP>(pc, P, phase, tap_f32);
#pragma unroll
                        for (int c = 0; c < NCX; ++c) acc[c] = t * static_cast<R>(v.c[c]);
                    }
                    if (seam) {
#pragma unroll
                        for (int c = 0; c < NCX; ++c) acc[c] = static_cast<R>(0) + acc[c];
                    }
                    for (int i = 1; i < T; ++i) {
                        const long long xi = base + i;
                        const Sample v = xi >= 0 ? xc[xi] : he[xi];
                        const R t = farrow_bank_tap<R, PP>(pc + i * (P + 1), P, phase, tap_f32);
#pragma unroll
                        for (int c = 0; c < NCX; ++c) acc[c] = mac<R, FUSED>(t, static_cast<R>(v.c[c]), acc[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < NCX; ++c) yc[k * NCX + c] = acc[c];
            }
        };
        if (P == kFarrowBankUnrolledP) outputs.template operator()<kFarrowBankUnrolledP>();
        else outputs.template operator()<-1>();
    }
    dev::shiftin_by_last_workgroup<TX, NCX>(a.fold, a.x, a.hist, a.x_stride, a.x_len, a.H, a.nch);
}

// (Tx scalar, R) combinations that promote_type can produce: (f32,f32) (f32,f64) (f64,f64), real and complex samples
template <typename F>
hipError_t dispatch_farrow_bank(const TypeKey &tk, F &&f)
{
    if (!tk.x_f64 && !tk.r_f64) return tk.complex_x ? f.template operator()<float, float, 2>() : f.template operator()<float, float, 1>();
    if (!tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<float, double, 2>() : f.template operator()<float, double, 1>();
    if (tk.x_f64 && tk.r_f64) return tk.complex_x ? f.template operator()<double, double, 2>() : f.template operator()<double, double, 1>();
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_farrow_bank_generic(const TypeKey &tk, bool fused, const FarrowArgs &a, hipStream_t s, const char **kname)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    if (a.n_out <= 0 && !a.dyn) return hipSuccess;
    const long long bx = a.n_out > 0 ? (a.n_out + kFarrowBankThreads - 1) / kFarrowBankThreads : 1;
    if (bx > 0x7fffffffLL) return hipErrorInvalidValue;
    *kname = "farrow_bank_generic_kernel";
    const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(a.nch < 65535 ? a.nch : 65535), 1);
    return dispatch_farrow_bank(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        if (fused) launch_kernel(farrow_bank_generic_kernel<TX, R, NCX, true>, grid, dim3(kFarrowBankThreads), 0, s, a);
        else launch_kernel(farrow_bank_generic_kernel<TX, R, NCX, false>, grid, dim3(kFarrowBankThreads), 0, s, a);
        return hipGetLastError();
    });
}

// Eligibility of farrow_bank_tiled_kernel: the sample run of a tile fits LDS at two workgroups a CU (the samples take at most 40 KiB; LDS
// holds nothing else).  A tile is 256 outputs (a lane each) of one channel; its planned span follows from the rate -- consecutive outputs
// are 1/rate samples apart -- and is cut to 40 KiB only because the kernel is forced (below): tiles with a longer run read global memory.
// MRHIP_FARROW_BANK_TILED=0: never; =1: wherever the plan fits (tests, measurements); unset: the measured rule -- which is NEVER: the
// tiled kernel beat the universal one nowhere by more than the spread of the repeats (profiles/r07/farrow_bank.txt:
// 0.76 ... 0.98 times its speed at Float32 samples, 166 ... 530 752 tiles; at 64 ch x 1e7 Float64, 2 618 048 tiles, 16.27 against 16.67 ms
// in one run and 16.68 against 16.80 with a spread of 0.46 in the next), so it stays behind its switch.
bool plan_farrow_bank_tiled(const TypeKey &tk, const FarrowArgs &a, double rate, int /*num_cus*/, ArbTileArgs *out, size_t *lds)
{
    const int mode = MRHIP_ENV_INT("MRHIP_FARROW_BANK_TILED", -1);
    if (mode != 1 || !tk.bank || tk.complex_h || a.n_out < 1 || a.T < 1 || a.polyorder < 0 || !(rate > 0.0)) return false;
    const size_t sb = (tk.x_f64 ? 8 : 4) * (tk.complex_x ? 2 : 1);                      // one sample
    constexpr size_t kSampleBytesMax = 40 * 1024;
    const long long tile_out = kFarrowBankThreads;
    // samples the run of a tile can hold: n advances by at most ceil(1/rate) + 1 per output (update(), Filters.jl:780-788)
    const double per_tile = std::ceil(static_cast<double>(tile_out - 1) / rate) + static_cast<double>(a.T) + 2.0;
    long long max_span = static_cast<long long>(kSampleBytesMax / sb);
    if (per_tile <= static_cast<double>(max_span)) max_span = static_cast<long long>(per_tile);   // (else: the span is cut)
    if (max_span < a.T + 1) return false;                                               // not even one window
    ArbTileArgs ta{};
    ta.cpl = 1;
    ta.max_span = static_cast<int>(max_span);
    ta.tile_out = tile_out;
    ta.tiles_per_channel = (a.n_out + tile_out - 1) / tile_out;
    ta.total_tiles = ta.tiles_per_channel * a.nch;
    *out = ta;
    *lds = static_cast<size_t>(max_span) * sb;
    return true;
}

hipError_t launch_farrow_bank_tiled(const TypeKey &tk, bool fused, const FarrowArgs &a, const ArbTileArgs &ta, size_t lds, hipStream_t s,
                                    const char **kname, int num_cus)
{
    if (!tk.bank || tk.complex_h) return hipErrorInvalidValue;
    *kname = "farrow_bank_tiled_kernel";
    // MRHIP_FARROW_BANK_GRID: the number of workgroups of the launch (tests: one workgroup that walks every channel, runs that cross a
    // channel in mid-run, more workgroups than tiles)
    const int grid_fixed = MRHIP_ENV_INT("MRHIP_FARROW_BANK_GRID", 0);
    return dispatch_farrow_bank(tk, [&]<typename TX, typename R, int NCX>() -> hipError_t {
        auto go = [&](auto kfn) -> hipError_t {
            const PersistentGrid pg = persistent_grid(reinterpret_cast<const void *>(kfn), kFarrowBankThreads, lds, num_cus, ta.total_tiles);
            if (pg.err != hipSuccess) return pg.err;
            long long g = std::max<long long>(std::min<long long>(pg.grid, ta.total_tiles), 1);
            if (grid_fixed > 0) g = std::min<long long>(grid_fixed, 65535);
            launch_kernel(kfn, dim3(static_cast<unsigned>(g)), dim3(kFarrowBankThreads), lds, s, a, ta);
            return hipGetLastError();
        };
        return fused ? go(farrow_bank_tiled_kernel<TX, R, NCX, true>) : go(farrow_bank_tiled_kernel<TX, R, NCX, false>);
    });
}

}  // namespace mrhip
