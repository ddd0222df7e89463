// kernels_rates_farrow_fit.hip -- the polynomial banks of a FIRFarrow filter with per-channel rates, FITTED ON THE DEVICE from taps that
// live there (mrhip_set_channel_taps_farrow_device, mrhip_set_channel_ctaps_farrow_device; include/multirate_hip.h, "The FIRFarrow fit on
// the device for the filters with per-channel rates").  A block-LMS equaliser or a matched-pulse tracker produces TAPS; the host calls
// pull them over and fit every row there, which costs many times a chunk.  This kernel runs the b side of polyfit_rows (host_logic.cpp)
// for every row of every channel in stream order; the A side -- reflectors, vnorm2, R: the same for every row -- comes in a table the host
// computed once (polyfit_factor).
//
//   rates_farrow_fit_kernel<TAP, NC>: one lane per (channel c, row i, component).  The lane's right-hand side is row i of the channel's
//      polyphase bank, the N𝜙 taps h_c[(T-1-i)*N𝜙 + 𝜙] (0 past hLen; contiguous in memory, a complex row interleaved), widened exactly to
//      Float64 into LDS as b[r][lane]: consecutive lanes on consecutive 8-byte words, so the 64-bit LDS reads and writes are free of bank
//      conflicts, and a lane touches its own column only -- no barrier.  polyfit_apply (rates_arb.h; tests/rates_farrow_fit_check.cpp
//      compiles the same text) leaves the coefficients in the column's first polyorder+1 words; the table entries it reads are indexed by
//      loop counters only, so they are uniform over the wave and arrive as scalar loads (the idiom of the FIRFarrow bank kernels, whose
//      polynomial coefficients are scalar operands).  The lane then writes its coefficients straight into the filter's bank, at the place
//      install_channel_pnfb / install_channel_pnfb_ctaps (api.hip) put them; Float32 taps: every value rounded to Float32 and widened
//      back, per component, as rates_pnfb_install_kernel<true> rounds.  No intermediate array, no second launch.
//
// One wave a workgroup; the workgroup has fewer than 64 lanes where 64 columns of N𝜙 words no longer fit the LDS plan
// (plan_rates_fit).  No workgroup waits for another; plain HIP.
#include "rates_arb.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

template <typename TAP, int NC>
__global__ __launch_bounds__(kFarrowFitMaxLanes) void rates_farrow_fit_kernel(FarrowFitArgs a, const double *__restrict__ table)
{
    extern __shared__ __attribute__((aligned(16))) double rates_fit_smem[];
    const int lanes = blockDim.x;
    double *const b = rates_fit_smem + threadIdx.x;                  // b[r] at b[r * lanes]
    const long long stride = static_cast<long long>(gridDim.x) * lanes;
    for (long long item = static_cast<long long>(blockIdx.x) * lanes + threadIdx.x; item < a.items; item += stride) {
        const FarrowFitItem it = farrow_fit_item(item, a.T, NC);
        const TAP *__restrict__ h = static_cast<const TAP *>(a.h) + it.c * a.hLen * NC;
        const long long j0 = farrow_fit_row_start(it.i, a.T, a.Nphi);
        for (long long phi = 0; phi < a.Nphi; ++phi) {
            const long long j = j0 + phi;
            b[phi * lanes] = j < a.hLen ? static_cast<double>(h[j * NC + it.comp]) : 0.0;
        }
        polyfit_apply(table, a.Nphi, a.m, b, lanes, b, lanes);
        for (int k = 0; k < a.m; ++k) {
            const double v = b[static_cast<long long>(k) * lanes];
            a.pnfb[farrow_fit_dst_index(it, k, a.T, a.m, NC)] = sizeof(TAP) == 4 ? static_cast<double>(static_cast<float>(v)) : v;
        }
    }
}

}  // namespace

hipError_t launch_rates_fit(bool tap_f64, bool complex_h, const FarrowFitArgs &a, const double *table, const FarrowFitPlan &p, hipStream_t st)
{
    if (!table || a.items < 1 || a.hLen < 1 || a.T < 1 || a.Nphi < 1 || a.m < 1 || a.m > a.Nphi || p.lanes < 1 || p.lanes > kFarrowFitMaxLanes ||
        p.lds_bytes != static_cast<size_t>(p.lanes) * static_cast<size_t>(a.Nphi) * sizeof(double) || p.lds_bytes > static_cast<size_t>(kFarrowFitLdsBytes))
        return hipErrorInvalidValue;
    const long long blocks = (a.items + p.lanes - 1) / p.lanes;
    const dim3 grid(static_cast<unsigned>(blocks < (1LL << 20) ? blocks : (1LL << 20)));
    auto kfn = tap_f64 ? (complex_h ? rates_farrow_fit_kernel<double, 2> : rates_farrow_fit_kernel<double, 1>)
                       : (complex_h ? rates_farrow_fit_kernel<float, 2> : rates_farrow_fit_kernel<float, 1>);
    hipLaunchKernelGGL(kfn, grid, dim3(static_cast<unsigned>(p.lanes)), p.lds_bytes, st, a, table);
    return hipGetLastError();
}

}  // namespace mrhip
