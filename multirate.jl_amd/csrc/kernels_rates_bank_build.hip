// kernels_rates_bank_build.hip -- the per-channel banks of the filters with per-channel rates, built ON THE DEVICE from taps or
// coefficients that live there (mrhip_set_channel_taps_device, mrhip_set_channel_pnfb_device; include/multirate_hip.h, "Device-resident
// updates for the filters with per-channel rates").  A tracker or a block-LMS equaliser computes the next taps from the last chunk's
// outputs on the GPU; these kernels install them in stream order, behind the filter calls already enqueued and ahead of the next one, so
// the host neither sees the values nor waits for the stream.
//
//   rates_bank_build_kernel<TAP, R>: FIRArbitrary.  The pfb and dpfb banks of every channel from the channel's row of taps -- what
//      create_pfb_banks and the widening of mrhip_set_channel_taps produce, bit for bit: the index map and the ONE subtraction per dpfb
//      element, rounded in the tap type, are rates_bank_tap_index / rates_bank_pfb_value / rates_bank_dpfb_value of rates_arb.h (the host
//      program tests/rates_device_updates_check.cpp compiles the same text); the widening TAP -> R is exact.  One workgroup per
//      (channel, slab of kBankBuildSlab bank elements).  Consecutive bank elements of a phase read taps N𝜙 apart, so the channel's row
//      goes through LDS first, with coalesced loads, when its hLen taps fit kBankBuildLdsBytes; a longer row is read from global memory
//      directly.  Both banks are stored with consecutive lanes on consecutive addresses.
//   rates_pnfb_install_kernel<F32>: FIRFarrow.  nch * T * (polyorder+1) Float64 coefficients into the filter's banks; Float32 taps: every
//      value rounded to Float32 and widened back, as install_channel_pnfb (api.hip) rounds on the host.
//
// No workgroup waits for another; plain HIP.
#include "rates_arb.h"

#pragma clang fp contract(off)

namespace mrhip {
namespace {

template <typename TAP, typename R>
__global__ __launch_bounds__(kBankBuildThreads) void rates_bank_build_kernel(BankBuildArgs b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rates_build_smem[];
    TAP *const lrow = reinterpret_cast<TAP *>(rates_build_smem);
    const int tid = threadIdx.x;
    const long long bank = b.Nphi * b.T;
    const long long e0 = static_cast<long long>(blockIdx.x) * kBankBuildSlab;
    const long long e1 = e0 + kBankBuildSlab < bank ? e0 + kBankBuildSlab : bank;
    for (int ch = blockIdx.y; ch < b.nch; ch += gridDim.y) {       // (uniform over the workgroup)
        const TAP *__restrict__ h = static_cast<const TAP *>(b.h) + static_cast<long long>(ch) * b.hLen;
        const TAP *src = h;
        if (b.row_in_lds) {
            __syncthreads();                                       // the previous channel's reads of the row are done
            for (long long j = tid; j < b.hLen; j += kBankBuildThreads) lrow[j] = h[j];
            __syncthreads();
            src = lrow;
        }
        R *__restrict__ p = static_cast<R *>(b.pfb) + static_cast<long long>(ch) * bank;
        R *__restrict__ d = static_cast<R *>(b.dpfb) + static_cast<long long>(ch) * bank;
        for (long long e = e0 + tid; e < e1; e += kBankBuildThreads) {
            const long long j = rates_bank_tap_index(e, b.T, b.Nphi);
            p[e] = static_cast<R>(rates_bank_pfb_value<TAP>(src, b.hLen, j));
            d[e] = static_cast<R>(rates_bank_dpfb_value<TAP>(src, b.hLen, j));
        }
    }
}

template <bool F32>
__global__ __launch_bounds__(kBankBuildThreads) void rates_pnfb_install_kernel(const double *__restrict__ src, double *__restrict__ dst, long long n)
{
    const long long stride = static_cast<long long>(gridDim.x) * kBankBuildThreads;
    for (long long i = static_cast<long long>(blockIdx.x) * kBankBuildThreads + threadIdx.x; i < n; i += stride) {
        const double v = src[i];
        dst[i] = F32 ? static_cast<double>(static_cast<float>(v)) : v;
    }
}

}  // namespace

hipError_t launch_rates_bank_build(bool tap_f64, bool r_f64, const BankBuildArgs &b, hipStream_t st)
{
    if (b.nch < 1 || b.hLen < 1 || b.T < 1 || b.Nphi < 1 || (tap_f64 && !r_f64)) return hipErrorInvalidValue;
    const long long slabs = (b.Nphi * b.T + kBankBuildSlab - 1) / kBankBuildSlab;
    if (slabs > 0x7fffffffLL) return hipErrorInvalidValue;
    BankBuildArgs a = b;
    const long long row_bytes = b.hLen * static_cast<long long>(tap_f64 ? sizeof(double) : sizeof(float));
    a.row_in_lds = row_bytes <= kBankBuildLdsBytes ? 1 : 0;
    const size_t lds = a.row_in_lds ? static_cast<size_t>(row_bytes) : 0;
    const dim3 grid(static_cast<unsigned>(slabs), static_cast<unsigned>(b.nch < 65535 ? b.nch : 65535), 1);
    auto kfn = tap_f64 ? rates_bank_build_kernel<double, double> : r_f64 ? rates_bank_build_kernel<float, double> : rates_bank_build_kernel<float, float>;
    hipLaunchKernelGGL(kfn, grid, dim3(kBankBuildThreads), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_rates_pnfb_install(bool tap_f32, const double *src, double *dst, long long n, hipStream_t st)
{
    if (n < 1) return hipErrorInvalidValue;
    const long long blocks = (n + kBankBuildThreads - 1) / kBankBuildThreads;
    const dim3 grid(static_cast<unsigned>(blocks < 65535 ? blocks : 65535));
    if (tap_f32) hipLaunchKernelGGL(rates_pnfb_install_kernel<true>, grid, dim3(kBankBuildThreads), 0, st, src, dst, n);
    else hipLaunchKernelGGL(rates_pnfb_install_kernel<false>, grid, dim3(kBankBuildThreads), 0, st, src, dst, n);
    return hipGetLastError();
}

}  // namespace mrhip
