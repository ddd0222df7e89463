// pipe_stage.h -- what the arbitrary-rate kernels share: the multiply-add (mac) of all of them (kernels_arbitrary.hip,
// kernels_arb_pipe.hip, kernels_farrow_pipe.hip) and, through the real-tap algebra of variant_device.h, of the per-channel-taps
// kernels of all three families (kernels_bank.hip, kernels_bank_arb.hip, kernels_bank_farrow.hip); the hand-out of tiles of
// arb_tiled_kernel and farrow_tiled_kernel, and for the
// two hand-scheduled pipe kernels the scalar-base pointers, the synchronous take-over of the schedule's first index and the
// planning of their sample buffers on the host (their grids: persistent_grid, mrhip_internal.h).  (The pipe kernels' staging lambdas and their own hand-out code are
// still written out in each of them.)
#pragma once

#include <cstdint>
#include <type_traits>

#include "mrhip_internal.h"
#include "pair_device.h"

#pragma clang fp contract(off)

namespace mrhip {

template <bool FUSED, typename R>
__device__ __forceinline__ R mac(R t, R x, R acc)
{
    if constexpr (FUSED) {
        if constexpr (sizeof(R) == 4) return __builtin_fmaf(t, x, acc);
        else return __builtin_fma(t, x, acc);
    } else {
        const R p = t * x;
        return acc + p;
    }
}

// A wave-uniform GLOBAL pointer the compiler can no longer fold into vector address arithmetic: base (SGPR pair) + 32-bit
// lane offset then selects the scalar-base form of global_load / global_store (no 64-bit vector adds per access).  The result
// is typed as an address-space-1 pointer: rebuilt from integers as a generic pointer it is accessed with flat_load /
// flat_store, which also count in lgkmcnt -- the counter the hand-issued LDS pipeline waits on.
template <typename P>
using global_ptr = __attribute__((address_space(1))) P *;
template <typename P>
__device__ __forceinline__ global_ptr<P> opaque_uniform(P *p)
{
    unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(reinterpret_cast<uintptr_t>(p)));
    unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) >> 32));
    asm volatile("" : "+s"(lo), "+s"(hi));
    return reinterpret_cast<global_ptr<P>>((static_cast<unsigned long long>(hi) << 32) | lo);
}

template <typename TX, typename R, int NC>
__device__ __forceinline__ R sample_part(dev::v2u_t v, int c)     // 8-byte sample: component c
{
    if constexpr (NC == 1) {
        static_assert(sizeof(TX) == 8 && sizeof(R) == 8, "one 8-byte real sample");
        return __builtin_bit_cast(double, v);
    } else {
        static_assert(sizeof(TX) == 4 && NC == 2, "one ComplexF32 sample");
        return static_cast<R>(__builtin_bit_cast(float, c == 0 ? v.x : v.y));
    }
}

// n_idx[first output of tile tau], as a scalar.  In the tile loops it is loaded TWO tiles ahead by an ordinary load and taken over
// into a scalar behind a staging wait, where nothing is in flight any more: left to a load at the top of the tile the compiler
// waits s_waitcnt vmcnt(0) there -- the previous tile's output stores included, microseconds per tile.  This synchronous form
// serves the first tiles of a workgroup.  (Round 3 first issued it as an asynchronous s_load_dword from inline assembly and waited
// a tile later: the compiler, which takes an asm output for valid at once, spilled and re-used that SGPR while the load was still
// in flight, and the landing data overwrote whatever lived there -- whole tiles of zeros in workgroups that take more than one
// tile, for some instantiations only.)
__device__ __forceinline__ int first_index_sync(const int *n_idx, long long tau, int threads)
{
    const int *p = n_idx + tau * threads;
    const unsigned plo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(reinterpret_cast<uintptr_t>(p)));
    const unsigned phi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) >> 32));
    const unsigned long long pu = (static_cast<unsigned long long>(phi) << 32) | plo;
    int v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(pu));   // (valid when the statement ends)
    return v;
}

// Tiles handed out in runs (ArbTileArgs::counters; kernels_arb_pipe.hip has the story): the workgroups of a CU do not advance evenly,
// with tile += gridDim the kernel's tail runs under-occupied.  Two runs are always in hand; lane 0 asks for another when one is
// taken into use and publishes the answer before the barrier at the top of the next tile.
struct TileHandout {
    unsigned *ctr;
    long long G, q0, q1;
    int run;
    static constexpr long long kNone = -1;
    __device__ __forceinline__ long long first(unsigned *counters, int run_tiles, unsigned *s_grab, int tid)
    {
        ctr = counters; G = gridDim.x; run = ctr ? run_tiles : 1; q0 = q1 = kNone;
        if (ctr) {
            if (tid == 0) { const unsigned b = atomicAdd(ctr, 2u); s_grab[0] = b; s_grab[1] = b + 1u; }
            __syncthreads();
            q0 = (G + s_grab[0]) * run; q1 = (G + s_grab[1]) * run;
            __syncthreads();
        }
        return static_cast<long long>(blockIdx.x) * run;
    }
    __device__ __forceinline__ long long after(long long t)       // the tile this workgroup takes after t
    {
        if (!ctr) return t + G;
        if (((t + 1) & (run - 1)) != 0) return t + 1;          // (run is a power of two)
        const long long r = q0;
        q0 = q1; q1 = kNone;
        return r;
    }
    __device__ __forceinline__ bool wants() const { return ctr && q1 == kNone; }
    __device__ __forceinline__ void take(const unsigned *s_grab, unsigned it) { q1 = (G + s_grab[it & 1]) * run; }
    __device__ __forceinline__ void leave(int tid) const          // every workgroup, the ones without a tile too
    {
        if (ctr && tid == 0) {
            __threadfence();                                      // (this workgroup's requests are in before it counts itself off)
            if (atomicAdd(ctr + 64, 1u) == static_cast<unsigned>(G) - 1u) {
                __threadfence();
                ctr[0] = 0u; ctr[64] = 0u;                        // re-armed for the next launch (stream order makes it visible)
            }
        }
    }
};

// ---- host side ------------------------------------------------------------------------------------------------

// Buffer geometry of a pipe kernel's plan: `copies` copies of [cpl][max_span] samples of `sb` bytes per buffer.  LDS-DMA staging
// (prefetch = 1): rows of whole 16-byte chunks, a copy rounded up to whole 1 KiB wave transfers, at most 16 of them; the lane
// offsets of the transfers are 32-bit: the channels of a group must lie within 2 GiB of each other.  Copy B starts 128 B (mod
// 256) behind copy A: the lanes of one read that use it do not land on their neighbours' banks.
struct PipeStagePlan { int row_pitch, dma_slots, prefetch, copyb_pad; size_t buf_bytes; };
inline PipeStagePlan pipe_stage_plan(size_t sb, int cpl, long long max_span, long long x_stride, int copies, bool allow_dma = true)
{
    const long long row_chunks = (max_span * static_cast<long long>(sb) + 15) / 16;
    const long long nslots = (row_chunks * cpl + 63) / 64;
    const bool dma = allow_dma && MRHIP_ENV_INT("MRHIP_PIPE_DMA", 1) != 0 && nslots <= 16 &&
                     static_cast<double>(cpl) * static_cast<double>(x_stride) * static_cast<double>(sb) < 2147483648.0;
    PipeStagePlan p{};
    p.row_pitch = static_cast<int>(row_chunks * 16 / static_cast<long long>(sb));
    p.dma_slots = static_cast<int>(nslots);
    p.prefetch = dma ? 1 : 0;
    if (dma) {
        p.copyb_pad = copies == 2 ? static_cast<int>(128 / sb) : 0;          // (a copy is a multiple of 1 KiB)
        p.buf_bytes = static_cast<size_t>(nslots) * 1024 * copies + p.copyb_pad * sb;
    } else {
        p.copyb_pad = copies == 2 ? static_cast<int>((128 + 256 - (static_cast<size_t>(max_span) * sb * cpl) % 256) % 256 / sb) : 0;
        p.buf_bytes = (static_cast<size_t>(max_span) * cpl * copies + p.copyb_pad) * sb;
    }
    return p;
}

}  // namespace mrhip
