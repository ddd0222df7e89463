// opair_kernel.inc -- the output-pair polyphase kernel and its launcher template.  Included by the translation units
// kernels_rational_opair_f32_s{0r,0c,1r,1c,2..5}.hip, _f32_s{0,1}_long.hip, _wide_s{0,1}.hip and _cmix_s{0,1}.hip (one per arithmetic width and per
// SMIN = floor(M/L)), which instantiate tapsPerPhi = 1..48 (32 for Float64 arithmetic and for SMIN >= 2); the mapping is
// described in kernels_rational_opair.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "mrhip_internal.h"
#include "pair_device.h"
#include "pair_loader.h"

#pragma clang fp contract(off)

#ifndef MRHIP_OPAIR_WIDE_LONG
#define MRHIP_OPAIR_WIDE_LONG 1      // Float64 arithmetic on real samples: 33..48 taps per phase too (two waves per SIMD)
#endif

namespace mrhip {
namespace {

constexpr int kOMaxThreads = 512;

using namespace dev;

// one multiply-accumulate of a slot; COND: the slot is outside the window for the lanes where `used` is false
__device__ __forceinline__ float fma_r(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_r(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <bool FUSED, bool FIRST, bool COND, typename R>
__device__ __forceinline__ R slot_mac(R tap, R w, R acc, bool used)
{
    if constexpr (FIRST) {
        const R p = tap * w;                           // the first product initialises the accumulator
        if constexpr (COND) return used ? p : static_cast<R>(-0.0);
        else return p;
    } else if constexpr (FUSED) {
        const R r = fma_r(tap, w, acc);
        if constexpr (COND) return used ? r : acc;
        else return r;
    } else {
        R p = tap * w;
        if constexpr (COND) p = used ? p : static_cast<R>(-0.0);   // acc + (-0.0) == acc, bit for bit
        return acc + p;
    }
}

// T taps per phase; NC components per sample (1 real, 2 complex); SMIN = floor(M/L) in 0..5; TXS = scalar type of
// the samples, R = scalar type of taps, arithmetic and outputs (promote_type(Th, Tx), Filters.jl:581): (Float32,
// Float32), (Float64, Float64) and the reference README's mixed case (Float32 samples, Float64 taps: every sample is
// widened exactly, as Julia's promotion does on every multiply).  Float64 arithmetic doubles the tap registers (~135
// VGPRs: three waves per SIMD; capping it at 128 spills a tap pair into the step loop, whose reload would make the
// compute waves wait on vmcnt, i.e. on their own output stores -- the one thing their tile loop never does: descriptors come by LDS
// instructions, pair_device.h: desc_get2).
// PLAIN: an instantiation for calls the host planned for ONE filter (no call record, no stream descriptors): its kernel arguments
// are never overwritten at entry, so they can be re-read from the kernarg segment instead of living in -- and being spilled
// from -- SGPRs (profiles/r04/experiments.md A: the overrides cost the headline 0.6-0.8 % and its 1e6-sample launches 1.5 %).
// Built for 24 and 32 taps per phase (the BASELINE configs' shapes), STRICT, M/L < 2: see opair_plain_instantiated().
// MODE 2 (RING): the resident consumer of a ring of arriving chunks (mrhip_internal.h: RingDesc; pair_loader.h: pair_ring_loader_wave): per
// tile the compute waves take the output address, the outputs left in the channel and the chunk's u0 from the tile's descriptor in
// LDS (the tap columns are re-gathered when u0 changes), store write-through and report every completed grab.  Same slots, same order,
// same roundings: bit-identical to the other two.
template <int T, bool FUSED, int NC, int SMIN, typename TXS, typename R, int MODE = 0>
#ifndef MRHIP_OPAIR_WIDE_WAVES
#define MRHIP_OPAIR_WIDE_WAVES 3
#endif
#ifndef MRHIP_RING_WAVES
#define MRHIP_RING_WAVES 4          // (6 would force 80 VGPRs = three workgroups per CU, but the loader then works out of scratch memory and becomes the bottleneck)
#endif
// (Float64 arithmetic with more than 32 taps per phase: up to 256 VGPRs, so a workgroup is at most eight waves: the plan keeps
//  its lanes within seven compute waves)
// (RING, Float32 arithmetic: six waves per SIMD like the other modes' 77 VGPRs give -- the ring loader's bookkeeping would take 91)
__global__ __launch_bounds__(sizeof(R) == 8 && T > 32 ? kOMaxThreads : kOMaxThreads + 64, sizeof(R) == 8 ? (T > 32 ? 2 : MRHIP_OPAIR_WIDE_WAVES) : (MODE == 2 ? MRHIP_RING_WAVES : 3))
void rational_opair_kernel(PolyArgs a, PairArgs pa)
{
    constexpr unsigned ES = static_cast<unsigned>(sizeof(TXS)) * NC;   // bytes per input sample
    constexpr unsigned OS = static_cast<unsigned>(sizeof(R)) * NC;     // bytes per output sample
    constexpr int NW = static_cast<int>(ES / 4);                       // 32-bit words per input sample (1, 2 or 4)
    static_assert(NW == 1 || NW == 2 || NW == 4, "sample size");
    // a ring unit is one LDS read: two samples of 4 or 8 bytes, or ONE 16-byte sample (ComplexF64)
    using pair_t = std::conditional_t<NW == 1, v2u_t, v4u_t>;
    constexpr int SPRD = NW == 4 ? 1 : 2;                              // samples per ring unit
    constexpr int W = T + SMIN + 2;             // samples of the run a lane may touch
    constexpr int NPR = (W + SPRD - 1) / SPRD;  // aligned reads per lane per step
    constexpr int NA = T + 1, NB = T + 2;       // slots of the two outputs (B's slot j' meets run sample SMIN + j')
    constexpr bool TAILM = T >= 3;              // the slots past a window's end run under a lane mask in EXEC ...
    constexpr bool HEADM = T >= 3 && !FUSED;    // ... and so do the slots in front of its start (otherwise: selects, slot_mac)

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds_base = static_cast<unsigned>(reinterpret_cast<uintptr_t>(smem));
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int ncw = (blockDim.x >> 6) - 1;      // compute waves; the last wave is the loader
    constexpr bool RING = MODE == 2;
    if constexpr (MODE == 0) pair_take_dyn(a, pa); // (MODE 1, 3: PLAIN -- no call record, no stream descriptors) a device-planned call: n_out, u0, d0 and the step walk from the call record

    if (wave == ncw) {
        if constexpr (RING) pair_ring_loader_wave<NW, static_cast<int>(OS)>(a, pa, smem, lane);
        else pair_loader_wave<NW, MODE != 1>(a, pa, smem, lane);   // (joins the tap-bank barrier below when pa.bank_off >= 0; MODE 1: seam tiles element by element)
        return;
    }
    if constexpr (RING) { if (blockIdx.x == 0) return; }   // workgroup 0 is the ring's feeder (its last wave): no barrier is ever used there
    const unsigned desc_base = lds_base + static_cast<unsigned>(pa.flags_off);   // the tile descriptors (pair_device.h: desc_put / desc_get)

    // ---- the lane's two outputs: window starts, offsets into the even-aligned run, shifted tap columns, masks ----
    // 32-bit: plan_rational_opair guarantees c*L <= 1024 and M < 2L, so every product below is < 2^22
    const int Li = static_cast<int>(a.L), Mi = static_cast<int>(a.M);
    int u0 = static_cast<int>(a.u0);                        // (ring mode: the chunk's, from the tile descriptor)
    const bool act = 2 * tid + 1 < pa.P;                    // P = c*L is even
    int uA = u0 + (act ? 2 * tid : 0) * Mi, uB = uA + Mi;
    int qA = uA / Li, phA = uA - qA * Li;
    int qB = uB / Li, phB = uB - qB * Li;
    int run0 = qA & ~1;                                     // first sample of the lane's run (even)
    int offA = qA - run0;                                   // 0 or 1
    int dB = qB - run0 - SMIN;                              // 0, 1 or 2
    R tapA[NA], tapB[NB];
    // the two shifted tap columns straight from global memory (a ring's compute waves: again whenever a chunk arrives with another u0)
    auto gather_taps = [&]() {
        const R *__restrict__ ca = static_cast<const R *>(a.taps) + static_cast<long long>(phA) * T;
        const R *__restrict__ cb = static_cast<const R *>(a.taps) + static_cast<long long>(phB) * T;
        R colA[T], colB[T];
#pragma unroll
        for (int i = 0; i < T; ++i) { colA[i] = ca[i]; colB[i] = cb[i]; }
        // from the last slot down, each pinned: slot j is the last reader of column element j, whose register is free from there on
        // (in any other order the shifted columns live beside the loaded ones: eight VGPRs more than the step loop needs)
#pragma unroll
        for (int j = NA - 1; j >= 0; --j) {
            const R t0 = j < T ? colA[j] : R(0), t1 = j >= 1 ? colA[j - 1] : R(0);
            tapA[j] = act ? (offA == 0 ? t0 : t1) : R(0);
            pin(tapA[j]);
        }
#pragma unroll
        for (int j = NB - 1; j >= 0; --j) {
            const R t0 = j < T ? colB[j] : R(0), t1 = (j >= 1 && j - 1 < T) ? colB[j - 1] : R(0), t2 = j >= 2 ? colB[j - 2] : R(0);
            tapB[j] = act ? (dB == 0 ? t0 : dB == 1 ? t1 : t2) : R(0);
            pin(tapB[j]);
        }
    };
    if constexpr (RING) {
#pragma unroll
        for (int j = 0; j < NA; ++j) tapA[j] = R(0);
#pragma unroll
        for (int j = 0; j < NB; ++j) tapB[j] = R(0);
        u0 = -1;                                            // no chunk seen yet: the first tile gathers
    } else if (pa.bank_off >= 0) {
        // Tap bank through LDS.  Gathering two 4*T-byte columns per lane straight from global memory costs every
        // workgroup 64 scattered column reads per wave instruction (c times the whole bank per workgroup, all
        // workgroups at once at launch: the "ramp" of a short launch).  Instead the compute waves copy the bank once,
        // coalesced, into the LDS of the last pipeline stage (free until the first tile barrier) with an ODD column
        // pitch PT and two pad slots at either end of a column, and every lane reads its two SHIFTED columns from
        // there: slot j of A is element j - offA of the column, so the shift is an address offset and the slots
        // outside the column fall on pads (their products are discarded by the lane masks below, whatever they hold).
        constexpr int PT = (T + 4) | 1;
        R *const bank = reinterpret_cast<R *>(smem + pa.bank_off);
        const R *__restrict__ tg = static_cast<const R *>(a.taps);
        const int ntaps = Li * T;
        for (int idx = tid; idx < ntaps; idx += ncw * 64) {
            const int col = idx / T, i = idx - col * T;
            bank[col * PT + 2 + i] = tg[idx];
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();             // bank complete (the loader wave joins: pair_loader_wave)
        const R *ba = bank + (act ? phA : 0) * PT + 2 - offA;
        const R *bb = bank + (act ? phB : 0) * PT + 2 - (act ? dB : 0);
#pragma unroll
        for (int j = 0; j < NA; ++j) tapA[j] = ba[j];
#pragma unroll
        for (int j = 0; j < NB; ++j) tapB[j] = bb[j];
        // (the reads complete before this wave reaches the first tile barrier: their values are pinned below; the
        //  loader overwrites the stage only after that barrier)
#pragma unroll
        for (int j = 0; j < NA; ++j) pin(tapA[j]);
#pragma unroll
        for (int j = 0; j < NB; ++j) pin(tapB[j]);
    } else gather_taps();
    // which lanes have the end slots inside their window (lane masks; wave-uniform SGPR pairs in the loop)
    bool useA0 = offA == 0, useAT = offA == 1;
    bool useB0 = dB == 0, useB1 = dB <= 1, useBT = dB >= 1, useBT1 = dB == 2;
    // T >= 3: the end slots run under these masks as EXEC (pair_device.h: masked_mac and its kin) -- the lanes a slot is outside of never
    // see it, which is the reference's operation sequence for them; slot 1 of A and slot 2 of B, inside every lane's window, initialise
    // the accumulators, and the slots in front of them are added in front: dB = 0: (p0 + p1) + p2, dB = 1: p1 + p2, dB = 2: p2.
    // FUSED keeps the select form for the heads (masking removes no instruction there).  T <= 2: slots 1 / 2 are not inside every window.
    auto lanes_of = [](bool b) { return static_cast<unsigned long long>(__builtin_amdgcn_ballot_w64(b)); };
    unsigned long long mA0 = lanes_of(useA0), mAT = lanes_of(useAT);
    unsigned long long mB0 = lanes_of(useB0), mB1 = lanes_of(useB1), mBT = lanes_of(useBT), mBT1 = lanes_of(useBT1);

    // The lane's constants of the tile loop, kept in registers: where its run starts within a stage, where its output pair lies within a
    // step, and which lanes own a pair at all (an SGPR pair).  They move only with u0 (a ring's new chunk).  (They used to be re-derived
    // per tile from a fresh lane id -- a 32-bit division, ~29 VALU instructions per tile -- to spare the registers; since the step loop
    // keeps ONE window address and the store's base advances on the scalar side, they fit.)
    unsigned loff = (static_cast<unsigned>(run0) - static_cast<unsigned>(pa.q0)) * ES;
    const unsigned my_out = 2u * static_cast<unsigned>(tid);              // first of the lane's two outputs within a step
    unsigned voff = my_out * OS;
    pin(voff);
    const unsigned long long mIn = lanes_of(act);                         // my_out + 1 < P

    const int n_out = static_cast<int>(a.n_out);
#ifdef MRHIP_OPAIR_PROBE
    unsigned long long pr_wait = 0, pr_tiles = 0;
    const unsigned long long pr_t0 = clock64(), pr_w0 = wall_clock64();
#endif
    unsigned ring_opts = 0;
    if constexpr (RING) ring_opts = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(ld_sc1(&a.ring_dev->opts))));
    unsigned long long rs_bar = 0, rs_drain = 0;
    const unsigned long long rs_t0 = RING ? wall_clock64() : 0ull;
    bool pend = false;                         // ring mode: a grab whose completion is still to be reported
    int p_stage = 0;
    unsigned p_slot = 0, p_shard = 0, p_cnt = 0, p_nshards = 0, p_seq_lo = 0, p_seq_hi = 0;
    for (int s = 0;; s = (s + 1 == pa.ns ? 0 : s + 1)) {
        // One barrier per tile and no memory wait: the loader arrives only after this tile's data has landed and its
        // descriptor is in LDS; all compute waves arriving proves the oldest stage is no longer read.  The descriptor is fetched
        // by an LDS read (lgkmcnt): the output stores of the tile before stay in flight across the hand-over.
#ifdef MRHIP_OPAIR_PROBE
        const unsigned long long pr_a = clock64();
#endif
        unsigned long long rs_b0 = 0;
        if constexpr (RING) { if (ring_opts & 256u) rs_b0 = wall_clock64(); }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (RING) { if (ring_opts & 256u) rs_bar += wall_clock64() - rs_b0; }
#ifdef MRHIP_OPAIR_PROBE
        pr_wait += clock64() - pr_a;
        ++pr_tiles;
#endif
        int J, remaining;
        R *__restrict__ yc;
        unsigned ring_flags = 0, ring_slot = 0, ring_shard = 0, ring_cnt = 0, ring_nshards = 0, ring_seq_lo = 0, ring_seq_hi = 0;
        if constexpr (RING) {
            const unsigned td = desc_base + kRingTileWords * 4u * static_cast<unsigned>(s);
            unsigned w0[4], w1[4], w2[4];
            desc_get4<0>(td, w0);
            const unsigned tj = w0[0];
            ring_flags = w0[1];
            // the grab that ended with the tile before this one: its write-through stores have had this tile's landing time to drain;
            // the wave of the workgroup that gets here last reports it (the last grab of a chunk raises the host's flag)
            if (pend) {
                pend = false;
                const unsigned long long rs_d0 = (ring_opts & 256u) ? wall_clock64() : 0ull;
                if (!(ring_opts & 16u)) vm_drain();     // (16: experiment -- report without the wait: NOT a valid hand-off)
                if (ring_opts & 256u) rs_drain += wall_clock64() - rs_d0;
                if (lane == 0) {
                    unsigned *const wg_done = reinterpret_cast<unsigned *>(smem + pa.flags_off) + kRingTileWords * pa.ns;
                    const unsigned prev = __hip_atomic_fetch_add(wg_done + p_stage, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (prev + 1u == static_cast<unsigned>(ncw)) {
                        __hip_atomic_store(wg_done + p_stage, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        ring_grab_done(a.ring_dev, a.ring_host, p_slot, (static_cast<unsigned long long>(p_seq_hi) << 32) | p_seq_lo, p_shard, p_cnt, p_nshards);
                    }
                }
            }
            if (tj == 0u) break;                  // the ring is closed and consumed
            if (ring_flags & 2u) continue;        // a FLUSH tile: nothing to compute (the loader had nothing to stage and grabs were unreported)
            J = static_cast<int>(tj);
            desc_get4<16>(td, w1);
            desc_get4<32>(td, w2);
            yc = reinterpret_cast<R *>((static_cast<unsigned long long>(w0[3]) << 32) | w0[2]);
            remaining = static_cast<int>(w1[0]);
            const int u0_t = static_cast<int>(w1[1]);
            ring_slot = w1[2]; ring_shard = w1[3]; ring_seq_lo = w2[0]; ring_seq_hi = w2[1]; ring_cnt = w2[2]; ring_nshards = w2[3];
            if (u0_t != u0) {                     // a chunk that starts elsewhere in the phase cycle: this lane's columns and offsets move
                u0 = u0_t;
                uA = u0 + (act ? 2 * tid : 0) * Mi; uB = uA + Mi;
                qA = uA / Li; phA = uA - qA * Li;
                qB = uB / Li; phB = uB - qB * Li;
                run0 = qA & ~1; offA = qA - run0; dB = qB - run0 - SMIN;
                loff = (static_cast<unsigned>(run0) - static_cast<unsigned>(pa.q0)) * ES;
                gather_taps();
                useA0 = offA == 0; useAT = offA == 1;
                useB0 = dB == 0; useB1 = dB <= 1; useBT = dB >= 1; useBT1 = dB == 2;
                mA0 = lanes_of(useA0); mAT = lanes_of(useAT);
                mB0 = lanes_of(useB0); mB1 = lanes_of(useB1); mBT = lanes_of(useBT); mBT1 = lanes_of(useBT1);
            }
        } else {
            unsigned tg, tj;
            desc_get2(desc_base + 8u * static_cast<unsigned>(s), tg, tj);
            if (tj == 0u) break;                      // end marker
            const TileAt ta = pair_tile_at(pa, tg, tj);
            J = ta.jt;
            yc = static_cast<R *>(a.y) + (static_cast<long long>(ta.ch) * a.y_stride + static_cast<long long>(ta.st) * pa.Sout) * NC;
            remaining = n_out - ta.st * pa.Sout;                          // outputs of this channel from this tile on
        }
        const bool full = remaining >= (J - 1) * pa.Sout + pa.P;          // wave-uniform (steps are Sout outputs apart: P unless the workgroup owns a block of the period)
        const unsigned wbase = lds_base + static_cast<unsigned>(s) * pa.stage_bytes + loff;
        // Which lanes store: a step whose outputs are all inside the channel stores the pairs of mIn.  A tile at a channel's end has at most ONE
        // step that is partly inside (steps are Sout >= P outputs apart): its lanes with both outputs inside, and the one with only its first,
        // are found here, once; the steps behind it store nothing.  In the loop the choice is scalar and the masks go into EXEC as they are.
        unsigned long long mPart2 = 0, mPart1 = 0;
        if constexpr (!RING) {
            if (!full) {
                int rp = remaining;
                while (rp >= pa.P) rp -= pa.Sout;
                const unsigned lim_p = rp > 0 ? static_cast<unsigned>(rp) : 0u;
                mPart2 = lanes_of(my_out + 1 < lim_p);
                mPart1 = lanes_of(my_out < lim_p) & ~mPart2;
            }
        }

        auto run_steps = [&](auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            constexpr int KP = NPR < (NW == 1 ? 5 : 3) ? NPR : (NW == 1 ? 5 : 3);   // ring: 5 pairs of 8 B or 3 pairs of 16 B
            constexpr int NPRV = (NPR + KP - 1) / KP * KP;
            constexpr bool PAIRED_WAITS = KP >= 5;
            pair_t pring[KP];
            char *ybytes = reinterpret_cast<char *>(yc);      // the step's first output: advances on the scalar side (the store's saddr)
            const unsigned wstep = pa.lds_step * ES;
            unsigned wcur = wbase;                            // the ONE window address: this step's run, then -- behind its last read -- the next step's
            unsigned kj = 0;                                  // outputs of the tile in front of this step
            auto read_pair = [&](auto off_tag, unsigned addr) -> pair_t {
                constexpr int OFFP = decltype(off_tag)::value;
                if constexpr (NW == 1) return lds_read_b64<OFFP * 8>(addr);
                else return lds_read_b128<OFFP * 16>(addr);
            };
            static_for<0, KP>([&](auto I) { pring[decltype(I)::value] = read_pair(I, wcur); });
#pragma unroll 1
            for (int j = 0; j < J; ++j) {
                const unsigned wadv = j + 1 < J ? wstep : 0u;  // the last step re-reads its own window (never used)
                R accA[NC] = {}, accB[NC] = {};
                R headA[NC], headB[NC], sumB[NC];                 // masked heads: slot 0's product, B's sum of slots 0 and 1
                static_for<0, NPRV>([&](auto I) {
                    constexpr int r = decltype(I)::value;
                    constexpr int slot = r % KP;
                    if constexpr (r < NPR) {
                        if constexpr (!PAIRED_WAITS) lgkm_wait<ring_younger(r, NPR, KP, 0)>(pring[slot]);
                        else if constexpr (r % 2 == 0) {
                            if constexpr (r + 1 < NPR) lgkm_wait2<ring_younger_pair(r, NPR, KP, 0)>(pring[slot], pring[(r + 1) % KP]);
                            else lgkm_wait<ring_younger(r, NPR, KP, 0)>(pring[slot]);
                        }
                        R wv[2][NC];                          // run samples 2r and 2r+1 (ComplexF64: sample r), widened to the arithmetic type
                        if constexpr (NW == 4) {              // ComplexF64: (re, im) in one 16-byte read
                            wv[0][0] = __hiloint2double(static_cast<int>(pring[slot].y), static_cast<int>(pring[slot].x));
                            wv[0][1] = __hiloint2double(static_cast<int>(pring[slot].w), static_cast<int>(pring[slot].z));
                        } else if constexpr (sizeof(TXS) == 8) {     // Float64 samples: one sample per 8 bytes
                            wv[0][0] = __hiloint2double(static_cast<int>(pring[slot].y), static_cast<int>(pring[slot].x));
                            wv[1][0] = __hiloint2double(static_cast<int>(pring[slot].w), static_cast<int>(pring[slot].z));
                        } else if constexpr (NC == 1) {
                            wv[0][0] = static_cast<R>(__uint_as_float(pring[slot].x)); wv[1][0] = static_cast<R>(__uint_as_float(pring[slot].y));
                        } else {
                            wv[0][0] = static_cast<R>(__uint_as_float(pring[slot].x)); wv[0][1] = static_cast<R>(__uint_as_float(pring[slot].y));
                            wv[1][0] = static_cast<R>(__uint_as_float(pring[slot].z)); wv[1][1] = static_cast<R>(__uint_as_float(pring[slot].w));
                        }
                        static_for<0, SPRD>([&](auto H) {
                            constexpr int js = SPRD * r + decltype(H)::value; // run sample index == A's slot
                            constexpr int jb = js - SMIN;                      // B's slot
                            // slot j of an output is inside the window of a lane with offset d iff d <= j <= d + T - 1: the
                            // lower bound matters for the first slots (j < max offset), the upper one for the last (j > T - 1)
                            constexpr bool a_lo = js < 1, a_hi = js > T - 1;             // A: offsets 0..1
                            constexpr bool b_lo = jb < 2, b_hi = jb > T - 1;             // B: offsets 0..2 (relative to SMIN)
                            constexpr int h = decltype(H)::value;
                            if constexpr (js < NA) {
                                if constexpr (HEADM && js == 0) {
                                    if constexpr (SPRD == 1) masked_mul(headA, tapA[0], wv[h], mA0);   // (else: with slot 1, whose sample came by the same read)
                                } else if constexpr (HEADM && js == 1) {
#pragma unroll
                                    for (int cc = 0; cc < NC; ++cc) accA[cc] = tapA[1] * wv[h][cc];
                                    if constexpr (SPRD == 1) masked_add(accA, headA, mA0);
                                    else masked_mul_add(accA, tapA[0], wv[0], mA0);
                                } else if constexpr (TAILM && a_hi) masked_mac<FUSED>(accA, tapA[js], wv[h], mAT);
                                else {
                                    const bool used = (a_lo ? useA0 : true) && (a_hi ? useAT : true);
#pragma unroll
                                    for (int cc = 0; cc < NC; ++cc) accA[cc] = slot_mac<FUSED, js == 0, a_lo || a_hi, R>(tapA[js], wv[h][cc], accA[cc], used);
                                }
                            }
                            if constexpr (jb >= 0 && jb < NB) {
                                if constexpr (HEADM && jb == 0) masked_mul(headB, tapB[0], wv[h], mB0);
                                else if constexpr (HEADM && jb == 1) masked_mul_then_add(sumB, headB, tapB[1], wv[h], mB1, mB0);
                                else if constexpr (HEADM && jb == 2) {
#pragma unroll
                                    for (int cc = 0; cc < NC; ++cc) accB[cc] = tapB[2] * wv[h][cc];
                                    masked_add(accB, sumB, mB1);
                                } else if constexpr (TAILM && b_hi) masked_mac<FUSED>(accB, tapB[jb], wv[h], jb == T ? mBT : mBT1);
                                else {
                                    const bool used = (b_lo ? (jb == 0 ? useB0 : useB1) : true) && (b_hi ? (jb == T ? useBT : useBT1) : true);
#pragma unroll
                                    for (int cc = 0; cc < NC; ++cc) accB[cc] = slot_mac<FUSED, jb == 0, b_lo || b_hi, R>(tapB[jb], wv[h][cc], accB[cc], used);
                                }
                            }
                        });
                        // pair r is consumed before its slot is re-targeted: whatever holds its products so far is pinned here
                        constexpr int js_l = SPRD * r + SPRD - 1, jb_l = js_l - SMIN;        // the unit's last sample as a slot of A, of B
#pragma unroll
                        for (int cc = 0; cc < NC; ++cc) {
                            if constexpr (HEADM && js_l == 0) pin(headA[cc]); else pin(accA[cc]);
                            if constexpr (HEADM && jb_l == 0) pin(headB[cc]);
                            else if constexpr (HEADM && jb_l == 1) pin(sumB[cc]);
                            else if constexpr (!HEADM || jb_l >= 2) pin(accB[cc]);
                        }
                    }
                    if constexpr (r + KP < NPR) pring[slot] = read_pair(std::integral_constant<int, r + KP>{}, wcur);
                    else if constexpr (r + KP >= NPRV) {
                        if constexpr (r + KP == NPRV) wcur += wadv;   // (this step's last read is issued: r + KP < NPR was false from NPR - KP on)
                        pring[slot] = read_pair(std::integral_constant<int, r + KP - NPRV>{}, wcur);
                    }
                });
                // the lane's two adjacent outputs: one dense 2*ES-byte store per lane, straight from the accumulators
                {
                    char *const dst = ybytes + voff;      // (the ring's stores; the others take ybytes as saddr and voff as voffset: no address register to advance)
                    R v[2 * NC];
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc) { v[cc] = accA[cc]; v[NC + cc] = accB[cc]; }
                    // (ring mode, small chunks: write-through, so that a chunk's completion flag never overtakes its outputs -- every lane its own
                    //  pair; the round's first form paired neighbours into 16-byte stores by the even lanes: MRHIP_RING_OPTS bit 3)
                    // (ring mode: plain stores too, unless the ring runs the write-through protocol -- mrhip_internal.h: RingDev::flush_req)
                    auto put2 = [&]() { if constexpr (RING) { if (ring_nshards >> 31) store_wt<2 * OS>(dst, v); else __builtin_memcpy(dst, v, 2 * OS); } else store_sv<2 * OS>(ybytes, voff, v); };
                    auto put1 = [&]() { if constexpr (RING) { if (ring_nshards >> 31) store_wt<OS>(dst, v); else __builtin_memcpy(dst, v, OS); } else store_sv<OS>(ybytes, voff, v); };
                    bool covered = false;                 // ring, Float32 real: this lane's pair went out with its even neighbour's
                    if constexpr (RING && 2 * OS == 8) {
                        if (!(ring_nshards >> 31)) {
                            // plain stores: the lane's own pair (the L2 merges them; nothing to gain from the neighbour's)
                            covered = true;
                            const unsigned lim_x = FULL ? static_cast<unsigned>(pa.P) : (static_cast<unsigned>(remaining) > kj ? umin(static_cast<unsigned>(remaining) - kj, static_cast<unsigned>(pa.P)) : 0u);
                            if (my_out + 1 < lim_x) __builtin_memcpy(dst, v, 2 * OS);
                            else if (my_out < lim_x) __builtin_memcpy(dst, v, OS);
                        } else if (ring_opts & 8u) {          // (experiment, the round's first form: the EVEN lanes store 16 bytes -- their own pair and the odd
                                                              //  neighbour's, by a quad permute.  Slower than every lane's own 8 bytes since the loader is lean: experiments.md R)
                            unsigned q[4];
                            q[0] = __float_as_uint(v[0]); q[1] = __float_as_uint(v[1]);
                            q[2] = static_cast<unsigned>(__builtin_amdgcn_mov_dpp(static_cast<int>(q[0]), 0xF5, 0xF, 0xF, false));   // quad_perm [1,1,3,3]: lane 2i reads lane 2i + 1
                            q[3] = static_cast<unsigned>(__builtin_amdgcn_mov_dpp(static_cast<int>(q[1]), 0xF5, 0xF, 0xF, false));
                            const unsigned lim_x = FULL ? static_cast<unsigned>(pa.P) : (static_cast<unsigned>(remaining) > kj ? umin(static_cast<unsigned>(remaining) - kj, static_cast<unsigned>(pa.P)) : 0u);
                            const bool even = (static_cast<unsigned>(lane) & 1u) == 0u;
                            // an even lane whose neighbour's pair is inside too stores all four; the neighbour then has nothing to do
                            if (even && my_out + 3 < lim_x) {
                                if (ring_opts & 2048u) {      // (experiment: system scope, the round's first form)
                                    v4u_t qq; __builtin_memcpy(&qq, q, 16);
                                    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(dst), "v"(qq) : "memory");
                                } else store_wt<16>(dst, q);
                                covered = true;
                            }
                            else if (!even && my_out + 1 < lim_x) covered = true;
                        }
                    }
                    if (!covered) {
                        bool in2, in1 = false;            // both outputs inside; only the first
                        if constexpr (RING) {
                            if constexpr (FULL) in2 = my_out + 1 < static_cast<unsigned>(pa.P);
                            else {
                                const unsigned rem_j = static_cast<unsigned>(remaining) > kj ? static_cast<unsigned>(remaining) - kj : 0u;
                                const unsigned lim = rem_j < static_cast<unsigned>(pa.P) ? rem_j : static_cast<unsigned>(pa.P);
                                in2 = my_out + 1 < lim; in1 = my_out < lim;
                            }
                        } else if constexpr (FULL) in2 = __builtin_amdgcn_inverse_ballot_w64(mIn);
                        else {
                            const int rem_j = remaining - static_cast<int>(kj);
                            const bool whole = rem_j >= pa.P, part = rem_j > 0;
                            in2 = __builtin_amdgcn_inverse_ballot_w64(whole ? mIn : part ? mPart2 : 0ull);
                            in1 = __builtin_amdgcn_inverse_ballot_w64(whole || !part ? 0ull : mPart1);
                        }
                        if (in2) put2();
                        else if (in1) put1();
                    }
                    ybytes += static_cast<size_t>(pa.Sout) * OS;
                    kj += static_cast<unsigned>(pa.Sout);
                }
            }
            lgkm_wait<0>(pring[0]);                           // retires the last step's unused reads
            static_for<0, KP>([&](auto I) { pin(pring[decltype(I)::value]); });
        };
        if (full) run_steps(std::true_type{});
        else run_steps(std::false_type{});
        if constexpr (RING) {
            if (ring_flags & 1u) {                // this tile ends a grab: reported at the start of the next tile (see above)
                pend = true; p_stage = s;
                p_slot = ring_slot; p_shard = ring_shard; p_cnt = ring_cnt; p_nshards = ring_nshards; p_seq_lo = ring_seq_lo; p_seq_hi = ring_seq_hi;
                if (ring_opts & 2u) {             // (experiment: at its own end)
                    pend = false;
                    vm_drain();
                    if (lane == 0) {
                        unsigned *const wg_done = reinterpret_cast<unsigned *>(smem + pa.flags_off) + kRingTileWords * pa.ns;
                        const unsigned prev = __hip_atomic_fetch_add(wg_done + p_stage, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (prev + 1u == static_cast<unsigned>(ncw)) {
                            __hip_atomic_store(wg_done + p_stage, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            ring_grab_done(a.ring_dev, a.ring_host, p_slot, (static_cast<unsigned long long>(p_seq_hi) << 32) | p_seq_lo, p_shard, p_cnt, p_nshards);
                        }
                    }
                }
            }
        }
    }
    if constexpr (RING) {
        if ((ring_opts & 256u) && lane == 0) {
            atomicAdd(&a.ring_dev->stats[0], wall_clock64() - rs_t0);
            atomicAdd(&a.ring_dev->stats[1], rs_bar);
            atomicAdd(&a.ring_dev->stats[2], rs_drain);
            atomicAdd(&a.ring_dev->stats[3], 1ull);
        }
    }
#ifdef MRHIP_OPAIR_PROBE
    if (pa.probe && lane == 0) {   // per wave: hardware id, total cycles, cycles at the tile barrier, tiles
        unsigned long long *r = pa.probe + (static_cast<unsigned long long>(blockIdx.x) * 8u + static_cast<unsigned>(wave)) * 4u;
        const unsigned hw = __builtin_amdgcn_s_getreg(0xF804), xcc = __builtin_amdgcn_s_getreg(0xF814);
        r[0] = hw | (static_cast<unsigned long long>(xcc) << 32);
        r[1] = clock64() - pr_t0; r[2] = pr_wait; r[3] = pr_tiles | ((wall_clock64() - pr_w0) << 32);
    }
#endif
}

// (opair_instantiated(fused, smin, T), mrhip_internal.h: which (numerics, M/L class, tapsPerPhi) combinations exist)
template <typename TXS, typename R>
constexpr bool opair_plain_instantiated(bool fused, int nc, int smin, int T)
{
    return !fused && smin <= 1 && (T == 24 || T == 32) && (nc >= 1) && sizeof(TXS) >= 4 && sizeof(R) >= 4;   // (every sample / tap type)
}
// the instantiation of one entry for a launch's mode (0: arguments overridable at entry; NULL: the ring's consumer is not built for it)
template <int T, bool FUSED, int NC, int SMIN, typename TXS, typename R>
PairKernelFn opair_select(int mode)
{
    if constexpr (opair_plain_instantiated<TXS, R>(FUSED, NC, SMIN, T)) {
        if (mode == 1) return rational_opair_kernel<T, FUSED, NC, SMIN, TXS, R, 1>;
        if (mode == 2) return rational_opair_kernel<T, FUSED, NC, SMIN, TXS, R, 2>;
        if (mode == 3) return rational_opair_kernel<T, FUSED, NC, SMIN, TXS, R, 3>;
    } else if (mode == 2) return nullptr;
    return rational_opair_kernel<T, FUSED, NC, SMIN, TXS, R>;
}
template <bool FUSED, int NC, int SMIN, typename TXS, typename R>
hipError_t launch_opair_T(int T, dim3 block, size_t lds, hipStream_t s, const PolyArgs &a, PairArgs pa, int num_cus)
{
    // each entry only selects the instantiation; sizing, debug line and launch: launch_opair_kernel (kernels_rational_opair.hip).
    // PLAIN (the arguments stay in the kernarg segment): MODE 1 for big launches (seam tiles element by element: the DMA variant's
    // loader code costs the headline 1.3 %), MODE 3 for small ones -- a 1e6-sample chunk of one channel -- whose seam tiles are a
    // good part of the launch and go by LDS-DMA; MODE 2: the ring's consumer
    const bool plain = !a.ring_dev && !a.dyn && !a.multi && MRHIP_ENV_INT("MRHIP_OPAIR_PLAIN", 1);
    const int mode = a.ring_dev ? 2 : !plain ? 0 : a.n_out * a.nch >= (1LL << 22) ? 1 : 3;
#define MRHIP_CASE(TT) \
    case TT: if constexpr (opair_instantiated(FUSED, SMIN, TT)) return launch_opair_kernel(opair_select<TT, FUSED, NC, SMIN, TXS, R>(mode), \
        reinterpret_cast<const void *>(rational_opair_kernel<TT, FUSED, NC, SMIN, TXS, R>), block, lds, s, a, pa, num_cus); else break;
#ifdef MRHIP_OPAIR_LONG      // the units that hold 49..64 taps per phase (Float32 samples)
    switch (T) {
#ifdef MRHIP_PS_FAST_BUILD
        MRHIP_CASE(56) MRHIP_CASE(64)
#else
        MRHIP_CASE(49) MRHIP_CASE(50) MRHIP_CASE(51) MRHIP_CASE(52) MRHIP_CASE(53) MRHIP_CASE(54) MRHIP_CASE(55) MRHIP_CASE(56)
        MRHIP_CASE(57) MRHIP_CASE(58) MRHIP_CASE(59) MRHIP_CASE(60) MRHIP_CASE(61) MRHIP_CASE(62) MRHIP_CASE(63) MRHIP_CASE(64)
#endif
    default: break;
    }
#else
    switch (T) {
#ifdef MRHIP_PS_FAST_BUILD
        MRHIP_CASE(24)
#else
        MRHIP_CASE(1) MRHIP_CASE(2) MRHIP_CASE(3) MRHIP_CASE(4) MRHIP_CASE(5) MRHIP_CASE(6) MRHIP_CASE(7) MRHIP_CASE(8)
        MRHIP_CASE(9) MRHIP_CASE(10) MRHIP_CASE(11) MRHIP_CASE(12) MRHIP_CASE(13) MRHIP_CASE(14) MRHIP_CASE(15) MRHIP_CASE(16)
        MRHIP_CASE(17) MRHIP_CASE(18) MRHIP_CASE(19) MRHIP_CASE(20) MRHIP_CASE(21) MRHIP_CASE(22) MRHIP_CASE(23) MRHIP_CASE(24)
        MRHIP_CASE(25) MRHIP_CASE(26) MRHIP_CASE(27) MRHIP_CASE(28) MRHIP_CASE(29) MRHIP_CASE(30) MRHIP_CASE(31) MRHIP_CASE(32)
#endif
    default: break;
    }
    // Float32 arithmetic holds two columns of up to 48 taps in registers (Float64: 32; SMIN >= 2: instantiated up to 32)
    if constexpr ((sizeof(R) == 4 || (NC == 1 && MRHIP_OPAIR_WIDE_LONG)) && SMIN <= 1) {
        switch (T) {
#ifndef MRHIP_PS_FAST_BUILD
        MRHIP_CASE(33) MRHIP_CASE(34) MRHIP_CASE(35) MRHIP_CASE(36) MRHIP_CASE(37) MRHIP_CASE(38) MRHIP_CASE(39) MRHIP_CASE(40)
        MRHIP_CASE(41) MRHIP_CASE(42) MRHIP_CASE(43) MRHIP_CASE(44) MRHIP_CASE(45) MRHIP_CASE(46) MRHIP_CASE(47) MRHIP_CASE(48)
#else
        MRHIP_CASE(36) MRHIP_CASE(48)
#endif
        default: break;
        }
    }
#endif
    return hipErrorInvalidValue;
#undef MRHIP_CASE
}

}  // namespace
}  // namespace mrhip
