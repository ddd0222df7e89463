// sched_step.h -- ONE update() of FIRArbitrary / FIRFarrow (src/Filters.jl:663-673), the branch-free form: the text that
// kernels_schedule.hip (the 64-step runs of its tables and emit kernels), kernels_rates_arb.hip (the serial walk of one channel a lane)
// and tests/rates_step_check.cpp (the host compiler, against the oracle's schedule) all compile.  Nothing but this function lives
// here, so that the host program needs no HIP header.  Every including unit is compiled with -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define MRHIP_SCHED_STEP_HD __host__ __device__ __forceinline__
#else
#define MRHIP_SCHED_STEP_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mrhip {

// One update() of the reference in a form whose every operation is exact except the one the reference rounds too (the sum):
// mod(a1-1, N) == (a1-1) - k*N with k = floor(fl((a1-1)/N)), minus one more N when the rounded quotient overshot an integer (possible
// for N that is not a power of two; the reference's xIdx step keeps that overshoot, Filters.jl:667, and so does `x` here).  k*N <= a1
// < 2^53 is an integer: exact; the difference is a multiple of ulp(a1) no larger than a1: exact.  Without a branch: the same operations
// on the same values in the same order as the branching form (sched_step, kernels_schedule.hip) -- the results of the path not taken are
// discarded -- and k, an integer below 2^31 (make_sched_plan: below 2^18 + 1; mrhip_create_arbitrary_rates: 1/rate below 2^30), goes
// through Int32 (a Float64 -> Int64 conversion is five instructions on gfx950).
// Plan: anything with the Float64 members delta (N𝜙/rate), N (N𝜙) and invN (1/N𝜙, exact when POW2).
template <bool POW2, typename Plan>
MRHIP_SCHED_STEP_HD void sched_step_nb(double &acc, long long &x, const Plan &c)
{
    const double a1 = acc + c.delta;                                  // :664
    const double am1 = a1 - 1.0;
    const double q = POW2 ? am1 * c.invN : am1 / c.N;                 // :667
    const double k = __builtin_floor(q);
    double r = am1 - k * c.N;
    // (a power of two: the scaling, the floor, k * N and the difference are all exact -- r is am1 mod N, never negative; only a ROUNDED
    //  quotient can overshoot an integer)
    if constexpr (!POW2) r = r < 0.0 ? r + c.N : r;
    const bool wrap = a1 > c.N;                                       // :666
    acc = wrap ? r + 1.0 : a1;                                        // :668
    x += wrap ? static_cast<long long>(static_cast<int>(k)) : 0LL;
}

}  // namespace mrhip
