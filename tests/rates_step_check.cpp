// rates_step_check.cpp -- stand-alone program of tests/test_rates_arb_cpu.py: the serial walk of one channel of a filter with
// per-channel rates (csrc/kernels_rates_arb.hip: rates_schedule_kernel) on the host, over the very step the kernel compiles
// (csrc/sched_step.h: sched_step_nb).  Built by the host compiler with -ffp-contract=off; needs no HIP header.  A row of stdin is
//     Nphi rate nchunks len_1 ... len_nchunks
// and the answer is, per chunk, one line
//     count deficit xIdx acc_bits  n_1 acc_bits_1 ... n_count acc_bits_count
// (the state after the chunk, then the entries; accumulators as the 64 bits of the Float64, in decimal).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sched_step.h"

namespace {
struct Step { double delta, N, invN; };
unsigned long long bits(double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; }

template <bool POW2>
long long walk(const Step &s, double &acc, long long &deficit, long long &xIdx, long long x_len, std::vector<long long> &n, std::vector<double> &a)
{
    n.clear(); a.clear();
    if (x_len < deficit) { deficit -= x_len; return 0; }      // src/Filters.jl:705-709
    long long x = deficit;                                      // :715
    while (x <= x_len) {                                        // :717
        n.push_back(x);
        a.push_back(acc);
        mrhip::sched_step_nb<POW2>(acc, x, s);                  // :731
    }
    xIdx = x;
    deficit = x - x_len;                                        // :734
    return static_cast<long long>(n.size());
}
}  // namespace

int main()
{
    for (;;) {
        long long Nphi = 0, nchunks = 0;
        double rate = 0.0;
        const int got = std::scanf("%lld %lf %lld", &Nphi, &rate, &nchunks);
        if (got <= 0) break;
        if (got != 3 || Nphi < 1 || !(rate > 0.0) || nchunks < 0) { std::fprintf(stderr, "bad row\n"); return 2; }
        const Step s{static_cast<double>(Nphi) / rate, static_cast<double>(Nphi), 1.0 / static_cast<double>(Nphi)};
        const bool pow2 = (Nphi & (Nphi - 1)) == 0;
        double acc = 1.0;                                       // constructor state, :110-115
        long long deficit = 1, xIdx = 1;
        std::vector<long long> n;
        std::vector<double> a;
        for (long long c = 0; c < nchunks; ++c) {
            long long len = 0;
            if (std::scanf("%lld", &len) != 1 || len < 0) { std::fprintf(stderr, "bad chunk\n"); return 2; }
            const long long count = pow2 ? walk<true>(s, acc, deficit, xIdx, len, n, a) : walk<false>(s, acc, deficit, xIdx, len, n, a);
            std::printf("%lld %lld %lld %llu", count, deficit, xIdx, bits(acc));
            for (long long k = 0; k < count; ++k) std::printf(" %lld %llu", n[static_cast<size_t>(k)], bits(a[static_cast<size_t>(k)]));
            std::printf("\n");
        }
    }
    return 0;
}
