// farrow_rates_plan_check.cpp -- stand-alone program of tests/test_rates_farrow_cpu.py: the host side of farrow_rates_multi_kernel
// (csrc/host_logic.cpp: plan_farrow_rates_multi with the switch value passed in, farrow_rates_multi_grid; csrc/rates_arb.h:
// farrow_rates_live_slots, the statement the kernel itself evaluates per lane) on the rows of stdin.  A row is
//     x_f64 r_f64 complex_x complex_h bank T polyorder n_out nch num_cus mode chip_grid grid_fixed count
// and the answer, one line per row, is
//     ok cpl tile_out tiles_per_channel total_tiles grid  then, for the LAST tile of a channel that reaches `count`,  k0 and the number of
//     lanes with 0, 1, ... kFarrowRatesOPL live slots
// (zeros after ok for a refused plan).  The test computes what it expects from the stated formulas.
#include <cstdio>

#include "rates_arb.h"

using namespace mrhip;

int main()
{
    for (;;) {
        long long v[14];
        int got = 0;
        for (int i = 0; i < 14; ++i) got += std::scanf("%lld", &v[i]) == 1;
        if (got == 0) break;
        if (got != 14) { std::fprintf(stderr, "short row\n"); return 2; }
        TypeKey tk{};
        tk.x_f64 = v[0] != 0; tk.r_f64 = v[1] != 0; tk.complex_x = v[2] != 0; tk.complex_h = v[3] != 0; tk.bank = v[4] != 0;
        FarrowArgs a{};
        a.T = static_cast<int>(v[5]); a.polyorder = static_cast<int>(v[6]); a.n_out = v[7]; a.nch = static_cast<int>(v[8]);
        ArbTileArgs ta{};
        const bool ok = plan_farrow_rates_multi(tk, a, static_cast<int>(v[9]), static_cast<int>(v[10]), &ta);
        if (!ok) {
            std::printf("0 0 0 0 0 0 0");
            for (int j = 0; j <= kFarrowRatesOPL; ++j) std::printf(" 0");
            std::printf("\n");
            continue;
        }
        const long long grid = farrow_rates_multi_grid(ta.total_tiles, v[11], static_cast<int>(v[12]));
        const long long count = v[13];
        // the last tile the kernel does not skip (k0 < count), and its lanes by live slots
        long long k0 = 0;
        long long lanes[kFarrowRatesOPL + 1] = {};
        for (long long tau = 0; tau < ta.tiles_per_channel; ++tau)
            if (tau * ta.tile_out < count) k0 = tau * ta.tile_out;
        for (int tid = 0; tid < kVariantThreads; ++tid) lanes[farrow_rates_live_slots(k0, tid, count)] += 1;
        std::printf("1 %d %lld %lld %lld %lld %lld", ta.cpl, static_cast<long long>(ta.tile_out), static_cast<long long>(ta.tiles_per_channel),
                    static_cast<long long>(ta.total_tiles), grid, k0);
        for (int j = 0; j <= kFarrowRatesOPL; ++j) std::printf(" %lld", lanes[j]);
        std::printf("\n");
    }
    return 0;
}
