// launch_grid_check.cpp -- stand-alone program of tests/test_launch_grid.py: the launchers' grid arithmetic (csrc/host_logic.cpp:
// pair_grid, opair_six_wave_cap, persistent_grid_size) against recorded rows on stdin.  A row is "P" or "G" and the integers of
// tests/golden/launch_grid_cases.json in its column order.  Prints every row that differs; exit status 1 if any did.
#include <cstdio>

#include "mrhip_internal.h"

using namespace mrhip;

int main()
{
    long long rows = 0, bad = 0;
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        long long v[15];
        const int n = kind == 'P' ? 15 : 7;
        for (int i = 0; i < n; ++i)
            if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row %lld\n", rows); return 2; }
        ++rows;
        if (kind == 'P') {
            // the composition of the call sites (launch_opair_kernel, launch_stream_kernel): occupancy -> [six-wave cap] -> bpc -> pair_grid
            int per_cu = static_cast<int>(v[1]);
            const int num_cus = static_cast<int>(v[2]), J = static_cast<int>(v[4]), bpc = static_cast<int>(v[9]);
            const unsigned total_steps = static_cast<unsigned>(v[3]);
            if (v[0] == 0) per_cu = opair_six_wave_cap(per_cu, num_cus, total_steps, J, static_cast<unsigned>(v[6]));
            else if (per_cu < 1) per_cu = 1;
            if (bpc > 0) per_cu = bpc;
            const PairGrid g = pair_grid(per_cu, num_cus, total_steps, J, kPairGroups, static_cast<int>(v[5]), v[7] != 0, static_cast<int>(v[8]));
            if (per_cu != v[10] || g.grid != v[11] || g.ngroups != v[12] || g.steps_per_group != v[13] || g.static_grabs != v[14]) {
                ++bad;
                std::printf("pair row %lld: per_cu %d grid %lld ngroups %d steps_per_group %u static_grabs %d\n", rows, per_cu, g.grid, g.ngroups,
                            g.steps_per_group, g.static_grabs);
            }
        } else {
            int per_cu = static_cast<int>(v[1]);
            const long long g = persistent_grid_size(&per_cu, static_cast<int>(v[2]), v[3], static_cast<int>(v[4]), v[0] == 0);
            if (per_cu != v[5] || g != v[6]) { ++bad; std::printf("persistent row %lld: per_cu %d grid %lld\n", rows, per_cu, g); }
        }
    }
    std::printf("rows %lld differing %lld\n", rows, bad);
    return bad != 0;
}
