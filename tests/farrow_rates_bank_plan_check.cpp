// farrow_rates_bank_plan_check.cpp -- stand-alone program of tests/test_rates_bank_farrow_cpu.py: the pure functions behind
// mrhip_set_channel_taps_farrow / mrhip_set_channel_pnfb (csrc/host_logic.cpp) on the rows of stdin.
//   plan x_f64 r_f64 complex_x complex_h bank T polyorder n_out nch num_cus mode chip_grid grid_fixed count
//        -> plan_farrow_rates_multi (the switch value passed in; either bank key), farrow_rates_multi_grid and, for the LAST tile of a channel that
//           reaches `count`, farrow_rates_live_slots (csrc/rates_arb.h: what the kernel evaluates per lane), answered as
//           ok cpl tile_out tiles_per_channel total_tiles grid k0  and the number of lanes with 0, 1, ... kFarrowRatesOPL live slots
//           (zeros after ok: refused)
//   args pnfb_call is_rates is_farrow src_is_null len polyorder tap_dtype filter_len filter_polyorder filter_tap_dtype
//        -> check_channel_taps_farrow, answered as
//           status message
// The test computes what it expects from the plan's stated formulas and from the header's contract.
#include <cstdio>
#include <cstring>

#include "create.h"
#include "rates_arb.h"

using namespace mrhip;

int main()
{
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            long long v[14];
            for (int i = 0; i < 14; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
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
            long long k0 = 0;            // the last tile the kernel does not skip (k0 < count), and its lanes by live slots
            long long lanes[kFarrowRatesOPL + 1] = {};
            for (long long tau = 0; tau < ta.tiles_per_channel; ++tau)
                if (tau * ta.tile_out < count) k0 = tau * ta.tile_out;
            for (int tid = 0; tid < kVariantThreads; ++tid) lanes[farrow_rates_live_slots(k0, tid, count)] += 1;
            std::printf("1 %d %lld %lld %lld %lld %lld", ta.cpl, static_cast<long long>(ta.tile_out), static_cast<long long>(ta.tiles_per_channel),
                        static_cast<long long>(ta.total_tiles), grid, k0);
            for (int j = 0; j <= kFarrowRatesOPL; ++j) std::printf(" %lld", lanes[j]);
            std::printf("\n");
        } else if (!std::strcmp(what, "args")) {
            long long v[10];
            for (int i = 0; i < 10; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
            static const double some_numbers[4] = {1.0, 2.0, 3.0, 4.0};      // (the check never reads them)
            const Refusal r = check_channel_taps_farrow(v[0] != 0, v[1] != 0, v[2] != 0, v[3] ? nullptr : some_numbers, v[4], v[5], static_cast<int>(v[6]),
                                                        v[7], v[8], static_cast<int>(v[9]));
            std::printf("%d %s\n", r.status, r.message.c_str());
        } else {
            std::fprintf(stderr, "unknown row %s\n", what);
            return 2;
        }
    }
    return 0;
}
