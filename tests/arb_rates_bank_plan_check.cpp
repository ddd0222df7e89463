// arb_rates_bank_plan_check.cpp -- stand-alone program of tests/test_rates_bank_arb_cpu.py: the two pure functions behind
// mrhip_set_channel_taps (csrc/host_logic.cpp) on the rows of stdin.
//   plan x_f64 r_f64 complex_x complex_h bank Nphi T n_out nch rate_min num_cus mode
//        -> plan_arb_rates_tiled (the switch value passed in; either bank key), answered as
//           ok cpl tap_pitch bank_elems x_offset_bytes max_span tile_out tiles_per_channel total_tiles lds      (zeros after ok: refused)
//   taps is_rates is_farrow h_is_null hLen tap_dtype filter_hLen filter_tap_dtype
//        -> check_channel_taps, answered as
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
            long long v[12];
            double rate = 0.0;
            int got = 0;
            for (int i = 0; i < 12; ++i) got += i == 9 ? std::scanf("%lf", &rate) == 1 : std::scanf("%lld", &v[i]) == 1;
            if (got != 12) { std::fprintf(stderr, "short row\n"); return 2; }
            TypeKey tk{};
            tk.x_f64 = v[0] != 0; tk.r_f64 = v[1] != 0; tk.complex_x = v[2] != 0; tk.complex_h = v[3] != 0; tk.bank = v[4] != 0;
            ArbArgs a{};
            a.Nphi = static_cast<int>(v[5]); a.T = static_cast<int>(v[6]); a.n_out = v[7]; a.nch = static_cast<int>(v[8]);
            ArbTileArgs ta{};
            size_t lds = 0;
            const bool ok = plan_arb_rates_tiled(tk, a, rate, static_cast<int>(v[10]), static_cast<int>(v[11]), &ta, &lds);
            if (!ok) { ta = ArbTileArgs{}; lds = 0; }
            std::printf("%d %d %d %d %d %d %lld %lld %lld %lld\n", ok ? 1 : 0, ta.cpl, ta.tap_pitch, ta.bank_elems, ta.x_offset_bytes, ta.max_span,
                        static_cast<long long>(ta.tile_out), static_cast<long long>(ta.tiles_per_channel), static_cast<long long>(ta.total_tiles),
                        static_cast<long long>(lds));
        } else if (!std::strcmp(what, "taps")) {
            long long v[7];
            for (int i = 0; i < 7; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
            static const float some_taps[4] = {1.0f, 2.0f, 3.0f, 4.0f};      // (the check never reads them)
            const Refusal r = check_channel_taps(v[0] != 0, v[1] != 0, v[2] ? nullptr : some_taps, v[3], static_cast<int>(v[4]), v[5], static_cast<int>(v[6]));
            std::printf("%d %s\n", r.status, r.message.c_str());
        } else {
            std::fprintf(stderr, "unknown row %s\n", what);
            return 2;
        }
    }
    return 0;
}
