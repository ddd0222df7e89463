// arb_rates_plan_check.cpp -- stand-alone program of tests/test_rates_arb_cpu.py: plan_arb_rates_tiled (csrc/host_logic.cpp, the
// switch value passed in) on the rows of stdin.  A row is
//     x_f64 r_f64 complex_x complex_h bank Nphi T n_out nch rate_min num_cus mode
// and the answer, one line per row, is
//     ok cpl tap_pitch bank_elems x_offset_bytes max_span tile_out tiles_per_channel total_tiles lds
// (zeros after ok for a refused plan).  The test computes what it expects from the plan's stated formulas.
#include <cstdio>

#include "rates_arb.h"

using namespace mrhip;

int main()
{
    for (;;) {
        long long v[12];
        double rate = 0.0;
        int got = 0;
        for (int i = 0; i < 12; ++i) got += i == 9 ? std::scanf("%lf", &rate) == 1 : std::scanf("%lld", &v[i]) == 1;
        if (got == 0) break;
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
    }
    return 0;
}
