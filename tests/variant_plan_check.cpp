// variant_plan_check.cpp -- stand-alone program of tests/test_variant_plans.py: the plans of the LDS-tiled variant kernels
// (csrc/host_logic.cpp: plan_variant_poly_tiled and plan_variant_arb_tiled under the seven families' eligibility functions, the
// switch value passed in) against recorded rows on stdin.  A row is the values of tests/golden/variant_plan_cases.json in its
// column order (column 10, the rate, is a double).  Prints every row that differs; exit status 1 if any did.
#include <cstdio>

#include "mrhip_internal.h"

using namespace mrhip;

int main()
{
    long long rows = 0, bad = 0;
    for (;;) {
        long long v[32];
        double rate = 0.0;
        int got = 0;
        for (int i = 0; i < 32; ++i) got += i == 10 ? std::scanf("%lf", &rate) == 1 : std::scanf("%lld", &v[i]) == 1;
        if (got == 0) break;
        if (got != 32) { std::fprintf(stderr, "short row %lld\n", rows); return 2; }
        ++rows;
        const int fn = static_cast<int>(v[0]), num_cus = static_cast<int>(v[11]), mode = static_cast<int>(v[12]);
        TypeKey tk{};
        tk.x_f64 = v[1] != 0; tk.r_f64 = v[2] != 0; tk.complex_x = v[3] != 0;
        tk.complex_h = fn == 0 || fn == 2 || fn == 3 || fn == 6;
        tk.bank = fn == 1 || fn == 2 || fn == 4 || fn == 5;
        ArbTileArgs ta{};
        size_t lds = 0;
        bool ok = false;
        if (fn <= 2) {
            PolyArgs a{};
            a.L = static_cast<int>(v[4]); a.M = static_cast<int>(v[5]); a.T = static_cast<int>(v[6]); a.n_out = v[8]; a.nch = static_cast<int>(v[9]);
            ok = fn == 0 ? plan_ctaps_tiled(tk, a, num_cus, mode, &ta, &lds) : fn == 1 ? plan_bank_tiled(tk, a, num_cus, mode, &ta, &lds)
                                                                                       : plan_bank_ctaps_tiled(tk, a, num_cus, mode, &ta, &lds);
        } else if (fn <= 4) {
            ArbArgs a{};
            a.Nphi = static_cast<int>(v[4]); a.T = static_cast<int>(v[6]); a.n_out = v[8]; a.nch = static_cast<int>(v[9]);
            const int min_work = v[13] ? static_cast<int>(v[14]) : kCtapsArbTiledMinDefault;
            ok = fn == 3 ? plan_ctaps_arb_tiled(tk, a, rate, num_cus, mode, min_work, &ta, &lds) : plan_arb_bank_tiled(tk, a, rate, num_cus, mode, &ta, &lds);
        } else {
            FarrowArgs a{};
            a.T = static_cast<int>(v[6]); a.polyorder = static_cast<int>(v[7]); a.n_out = v[8]; a.nch = static_cast<int>(v[9]);
            const int min_out = v[13] ? static_cast<int>(v[14]) : kCtapsFarrowTiledMinDefault;
            ok = fn == 5 ? plan_farrow_bank_tiled(tk, a, rate, num_cus, mode, &ta, &lds) : plan_ctaps_farrow_tiled(tk, a, rate, num_cus, mode, min_out, &ta, &lds);
        }
        if (!ok) { ta = ArbTileArgs{}; lds = 0; }      // (a refused plan leaves nothing to compare)
        const long long have[17] = {ok, ta.cpl, ta.tap_pitch, ta.bank_elems, ta.x_offset_bytes, ta.max_span, ta.prefetch, ta.copyb_pad, ta.pipe, ta.row_pitch,
                                    ta.dma_slots, ta.tile_out, ta.tiles_per_channel, ta.total_tiles, ta.counters != nullptr, ta.run_tiles,
                                    static_cast<long long>(lds)};
        bool same = true;
        for (int i = 0; i < 17; ++i) same = same && have[i] == v[15 + i];
        if (!same) {
            ++bad;
            std::printf("row %lld (fn %d):", rows, fn);
            for (int i = 0; i < 17; ++i) std::printf(" %lld", have[i]);
            std::printf("\n");
        }
    }
    std::printf("rows %lld differing %lld\n", rows, bad);
    return bad != 0;
}
