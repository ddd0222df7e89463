// farrow_rates_ctaps_check.cpp -- stand-alone program of tests/test_rates_farrow_ctaps_cpu.py: the host side of complex per-channel taps
// on the FIRFarrow filter with per-channel rates (include/multirate_hip.h, "Complex per-channel taps with per-channel rates for
// FIRFarrow") on the rows of stdin.
//   plan x_f64 r_f64 complex_x complex_h bank T polyorder n_out nch num_cus mode
//        -> plan_farrow_rates_ctaps_multi (csrc/host_logic.cpp; the switch value passed in), answered as
//           ok cpl tile_out tiles_per_channel total_tiles                                                    (zeros after ok: refused)
//   live k0 tid count
//        -> farrow_rates_ctaps_live_slots (csrc/rates_arb.h -- the text the multi kernel compiles), answered as the slot count
//   grid total_tiles chip_grid grid_fixed
//        -> farrow_rates_multi_grid, answered as the grid
//   check which is_rates is_farrow src_is_null len polyorder tap_dtype filter_len filter_polyorder filter_tap_dtype fused
//        -> check_channel_ctaps_farrow in the name of mrhip_set_channel_ctaps_farrow (which 0: len is hLen), mrhip_set_channel_pnfb_ctaps
//           (1) or mrhip_set_channel_pnfb_ctaps_device (2; both: len is tapsPerPhi), answered as
//           status message
//   banks Nphi hLen polyorder tap_f64
//        -> create_farrow_banks over THREE random complex rows at once (what mrhip_set_channel_ctaps_farrow installs) against the same
//           function over each row alone (the bank of mrhip_create_farrow_ctaps(h_c, ...)), and the real and imaginary parts of bank c
//           against the fits of real(h_c) and imag(h_c) (the fit is per component), byte for byte; answered as
//           T ok mismatches_rows mismatches_components
#include <cstdio>
#include <cstring>
#include <vector>

#include "create.h"
#include "rates_arb.h"

using namespace mrhip;

template <typename TAP>
static void bank_rows(long long Nphi, long long hLen, long long P, int th_complex, int th_real)
{
    constexpr size_t kRows = 3;
    std::vector<TAP> h(kRows * static_cast<size_t>(hLen) * 2);
    unsigned long long s = 0x9e3779b97f4a7c15ULL + static_cast<unsigned long long>(hLen) * 131 + static_cast<unsigned long long>(Nphi);
    for (TAP &v : h) {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        const double u = static_cast<double>(s >> 11) / 9007199254740992.0 - 0.5;
        v = static_cast<TAP>(u * (1.0 + static_cast<double>((s >> 7) & 1023)));
    }
    const long long T = (hLen + Nphi - 1) / Nphi;
    const size_t np = static_cast<size_t>(P + 1), bank = static_cast<size_t>(T) * np * 2;
    std::vector<double> all;
    const bool ok = create_farrow_banks(h.data(), hLen, th_complex, Nphi, P, kRows, &all);
    long long bad_rows = 0, bad_comp = 0;
    if (ok && all.size() != kRows * bank) { std::fprintf(stderr, "bank size\n"); return; }
    for (size_t r = 0; ok && r < kRows; ++r) {
        const TAP *row = h.data() + r * static_cast<size_t>(hLen) * 2;
        std::vector<double> one;
        if (!create_farrow_banks(row, hLen, th_complex, Nphi, P, 1, &one) || one.size() != bank) { ++bad_rows; continue; }
        bad_rows += std::memcmp(one.data(), all.data() + r * bank, bank * sizeof(double)) != 0;
        for (int comp = 0; comp < 2; ++comp) {
            std::vector<TAP> part(static_cast<size_t>(hLen));
            for (long long j = 0; j < hLen; ++j) part[static_cast<size_t>(j)] = row[2 * j + comp];
            std::vector<double> fit;
            if (!create_farrow_banks(part.data(), hLen, th_real, Nphi, P, 1, &fit) || fit.size() * 2 != bank) { ++bad_comp; continue; }
            for (size_t e = 0; e < fit.size(); ++e) bad_comp += std::memcmp(&fit[e], &all[r * bank + 2 * e + comp], sizeof(double)) != 0;
        }
    }
    std::printf("%lld %d %lld %lld\n", T, ok ? 1 : 0, bad_rows, bad_comp);
}

int main()
{
    char what[16];
    static const double some_values[4] = {1.0, 2.0, 3.0, 4.0};      // (the checks never read them)
    static const char *const names[3] = {"mrhip_set_channel_ctaps_farrow", "mrhip_set_channel_pnfb_ctaps", "mrhip_set_channel_pnfb_ctaps_device"};
    while (std::scanf("%15s", what) == 1) {
        long long v[11];
        auto read = [&](int n) {
            for (int i = 0; i < n; ++i)
                if (std::scanf("%lld", &v[i]) != 1) return false;
            return true;
        };
        if (!std::strcmp(what, "plan")) {
            if (!read(11)) { std::fprintf(stderr, "short row\n"); return 2; }
            TypeKey tk{};
            tk.x_f64 = v[0] != 0; tk.r_f64 = v[1] != 0; tk.complex_x = v[2] != 0; tk.complex_h = v[3] != 0; tk.bank = v[4] != 0;
            FarrowArgs a{};
            a.T = static_cast<int>(v[5]); a.polyorder = static_cast<int>(v[6]); a.n_out = v[7]; a.nch = static_cast<int>(v[8]);
            ArbTileArgs ta{};
            const bool ok = plan_farrow_rates_ctaps_multi(tk, a, static_cast<int>(v[9]), static_cast<int>(v[10]), &ta);
            if (!ok) ta = ArbTileArgs{};
            std::printf("%d %d %lld %lld %lld\n", ok ? 1 : 0, ta.cpl, static_cast<long long>(ta.tile_out), static_cast<long long>(ta.tiles_per_channel),
                        static_cast<long long>(ta.total_tiles));
        } else if (!std::strcmp(what, "live")) {
            if (!read(3)) { std::fprintf(stderr, "short row\n"); return 2; }
            std::printf("%d\n", farrow_rates_ctaps_live_slots(v[0], static_cast<int>(v[1]), v[2]));
        } else if (!std::strcmp(what, "grid")) {
            if (!read(3)) { std::fprintf(stderr, "short row\n"); return 2; }
            std::printf("%lld\n", farrow_rates_multi_grid(v[0], v[1], static_cast<int>(v[2])));
        } else if (!std::strcmp(what, "check")) {
            if (!read(11) || v[0] < 0 || v[0] > 2) { std::fprintf(stderr, "short row\n"); return 2; }
            const Refusal r = check_channel_ctaps_farrow(names[v[0]], v[0] != 0, v[1] != 0, v[2] != 0, v[3] ? nullptr : some_values, v[4], v[5],
                                                         static_cast<int>(v[6]), v[7], v[8], static_cast<int>(v[9]), v[10] != 0);
            std::printf("%d %s\n", r.status, r.message.c_str());
        } else if (!std::strcmp(what, "banks")) {
            if (!read(4)) { std::fprintf(stderr, "short row\n"); return 2; }
            if (v[3]) bank_rows<double>(v[0], v[1], v[2], MRHIP_C128, MRHIP_F64);
            else bank_rows<float>(v[0], v[1], v[2], MRHIP_C64, MRHIP_F32);
        } else {
            std::fprintf(stderr, "unknown row %s\n", what);
            return 2;
        }
    }
    return 0;
}
