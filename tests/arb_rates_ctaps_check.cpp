// arb_rates_ctaps_check.cpp -- stand-alone program of tests/test_rates_arb_ctaps_cpu.py: the host side of complex per-channel taps on
// the FIRArbitrary filter with per-channel rates (include/multirate_hip.h, "Complex per-channel taps with per-channel rates for
// FIRArbitrary") on the rows of stdin.
//   plan x_f64 r_f64 complex_x complex_h bank Nphi T n_out nch rate_min num_cus mode
//        -> plan_arb_rates_ctaps_tiled (csrc/host_logic.cpp; the switch value passed in), answered as
//           ok cpl tap_pitch bank_elems x_offset_bytes max_span tile_out tiles_per_channel total_tiles lds      (zeros after ok: refused)
//   ctaps device is_rates is_farrow h_is_null hLen tap_dtype filter_hLen filter_tap_dtype fused
//        -> check_channel_ctaps in the name of mrhip_set_channel_ctaps (device 0) or mrhip_set_channel_ctaps_device (1), answered as
//           status message
//   map Nphi hLen tap_f64
//        -> the pair value functions of the bank build kernel (csrc/rates_arb.h: rates_bank_tap_index, rates_cbank_pfb_value,
//           rates_cbank_dpfb_value -- the text the kernel compiles) over every element of the banks of THREE random complex rows,
//           against create_pfb_banks of the same rows (what mrhip_set_channel_ctaps uploads), byte for byte; answered as
//           T mismatches_pfb mismatches_dpfb zeros_pfb zeros_dpfb
#include <cstdio>
#include <cstring>
#include <vector>

#include "create.h"
#include "rates_arb.h"

using namespace mrhip;

template <typename TAP>
static void map_rows(long long Nphi, long long hLen, int th)
{
    constexpr size_t kRows = 3;
    std::vector<TAP> h(kRows * static_cast<size_t>(hLen) * 2);
    unsigned long long s = 0x9e3779b97f4a7c15ULL + static_cast<unsigned long long>(hLen) * 131 + static_cast<unsigned long long>(Nphi);
    for (TAP &v : h) {                       // components whose differences round: a full mantissa each, mixed signs and magnitudes
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        const double u = static_cast<double>(s >> 11) / 9007199254740992.0 - 0.5;
        v = static_cast<TAP>(u * (1.0 + static_cast<double>((s >> 7) & 1023)));
    }
    std::vector<unsigned char> pfb, dpfb;
    const long long T = create_pfb_banks(h.data(), hLen, th, Nphi, kRows, &pfb, &dpfb);
    const size_t bank = static_cast<size_t>(T * Nphi);
    long long bad_p = 0, bad_d = 0, zero_p = 0, zero_d = 0;
    if (pfb.size() != kRows * bank * 2 * sizeof(TAP) || dpfb.size() != pfb.size()) { std::fprintf(stderr, "bank size\n"); return; }
    for (size_t r = 0; r < kRows; ++r) {
        const TAP *row = h.data() + r * static_cast<size_t>(hLen) * 2;
        for (size_t e = 0; e < bank; ++e) {
            const long long j = rates_bank_tap_index(static_cast<long long>(e), T, Nphi);
            const RatesTapPair<TAP> p = rates_cbank_pfb_value<TAP>(row, hLen, j), d = rates_cbank_dpfb_value<TAP>(row, hLen, j);
            const TAP pv[2] = {p.re, p.im}, dv[2] = {d.re, d.im};
            bad_p += std::memcmp(pv, pfb.data() + (r * bank + e) * 2 * sizeof(TAP), 2 * sizeof(TAP)) != 0;
            bad_d += std::memcmp(dv, dpfb.data() + (r * bank + e) * 2 * sizeof(TAP), 2 * sizeof(TAP)) != 0;
            zero_p += j >= hLen;
            zero_d += j >= hLen - 1;
        }
    }
    std::printf("%lld %lld %lld %lld %lld\n", T, bad_p, bad_d, zero_p, zero_d);
}

int main()
{
    char what[16];
    static const float some_taps[4] = {1.0f, 2.0f, 3.0f, 4.0f};      // (the checks never read them)
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
            const bool ok = plan_arb_rates_ctaps_tiled(tk, a, rate, static_cast<int>(v[10]), static_cast<int>(v[11]), &ta, &lds);
            if (!ok) { ta = ArbTileArgs{}; lds = 0; }
            std::printf("%d %d %d %d %d %d %lld %lld %lld %lld\n", ok ? 1 : 0, ta.cpl, ta.tap_pitch, ta.bank_elems, ta.x_offset_bytes, ta.max_span,
                        static_cast<long long>(ta.tile_out), static_cast<long long>(ta.tiles_per_channel), static_cast<long long>(ta.total_tiles),
                        static_cast<long long>(lds));
        } else if (!std::strcmp(what, "ctaps")) {
            long long v[9];
            for (int i = 0; i < 9; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
            const Refusal r = check_channel_ctaps(v[0] ? "mrhip_set_channel_ctaps_device" : "mrhip_set_channel_ctaps", v[1] != 0, v[2] != 0,
                                                  v[3] ? nullptr : some_taps, v[4], static_cast<int>(v[5]), v[6], static_cast<int>(v[7]), v[8] != 0);
            std::printf("%d %s\n", r.status, r.message.c_str());
        } else if (!std::strcmp(what, "map")) {
            long long v[3];
            for (int i = 0; i < 3; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
            if (v[2]) map_rows<double>(v[0], v[1], MRHIP_C128);
            else map_rows<float>(v[0], v[1], MRHIP_C64);
        } else {
            std::fprintf(stderr, "unknown row %s\n", what);
            return 2;
        }
    }
    return 0;
}
