// rates_device_updates_check.cpp -- stand-alone program of tests/test_rates_device_updates_cpu.py: the host side of the device-resident
// updates (include/multirate_hip.h, "Device-resident updates for the filters with per-channel rates") on the rows of stdin.
//   map Nphi hLen tap_f64
//        -> the index map of the bank build kernel (csrc/rates_arb.h: rates_bank_tap_index, rates_bank_pfb_value, rates_bank_dpfb_value --
//           the text the kernel compiles) over every element of one channel's banks, against taps2pfb of h and of dh = [diff(h), 0]
//           (csrc/host_logic.cpp: what mrhip_taps2pfb and create_pfb_banks run), byte for byte; answered as
//           T mismatches_pfb mismatches_dpfb zeros_pfb zeros_dpfb
//   range is_rates rates_is_null rate_lo rate_hi
//        -> check_channel_rates_device, answered as
//           status message
//   taps is_rates is_farrow h_is_null hLen tap_dtype filter_hLen filter_tap_dtype            -> check_channel_taps_device
//   pnfb is_rates is_farrow pnfb_is_null tapsPerPhi polyorder filter_T filter_polyorder      -> check_channel_pnfb_device
#include <cstdio>
#include <cstring>
#include <vector>

#include "create.h"
#include "rates_arb.h"

using namespace mrhip;

template <typename TAP>
static void map_row(long long Nphi, long long hLen, int th)
{
    std::vector<TAP> h(static_cast<size_t>(hLen));
    unsigned long long s = 0x9e3779b97f4a7c15ULL + static_cast<unsigned long long>(hLen) * 131 + static_cast<unsigned long long>(Nphi);
    for (TAP &v : h) {                       // taps whose differences round: a full mantissa each, mixed signs and magnitudes
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        const double u = static_cast<double>(s >> 11) / 9007199254740992.0 - 0.5;
        v = static_cast<TAP>(u * (1.0 + static_cast<double>((s >> 7) & 1023)));
    }
    const long long T = taps2pfb(h.data(), hLen, th, Nphi, nullptr);
    const size_t bank = static_cast<size_t>(T * Nphi);
    std::vector<TAP> want_p(bank), want_d(bank), dh(static_cast<size_t>(hLen));
    taps2pfb(h.data(), hLen, th, Nphi, want_p.data());
    arbitrary_dh(h.data(), hLen, th, dh.data());
    taps2pfb(dh.data(), hLen, th, Nphi, want_d.data());
    long long bad_p = 0, bad_d = 0, zero_p = 0, zero_d = 0;
    for (size_t e = 0; e < bank; ++e) {
        const long long j = rates_bank_tap_index(static_cast<long long>(e), T, Nphi);
        const TAP p = rates_bank_pfb_value<TAP>(h.data(), hLen, j), d = rates_bank_dpfb_value<TAP>(h.data(), hLen, j);
        bad_p += std::memcmp(&p, &want_p[e], sizeof(TAP)) != 0;
        bad_d += std::memcmp(&d, &want_d[e], sizeof(TAP)) != 0;
        zero_p += j >= hLen;
        zero_d += j >= hLen - 1;
    }
    std::printf("%lld %lld %lld %lld %lld\n", T, bad_p, bad_d, zero_p, zero_d);
}

int main()
{
    char what[16];
    static const float some_taps[4] = {1.0f, 2.0f, 3.0f, 4.0f};      // (the checks never read them)
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "map")) {
            long long v[3];
            for (int i = 0; i < 3; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
            if (v[2]) map_row<double>(v[0], v[1], MRHIP_F64);
            else map_row<float>(v[0], v[1], MRHIP_F32);
        } else if (!std::strcmp(what, "range")) {
            long long v[2];
            double lo = 0.0, hi = 0.0;
            if (std::scanf("%lld %lld %lf %lf", &v[0], &v[1], &lo, &hi) != 4) { std::fprintf(stderr, "short row\n"); return 2; }
            const Refusal r = check_channel_rates_device(v[0] != 0, v[1] != 0, lo, hi);
            std::printf("%d %s\n", r.status, r.message.c_str());
        } else if (!std::strcmp(what, "taps") || !std::strcmp(what, "pnfb")) {
            long long v[7];
            for (int i = 0; i < 7; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
            const Refusal r = what[0] == 't' ? check_channel_taps_device(v[0] != 0, v[1] != 0, v[2] ? nullptr : some_taps, v[3], static_cast<int>(v[4]), v[5], static_cast<int>(v[6]))
                                             : check_channel_pnfb_device(v[0] != 0, v[1] != 0, v[2] ? nullptr : some_taps, v[3], v[4], v[5], v[6], MRHIP_F32);
            std::printf("%d %s\n", r.status, r.message.c_str());
        } else {
            std::fprintf(stderr, "unknown row %s\n", what);
            return 2;
        }
    }
    return 0;
}
