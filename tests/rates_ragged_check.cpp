// rates_ragged_check.cpp -- stand-alone program of tests/test_rates_ragged_cpu.py, built by the host compiler with
// -fsanitize=address,undefined and linked with csrc/host_logic.cpp (no HIP call is made):
//   * no argument: the pure length checks of mrhip_filt_device_rates_ragged (check_ragged_lengths, csrc/create.h).  A row of stdin is
//         nch x_is_null x_stride lens_is_null len_1 ... len_nch
//     and the answer one line   status | len_max | message   (len_max: -1 where the check refused)
//   * "history": the index rule of the ragged shiftin! (rates_hist_source, csrc/rates_arb.h -- the text the kernels' epilogue runs)
//     against the last H elements of the concatenation [hist ; x[0:len)], for H in {0, 1, 7, 31} and every len in 0 ... 2H+1; also
//     rates_channel_len.  Prints "history ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "create.h"
#include "rates_arb.h"

namespace {
int check_history()
{
    for (int H : {0, 1, 7, 31}) {
        for (long long len = 0; len <= 2 * H + 1; ++len) {
            std::vector<long long> hist(static_cast<size_t>(H)), x(static_cast<size_t>(len)), cat;
            for (int i = 0; i < H; ++i) hist[static_cast<size_t>(i)] = 1000 + i;
            for (long long i = 0; i < len; ++i) x[static_cast<size_t>(i)] = 2000 + i;
            cat = hist;
            cat.insert(cat.end(), x.begin(), x.end());
            for (int i = 0; i < H; ++i) {
                const long long want = cat[cat.size() - static_cast<size_t>(H) + static_cast<size_t>(i)];
                const mrhip::HistSource s = mrhip::RatesHistSource{}(i, len, H);
                if (s.index < 0 || s.index >= (s.from_hist ? H : len)) { std::printf("H %d len %lld i %d: index %lld out of range\n", H, len, i, s.index); return 1; }
                const long long got = s.from_hist ? hist[static_cast<size_t>(s.index)] : x[static_cast<size_t>(s.index)];
                if (got != want) { std::printf("H %d len %lld i %d: got %lld want %lld\n", H, len, i, got, want); return 1; }
                if (len == 0 && !(s.from_hist && s.index == i)) { std::printf("H %d: an empty channel must keep its history\n", H); return 1; }
                if (len >= H && s.from_hist) { std::printf("H %d len %lld: everything comes from x\n", H, len); return 1; }
            }
        }
    }
    const long long lens[3] = {5, 0, 9};
    for (int c = 0; c < 3; ++c)
        if (mrhip::rates_channel_len(lens, 77, c) != lens[c] || mrhip::rates_channel_len(nullptr, 77, c) != 77) { std::printf("rates_channel_len\n"); return 1; }
    std::printf("history ok\n");
    return 0;
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "history") == 0) return check_history();
    for (;;) {
        long long nch = 0, x_null = 0, x_stride = 0, lens_null = 0;
        const int got = std::scanf("%lld %lld %lld %lld", &nch, &x_null, &x_stride, &lens_null);
        if (got <= 0) break;
        if (got != 4 || nch < 1) { std::fprintf(stderr, "bad row\n"); return 2; }
        std::vector<int64_t> lens(static_cast<size_t>(nch));
        for (auto &v : lens) {
            long long t = 0;
            if (std::scanf("%lld", &t) != 1) { std::fprintf(stderr, "bad length\n"); return 2; }
            v = t;
        }
        int64_t len_max = -1;
        const mrhip::Refusal r = mrhip::check_ragged_lengths(lens_null ? nullptr : lens.data(), nch, x_null != 0, x_stride, &len_max);
        std::printf("%d | %lld | %s\n", r.status, static_cast<long long>(r ? -1 : len_max), r.message.c_str());
    }
    return 0;
}
