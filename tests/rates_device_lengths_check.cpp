// rates_device_lengths_check.cpp -- stand-alone program of tests/test_rates_device_lengths_cpu.py, built by the host compiler with
// -fsanitize=address,undefined and linked with csrc/host_logic.cpp (no HIP call is made):
//   * "lengths": the pure checks both calls share (check_device_lengths, csrc/create.h).  A row of stdin is
//         who lens_is_null len_max x_is_null nch x_stride          (who: 0 mrhip_filt_device_rates_lens_device, 1 ..._rates_chained)
//     and the answer one line   status | message
//   * "chain": what mrhip_filt_device_rates_chained refuses about the pair (check_rates_chain).  A row of stdin is
//         f_is_rates same_filter prev_is_rates f_nch prev_nch f_device prev_device f_tx prev_ty prev_called prev_dev_planned
//     and the answer one line   status | message
//   * "accept": the acceptance rule the import kernel compiles (rates_length_accepted, csrc/rates_arb.h).  A row of stdin is
//         value len_max      and the answer one line: 1 accepted, 0 refused
//     After the rows the program runs the kernel's statement for every source over the rows read -- the accepted length or 0 into the
//     array of lengths, the mark into the record -- against arrays of exactly nch elements, and prints "import ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "create.h"
#include "rates_arb.h"

namespace {
// the statement of rates_lens_set_kernel for lane c, on host memory
void import_lane(const mrhip::RatesLensArgs &a, int c)
{
    const long long l = a.source == mrhip::kRatesLensCaller ? a.src[c] : a.source == mrhip::kRatesLensRecords ? a.prev_rec[c].count : a.prev_call->n_out;
    const bool ok = mrhip::rates_length_accepted(l, a.len_max);
    a.x_lens[c] = ok ? l : 0;
    if (!ok) a.rec[c].len_refused = 1;
}

int check_accept()
{
    std::vector<long long> values;
    long long len_max = -1;
    for (;;) {
        long long v = 0, m = 0;
        const int got = std::scanf("%lld %lld", &v, &m);
        if (got <= 0) break;
        if (got != 2) { std::fprintf(stderr, "bad row\n"); return 2; }
        std::printf("%d\n", mrhip::rates_length_accepted(v, m) ? 1 : 0);
        if (len_max >= 0 && m != len_max) continue;      // (the import below runs over the rows of the first maximum)
        len_max = m;
        values.push_back(v);
    }
    const int nch = static_cast<int>(values.size());
    if (nch == 0) return 0;
    for (int source : {mrhip::kRatesLensCaller, mrhip::kRatesLensRecords, mrhip::kRatesLensCall}) {
        std::vector<mrhip::RateChannel> rec(static_cast<size_t>(nch)), prev(static_cast<size_t>(nch));
        std::vector<long long> lens(static_cast<size_t>(nch), -7);
        mrhip::DevCall call{};
        for (int c = 0; c < nch; ++c) {
            rec[static_cast<size_t>(c)] = mrhip::RateChannel{2.0, 16.0, 1.0 + c, 1 + c, 1, 5, 0, 0};
            prev[static_cast<size_t>(c)].count = values[static_cast<size_t>(c)];
        }
        for (int pass = 0; pass < (source == mrhip::kRatesLensCall ? nch : 1); ++pass) {
            call.n_out = values[static_cast<size_t>(pass)];
            mrhip::RatesLensArgs a{};
            a.rec = rec.data(); a.x_lens = lens.data(); a.src = values.data(); a.prev_rec = prev.data(); a.prev_call = &call;
            a.len_max = len_max; a.nch = nch; a.source = source;
            for (auto &r : rec) r.len_refused = 0;
            for (int c = 0; c < nch; ++c) import_lane(a, c);
            for (int c = 0; c < nch; ++c) {
                const long long v = source == mrhip::kRatesLensCall ? call.n_out : values[static_cast<size_t>(c)];
                const bool ok = v >= 0 && v <= len_max;
                const mrhip::RateChannel &r = rec[static_cast<size_t>(c)];
                if (lens[static_cast<size_t>(c)] != (ok ? v : 0) || r.len_refused != (ok ? 0 : 1)) { std::printf("source %d channel %d: length or mark\n", source, c); return 1; }
                if (r.rate != 2.0 || r.delta != 16.0 || r.acc != 1.0 + c || r.inputDeficit != 1 + c || r.xIdx != 1 || r.count != 5 || r.error != 0) {
                    std::printf("source %d channel %d: the import touched the record\n", source, c);
                    return 1;
                }
            }
        }
    }
    std::printf("import ok\n");
    return 0;
}
}  // namespace

int main(int argc, char **argv)
{
    static_assert(sizeof(mrhip::RateChannel) == 64, "the record keeps its size");
    if (argc < 2) { std::fprintf(stderr, "lengths | chain | accept\n"); return 2; }
    if (std::strcmp(argv[1], "accept") == 0) return check_accept();
    const bool chain = std::strcmp(argv[1], "chain") == 0;
    for (;;) {
        long long v[11] = {};
        const int want = chain ? 11 : 6;
        int got = 0;
        for (; got < want; ++got)
            if (std::scanf("%lld", &v[got]) != 1) break;
        if (got == 0) break;
        if (got != want) { std::fprintf(stderr, "bad row\n"); return 2; }
        const mrhip::Refusal r = chain ? mrhip::check_rates_chain(v[0] != 0, v[1] != 0, v[2] != 0, v[3], v[4], static_cast<int>(v[5]), static_cast<int>(v[6]),
                                                                  static_cast<int>(v[7]), static_cast<int>(v[8]), v[9] != 0, v[10] != 0)
                                       : mrhip::check_device_lengths(v[0] ? "mrhip_filt_device_rates_chained" : "mrhip_filt_device_rates_lens_device",
                                                                     v[1] != 0, v[2], v[3] != 0, v[4], v[5]);
        std::printf("%d | %s\n", r.status, r.message.c_str());
    }
    return 0;
}
