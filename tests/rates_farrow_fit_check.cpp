// rates_farrow_fit_check.cpp -- stand-alone program of tests/test_rates_farrow_fit_device_cpu.py: the host side of the FIRFarrow fit on the
// device (include/multirate_hip.h, "The FIRFarrow fit on the device for the filters with per-channel rates") on the rows of stdin.
//   fit Nphi polyorder rows
//        -> polyfit_factor (csrc/host_logic.cpp) and polyfit_apply (csrc/rates_arb.h: the text rates_farrow_fit_kernel compiles) against the
//           untouched polyfit_rows, byte for byte, over `rows` right-hand sides of each of four kinds: random Float64; Float32 values
//           widened; rows whose tail is zero (the padding of a bank's first row); one all-zero row among random ones.  polyfit_apply runs
//           twice per row: into an array of its own, and in place with a stride (coef == b, as the kernel calls it).  Answered as
//           factored rows_refused rows_tested mismatches mismatches_in_place
//           (factored 0: polyfit_factor refused; rows_refused: the rows polyfit_rows refused -- all of them or none)
//   map Nphi hLen complex
//        -> the rows the kernel's lanes read (farrow_fit_row_start, 0 past hLen) against taps2pfb of h, Float32 and Float64 taps, byte for
//           byte; answered as
//           T mismatches zeros
//   lanes Nphi hLen polyorder nch complex
//        -> every lane of the kernel restated on the host, Float32 and Float64 taps: the item map, the row load, polyfit_apply in place at
//           the plan's stride, the rounding and the destination index (farrow_fit_item, farrow_fit_dst_index: the text the kernel
//           compiles) into a buffer of nch banks with poisoned guard words on both sides, against create_farrow_banks rounded as
//           install_channel_pnfb rounds; answered as
//           words mismatches not_written_once strays guards_changed
//           (strays: destination indices outside the banks -- not written, counted)
//   plan Nphi                                                                      -> plan_rates_fit: ok lanes lds_bytes
//   taps is_rates is_farrow h_is_null hLen tap_dtype filter_hLen filter_tap_dtype          -> check_channel_taps_farrow_device
//   ctaps is_rates is_farrow h_is_null hLen tap_dtype filter_hLen filter_tap_dtype fused   -> check_channel_ctaps_farrow_device
//        -> status message
#include <cstdio>
#include <cstring>
#include <vector>

#include "create.h"
#include "rates_arb.h"

using namespace mrhip;

static unsigned long long g_seed = 0x9e3779b97f4a7c15ULL;
static double next_value()                   // a full mantissa, mixed signs and magnitudes
{
    g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL;
    const double u = static_cast<double>(g_seed >> 11) / 9007199254740992.0 - 0.5;
    return u * (1.0 + static_cast<double>((g_seed >> 7) & 1023));
}

static void fit_rows(long long n, int polyorder, long long rows)
{
    const int m = polyorder + 1;
    std::vector<double> table;
    const bool factored = polyfit_factor(n, polyorder, &table);
    long long refused = 0, tested = 0, bad = 0, bad_in_place = 0;
    const long long stride = 3;              // (any stride: the kernel's is its lane count)
    std::vector<double> y(static_cast<size_t>(n)), b(static_cast<size_t>(n)), want(static_cast<size_t>(m)), got(static_cast<size_t>(m)),
        col(static_cast<size_t>(n * stride));
    for (int kind = 0; kind < 4; ++kind)
        for (long long row = 0; row < rows; ++row) {
            for (long long r = 0; r < n; ++r) {
                double v = next_value();
                if (kind == 1) v = static_cast<double>(static_cast<float>(v));
                if (kind == 2 && r >= n - 1 - row % n) v = 0.0;         // 1 ... n trailing zeros
                if (kind == 3 && row == rows / 2) v = 0.0;
                y[static_cast<size_t>(r)] = v;
            }
            ++tested;
            if (!polyfit_rows(y.data(), n, polyorder, want.data())) { ++refused; continue; }
            if (!factored) continue;
            b = y;
            polyfit_apply(table.data(), n, m, b.data(), 1, got.data(), 1);
            bad += std::memcmp(got.data(), want.data(), sizeof(double) * static_cast<size_t>(m)) != 0;
            for (long long r = 0; r < n; ++r) col[static_cast<size_t>(r * stride + 1)] = y[static_cast<size_t>(r)];
            polyfit_apply(table.data(), n, m, col.data() + 1, stride, col.data() + 1, stride);
            for (int c = 0; c < m; ++c) got[static_cast<size_t>(c)] = col[static_cast<size_t>(c * stride + 1)];
            bad_in_place += std::memcmp(got.data(), want.data(), sizeof(double) * static_cast<size_t>(m)) != 0;
        }
    std::printf("%d %lld %lld %lld %lld\n", factored ? 1 : 0, refused, tested, bad, bad_in_place);
}

template <typename TAP>
static void map_rows(long long Nphi, long long hLen, int nc, int th, long long *bad, long long *zeros, long long *T_out)
{
    std::vector<TAP> h(static_cast<size_t>(hLen * nc));
    for (TAP &v : h) v = static_cast<TAP>(next_value());
    const long long T = taps2pfb(h.data(), hLen, th, Nphi, nullptr);
    std::vector<TAP> pfb(static_cast<size_t>(T * Nphi * nc));
    taps2pfb(h.data(), hLen, th, Nphi, pfb.data());                      // column-major T x Nphi: element (row i, column phi) at phi*T + i
    for (long long i = 0; i < T; ++i)
        for (int comp = 0; comp < nc; ++comp)
            for (long long phi = 0; phi < Nphi; ++phi) {
                const long long j = farrow_fit_row_start(i, T, Nphi) + phi;
                const TAP v = j < hLen ? h[static_cast<size_t>(j * nc + comp)] : TAP(0);      // the kernel's load
                *bad += std::memcmp(&v, &pfb[static_cast<size_t>((phi * T + i) * nc + comp)], sizeof(TAP)) != 0;
                *zeros += j >= hLen;
            }
    *T_out = T;
}

template <typename TAP>
static void lanes_run(long long Nphi, long long hLen, int polyorder, long long nch, int nc, int th, long long out[5])
{
    const int m = polyorder + 1;
    const long long T = taps2pfb(nullptr, hLen, th, Nphi, nullptr), items = nch * T * nc, words = nch * T * m * nc, guard = 64;
    std::vector<TAP> h(static_cast<size_t>(nch * hLen * nc));
    for (TAP &v : h) v = static_cast<TAP>(next_value());
    std::vector<double> table, want;
    FarrowFitPlan plan{};
    if (!polyfit_factor(Nphi, polyorder, &table) || !plan_rates_fit(Nphi, &plan) ||
        !create_farrow_banks(h.data(), hLen, th, Nphi, polyorder, static_cast<size_t>(nch), &want)) { out[3] += 1; return; }
    if (sizeof(TAP) == 4) for (double &c : want) c = static_cast<double>(static_cast<float>(c));      // install_channel_pnfb
    const double poison = -12345.678;
    std::vector<double> buf(static_cast<size_t>(words + 2 * guard), poison), lds(static_cast<size_t>(plan.lanes * Nphi));
    std::vector<int> written(static_cast<size_t>(words), 0);
    double *pnfb = buf.data() + guard;
    for (long long item = 0; item < items; ++item) {                    // the kernel's loop body, lane by lane
        const long long lane = item % plan.lanes;
        double *b = lds.data() + lane;
        const FarrowFitItem it = farrow_fit_item(item, T, nc);
        const TAP *hc = h.data() + it.c * hLen * nc;
        const long long j0 = farrow_fit_row_start(it.i, T, Nphi);
        for (long long phi = 0; phi < Nphi; ++phi) {
            const long long j = j0 + phi;
            b[phi * plan.lanes] = j < hLen ? static_cast<double>(hc[j * nc + it.comp]) : 0.0;
        }
        polyfit_apply(table.data(), Nphi, m, b, plan.lanes, b, plan.lanes);
        for (int k = 0; k < m; ++k) {
            const double v = b[static_cast<long long>(k) * plan.lanes];
            const long long d = farrow_fit_dst_index(it, k, T, m, nc);
            if (d < 0 || d >= words) { out[3] += 1; continue; }
            pnfb[d] = sizeof(TAP) == 4 ? static_cast<double>(static_cast<float>(v)) : v;
            written[static_cast<size_t>(d)] += 1;
        }
    }
    out[0] += words;
    out[1] += std::memcmp(pnfb, want.data(), sizeof(double) * static_cast<size_t>(words)) != 0 || static_cast<long long>(want.size()) != words;
    for (int w : written) out[2] += w != 1;
    for (long long g = 0; g < guard; ++g) out[4] += (std::memcmp(&buf[static_cast<size_t>(g)], &poison, 8) != 0) + (std::memcmp(&pnfb[words + g], &poison, 8) != 0);
}

int main()
{
    char what[16];
    static const float some_taps[4] = {1.0f, 2.0f, 3.0f, 4.0f};      // (the checks never read them)
    while (std::scanf("%15s", what) == 1) {
        long long v[8] = {};
        const int want = !std::strcmp(what, "fit") || !std::strcmp(what, "map") ? 3 : !std::strcmp(what, "plan") ? 1 : !std::strcmp(what, "lanes") ? 5 : !std::strcmp(what, "taps") ? 7
                         : !std::strcmp(what, "ctaps") ? 8 : -1;
        if (want < 0) { std::fprintf(stderr, "unknown row %s\n", what); return 2; }
        for (int i = 0; i < want; ++i)
            if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "short row\n"); return 2; }
        if (!std::strcmp(what, "fit")) {
            fit_rows(v[0], static_cast<int>(v[1]), v[2]);
        } else if (!std::strcmp(what, "map")) {
            long long bad = 0, zeros = 0, T = 0;
            const int nc = v[2] ? 2 : 1;
            map_rows<float>(v[0], v[1], nc, v[2] ? MRHIP_C64 : MRHIP_F32, &bad, &zeros, &T);
            map_rows<double>(v[0], v[1], nc, v[2] ? MRHIP_C128 : MRHIP_F64, &bad, &zeros, &T);
            std::printf("%lld %lld %lld\n", T, bad, zeros);
        } else if (!std::strcmp(what, "lanes")) {
            long long out[5] = {};
            const int nc = v[4] ? 2 : 1;
            lanes_run<float>(v[0], v[1], static_cast<int>(v[2]), v[3], nc, v[4] ? MRHIP_C64 : MRHIP_F32, out);
            lanes_run<double>(v[0], v[1], static_cast<int>(v[2]), v[3], nc, v[4] ? MRHIP_C128 : MRHIP_F64, out);
            std::printf("%lld %lld %lld %lld %lld\n", out[0], out[1], out[2], out[3], out[4]);
        } else if (!std::strcmp(what, "plan")) {
            FarrowFitPlan p{};
            const bool ok = plan_rates_fit(v[0], &p);
            std::printf("%d %d %zu\n", ok ? 1 : 0, ok ? p.lanes : 0, ok ? p.lds_bytes : static_cast<size_t>(0));
        } else {
            const void *h = v[2] ? nullptr : some_taps;
            const Refusal r = want == 7 ? check_channel_taps_farrow_device(v[0] != 0, v[1] != 0, h, v[3], static_cast<int>(v[4]), v[5], static_cast<int>(v[6]))
                                        : check_channel_ctaps_farrow_device(v[0] != 0, v[1] != 0, h, v[3], static_cast<int>(v[4]), v[5], static_cast<int>(v[6]), v[7] != 0);
            std::printf("%d %s\n", r.status, r.message.c_str());
        }
    }
    return 0;
}
