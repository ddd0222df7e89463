// create_check.cpp -- stand-alone program of tests/test_create_cpu.py: the constructors' host side (csrc/create.h, csrc/host_logic.cpp)
// on the CPU.  It needs nothing of the library's error state: the checks return their refusal as a value.
//
// Without arguments: the cases of stdin (tests/create_refusal_cases.py: text_row), one a line,
//     id | name h_null out_null hLen th tx nch num den rate nrates r0 r1 Nphi polyorder
// through create_check_args and, where that passes, create_check_params (the device checks between them are the library's); a line each,
//     id | stage status out_cleared | message        stage: "args" or "params" (status 0 there: the constructor would go on)
// With the argument "fit": the merged polynomial fit and the bank building, each against itself one row and one component at a time,
// bit for bit; prints "fit ok" or what differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "create.h"

using namespace mrhip;

namespace {

int check_cases()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t bar = line.find(" | ");
        if (bar == std::string::npos) { std::fprintf(stderr, "bad row: %s\n", line.c_str()); return 2; }
        const std::string id = line.substr(0, bar);
        std::istringstream in(line.substr(bar + 3));
        std::string name, rate, r0, r1;
        long long h_null, out_null, hLen, th, tx, nch, num, den, nrates, Nphi, polyorder;
        if (!(in >> name >> h_null >> out_null >> hLen >> th >> tx >> nch >> num >> den >> rate >> nrates >> r0 >> r1 >> Nphi >> polyorder)) {
            std::fprintf(stderr, "short row: %s\n", line.c_str());
            return 2;
        }
        const CreateEntry &e = create_entry(name);
        const double taps[1] = {0.0};                       // never read: the checks look at the pointer only
        mrhip_filter *cell = reinterpret_cast<mrhip_filter *>(0xdead0);
        const double rates[2] = {std::strtod(r0.c_str(), nullptr), std::strtod(r1.c_str(), nullptr)};
        CreateParams p;
        p.num = num; p.den = den; p.rate = std::strtod(rate.c_str(), nullptr); p.rates = nrates > 0 ? rates : nullptr;
        p.Nphi = Nphi; p.polyorder = polyorder;
        const char *stage = "args";
        Refusal r = create_check_args(e, h_null ? nullptr : taps, hLen, static_cast<int>(th), static_cast<int>(tx), nch, out_null ? nullptr : &cell);
        if (!r) { stage = "params"; r = create_check_params(e, hLen, nch, &p); }
        std::printf("%s | %s %d %d | %s\n", id.c_str(), stage, r.status, out_null || cell == nullptr ? 1 : 0, r.message.c_str());
    }
    return 0;
}

// tap vectors of 8 and of 11 taps (a zero-padded bank) x Nphi = 4 x polyorder 0, 2, 3, in both scalar widths
template <typename S>
int check_fit(int th_real, int th_complex)
{
    int bad = 0;
    for (int hLen : {8, 11})
        for (int P : {0, 2, 3}) {
            const int64_t Nphi = 4;
            const size_t rows = 3, n = rows * static_cast<size_t>(hLen);
            std::vector<S> re(n), im(n), z(2 * n);
            unsigned v = 12345u + static_cast<unsigned>(hLen * 7 + P);
            auto next = [&] { v = v * 1664525u + 1013904223u; return static_cast<S>(static_cast<int>(v >> 8) % 2001 - 1000) / static_cast<S>(257); };
            for (size_t i = 0; i < n; ++i) { re[i] = next(); im[i] = next(); z[2 * i] = re[i]; z[2 * i + 1] = im[i]; }
            std::vector<double> bank_re, bank_im, bank_z, one;
            if (!create_farrow_banks(re.data(), hLen, th_real, Nphi, P, rows, &bank_re) || !create_farrow_banks(im.data(), hLen, th_real, Nphi, P, rows, &bank_im) ||
                !create_farrow_banks(z.data(), hLen, th_complex, Nphi, P, rows, &bank_z)) { std::printf("a fit failed (hLen %d P %d)\n", hLen, P); return 1; }
            const size_t per_row = bank_re.size() / rows;            // T * (P + 1)
            if (bank_z.size() != 2 * bank_re.size() || per_row != static_cast<size_t>((hLen + Nphi - 1) / Nphi) * (P + 1)) { std::printf("sizes\n"); return 1; }
            // a complex vector's coefficients: the real fits of its real and of its imaginary parts
            for (size_t i = 0; i < bank_re.size(); ++i)
                if (std::memcmp(&bank_z[2 * i], &bank_re[i], 8) != 0 || std::memcmp(&bank_z[2 * i + 1], &bank_im[i], 8) != 0) {
                    std::printf("complex fit differs from the component fits at %zu (hLen %d P %d)\n", i, hLen, P);
                    ++bad;
                    break;
                }
            // row r of a bank: the fit of row r alone (real and complex); the same for both filter banks of FIRArbitrary
            for (size_t r = 0; r < rows; ++r) {
                create_farrow_banks(re.data() + r * hLen, hLen, th_real, Nphi, P, 1, &one);
                if (one.size() != per_row || std::memcmp(one.data(), &bank_re[r * per_row], per_row * 8) != 0) { std::printf("real row %zu differs (hLen %d P %d)\n", r, hLen, P); ++bad; }
                create_farrow_banks(z.data() + 2 * r * hLen, hLen, th_complex, Nphi, P, 1, &one);
                if (one.size() != 2 * per_row || std::memcmp(one.data(), &bank_z[2 * r * per_row], 2 * per_row * 8) != 0) { std::printf("complex row %zu differs (hLen %d P %d)\n", r, hLen, P); ++bad; }
            }
            std::vector<unsigned char> pfb, dpfb, pfb1, dpfb1;
            const int64_t T = create_pfb_banks(z.data(), hLen, th_complex, Nphi, rows, &pfb, &dpfb);
            const size_t bank_bytes = static_cast<size_t>(T) * Nphi * 2 * sizeof(S);
            if (pfb.size() != rows * bank_bytes || dpfb.size() != pfb.size()) { std::printf("bank sizes\n"); return 1; }
            for (size_t r = 0; r < rows; ++r) {
                create_pfb_banks(z.data() + 2 * r * hLen, hLen, th_complex, Nphi, 1, &pfb1, &dpfb1);
                if (std::memcmp(pfb1.data(), &pfb[r * bank_bytes], bank_bytes) != 0 || std::memcmp(dpfb1.data(), &dpfb[r * bank_bytes], bank_bytes) != 0) { std::printf("pfb row %zu differs\n", r); ++bad; }
            }
        }
    return bad;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "fit") == 0) {
        const int bad = check_fit<float>(MRHIP_F32, MRHIP_C64) + check_fit<double>(MRHIP_F64, MRHIP_C128);
        if (bad == 0) std::printf("fit ok\n");
        return bad == 0 ? 0 : 1;
    }
    return check_cases();
}
