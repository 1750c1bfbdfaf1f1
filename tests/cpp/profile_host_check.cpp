// profile_host_check.cpp -- gsim_isim and gsim_isim_complement (capi_profile.cpp, host code) on random and malformed inputs: a
// stand-alone program for a sanitizer build (DESIGN.md section 20 has the command line and the result).  It checks the outputs
// against brute-force pair sums of its own (exactly where they fit 53 bits, within 2^-50 on the 128-bit case) and exits non-zero on
// the first difference; the sanitizers report on their own.
#include "../../include/gpusim_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace
{

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

typedef unsigned __int128 u128;

struct Sums {
    u128 a = 0, d = 0, dis = 0;
};

// brute force over all pairs of rows (bits unpacked, one byte each)
Sums pair_sums(const std::vector<std::vector<uint8_t>>& rows, size_t skip)
{
    Sums s;
    for (size_t i = 0; i < rows.size(); i++)
        for (size_t j = i + 1; j < rows.size(); j++) {
            if (i == skip || j == skip) continue;
            for (size_t k = 0; k < rows[i].size(); k++) {
                s.a += rows[i][k] & rows[j][k];
                s.d += (rows[i][k] | rows[j][k]) ^ 1;
                s.dis += rows[i][k] ^ rows[j][k];
            }
        }
    return s;
}

// is `got` the double nearest to num / den, up to the two roundings of the rule (each operand once, then the divide)?  The check is
// that got x den lies within 2^-50 of num, relative: far tighter than any formula error, looser than the rule's three roundings.
bool close_to(double got, u128 num, u128 den)
{
    if (den == 0) return got == 0.0;
    const long double want = static_cast<long double>(num) / static_cast<long double>(den);
    return std::fabs(static_cast<long double>(got) - want) <= want * 0x1p-50L;
}

double expect(const Sums& s, int index) // the rule itself, with the compiler's own conversions (a and d here are far below 2^53: exact)
{
    const u128 num = index == GSIM_ISIM_SIMPLE_MATCHING ? s.a + s.d : s.a;
    const u128 den = index == GSIM_ISIM_TANIMOTO ? s.a + s.dis : s.a + s.d + s.dis;
    return den == 0 ? 0.0 : static_cast<double>(static_cast<uint64_t>(num)) / static_cast<double>(static_cast<uint64_t>(den));
}

} // namespace

int main()
{
    std::mt19937_64 rng(0x1517);
    for (int it = 0; it < 200; it++) {
        const uint32_t fp_bits = 1 + rng() % 200; // (the host functions take any fp_bits > 0)
        const uint64_t n = rng() % 40;
        const double density = it % 3 == 0 ? 0.05 : it % 3 == 1 ? 0.5 : 0.95;
        std::uniform_real_distribution<double> u(0.0, 1.0);
        std::vector<std::vector<uint8_t>> rows(n, std::vector<uint8_t>(fp_bits));
        // exactly the documented lengths: fp_bits counts, m sums / popcounts / outputs
        std::vector<uint64_t> counts(fp_bits, 0), sums(n, 0);
        std::vector<uint32_t> popc(n, 0);
        for (uint64_t i = 0; i < n; i++)
            for (uint32_t k = 0; k < fp_bits; k++) {
                rows[i][k] = u(rng) < density;
                counts[k] += rows[i][k];
                popc[i] += rows[i][k];
            }
        for (uint64_t i = 0; i < n; i++)
            for (uint32_t k = 0; k < fp_bits; k++) sums[i] += rows[i][k] ? counts[k] : 0;
        const Sums all = pair_sums(rows, ~size_t{0});
        for (int index = 0; index < 3; index++) {
            double v = -1.0;
            CHECK(gsim_isim(counts.data(), fp_bits, n, index, &v) == GSIM_OK);
            CHECK(v == expect(all, index));
            std::vector<double> out(n, -1.0);
            CHECK(gsim_isim_complement(counts.data(), fp_bits, n, index, sums.data(), popc.data(), n, n ? out.data() : nullptr) == GSIM_OK);
            for (uint64_t i = 0; i < n; i++) CHECK(out[i] == expect(pair_sums(rows, i), index));
        }
        // malformed: every check must come before any read past the arrays or any write
        double v = 0.0;
        std::vector<double> out(n + 1, 0.0);
        CHECK(gsim_isim(counts.data(), fp_bits, n, 3 + static_cast<int>(rng() % 5), &v) == GSIM_ERR_INVALID);
        CHECK(gsim_isim(counts.data(), 0, n, 0, &v) == GSIM_ERR_INVALID);
        CHECK(gsim_isim(nullptr, fp_bits, n, 0, &v) == GSIM_ERR_INVALID);
        CHECK(gsim_isim(counts.data(), fp_bits, n, 0, nullptr) == GSIM_ERR_INVALID);
        CHECK(gsim_isim(counts.data(), fp_bits, (uint64_t{1} << 32) + rng() % 7, 0, &v) == GSIM_ERR_INVALID);
        std::vector<uint64_t> bad = counts;
        bad[rng() % fp_bits] = n + 1 + rng() % 3;
        CHECK(gsim_isim(bad.data(), fp_bits, n, 0, &v) == GSIM_ERR_INVALID);
        CHECK(gsim_isim_complement(bad.data(), fp_bits, n, 0, sums.data(), popc.data(), n, out.data()) == GSIM_ERR_INVALID);
        if (n > 0) {
            std::vector<uint32_t> bad_popc = popc;
            bad_popc[rng() % n] = fp_bits + 1 + static_cast<uint32_t>(rng() % 3);
            CHECK(gsim_isim_complement(counts.data(), fp_bits, n, 0, sums.data(), bad_popc.data(), n, out.data()) == GSIM_ERR_INVALID);
            std::vector<uint64_t> bad_sums = sums;
            bad_sums[rng() % n] = ~uint64_t{0} - rng() % 3; // a sum no row can have: refused, never wrapped into a value
            CHECK(gsim_isim_complement(counts.data(), fp_bits, n, 0, bad_sums.data(), popc.data(), n, out.data()) == GSIM_ERR_INVALID);
            CHECK(gsim_isim_complement(counts.data(), fp_bits, n, 0, nullptr, popc.data(), n, out.data()) == GSIM_ERR_INVALID);
            CHECK(gsim_isim_complement(counts.data(), fp_bits, n, 0, sums.data(), nullptr, n, out.data()) == GSIM_ERR_INVALID);
            CHECK(gsim_isim_complement(counts.data(), fp_bits, n, 0, sums.data(), popc.data(), n, nullptr) == GSIM_ERR_INVALID);
            CHECK(gsim_isim_complement(counts.data(), fp_bits, 0, 0, sums.data(), popc.data(), n, out.data()) == GSIM_ERR_INVALID);
        }
        CHECK(gsim_isim_complement(counts.data(), fp_bits, n, 0, nullptr, nullptr, 0, nullptr) == GSIM_OK);
    }
    // the 128-bit path: 4096 columns at n = 2^32 - 1, counts near 0, n / 2 and n
    const uint64_t n = 0xFFFFFFFFull;
    std::vector<uint64_t> counts(4096);
    for (uint32_t k = 0; k < 4096; k++) counts[k] = k % 5 == 0 ? 0 : k % 5 == 1 ? 1 : k % 5 == 2 ? n / 2 : k % 5 == 3 ? n - 1 : n;
    u128 a = 0, d = 0, dis = 0;
    for (uint64_t c : counts) {
        a += static_cast<u128>(c) * (c ? c - 1 : 0) / 2;
        d += static_cast<u128>(n - c) * (n - c ? n - c - 1 : 0) / 2;
        dis += static_cast<u128>(c) * (n - c);
    }
    CHECK((a >> 64) != 0 && (d >> 64) != 0);
    double v = 0.0;
    CHECK(gsim_isim(counts.data(), 4096, n, GSIM_ISIM_TANIMOTO, &v) == GSIM_OK && close_to(v, a, a + dis));
    CHECK(gsim_isim(counts.data(), 4096, n, GSIM_ISIM_RUSSELL_RAO, &v) == GSIM_OK && close_to(v, a, a + d + dis));
    CHECK(gsim_isim(counts.data(), 4096, n, GSIM_ISIM_SIMPLE_MATCHING, &v) == GSIM_OK && close_to(v, a + d, a + d + dis));
    // ... and a member row of that set: every column of count >= 1 set
    uint64_t s = 0;
    uint32_t p = 0;
    for (uint64_t c : counts)
        if (c) {
            s += c;
            p++;
        }
    double o = -1.0;
    CHECK(gsim_isim_complement(counts.data(), 4096, n, GSIM_ISIM_TANIMOTO, &s, &p, 1, &o) == GSIM_OK && o > 0.0 && o < 1.0);
    std::printf("profile_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
