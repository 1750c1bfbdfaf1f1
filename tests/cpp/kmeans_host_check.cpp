// kmeans_host_check.cpp -- gsim_label_centroids (capi_labels.cpp, host code) on random and malformed inputs: a stand-alone program,
// built plainly by tests/test_kmeans_host.py and once by hand for a sanitizer build (DESIGN.md section 21 has the command line and
// the result).  Arrays have exactly the documented lengths, so that a read or write past them is the sanitizer's to report; the
// outputs are checked against a bit-by-bit restatement of the rule and the program exits non-zero on the first difference.
#include "../../include/gpusim_hip.h"

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

void one_case(std::mt19937& rng, uint32_t nlabels, uint32_t fp_bits, bool with_previous)
{
    const uint32_t W = fp_bits / 32;
    std::vector<uint32_t> sizes(nlabels), counts(static_cast<size_t>(nlabels) * fp_bits), previous(static_cast<size_t>(nlabels) * W),
        centres(static_cast<size_t>(nlabels) * W, 0xDEADBEEFu);
    for (uint32_t l = 0; l < nlabels; l++) {
        const uint32_t kinds[] = {0u, 1u, 2u, 3u, 4u, 7u, 1000u, 0xFFFFFFFFu, 0x80000000u};
        sizes[l] = kinds[rng() % 9];
        for (uint32_t k = 0; k < fp_bits; k++) {
            const uint32_t n = sizes[l];
            uint32_t c;
            switch (rng() % 5) {
            case 0: c = 0; break;
            case 1: c = n; break;
            case 2: c = n / 2; break;                // 2c == n for an even n (the tie sets the bit), 2c == n - 1 for an odd one
            case 3: c = n - n / 2; break;            // (n + 1) / 2
            default: c = n ? rng() % n : 0; break;
            }
            counts[static_cast<size_t>(l) * fp_bits + k] = c;
        }
        for (uint32_t w = 0; w < W; w++) previous[static_cast<size_t>(l) * W + w] = rng();
    }
    const int rc = gsim_label_centroids(counts.data(), sizes.data(), nlabels, fp_bits, with_previous ? previous.data() : nullptr, centres.data());
    CHECK(rc == GSIM_OK);
    for (uint32_t l = 0; l < nlabels; l++)
        for (uint32_t k = 0; k < fp_bits; k++) {
            const uint32_t got = (centres[static_cast<size_t>(l) * W + k / 32] >> (k % 32)) & 1u;
            uint32_t want;
            if (sizes[l] == 0) want = with_previous ? (previous[static_cast<size_t>(l) * W + k / 32] >> (k % 32)) & 1u : 0u;
            else want = 2ull * counts[static_cast<size_t>(l) * fp_bits + k] >= sizes[l] ? 1u : 0u;
            if (got != want) {
                std::fprintf(stderr, "label %u bit %u: size %u count %u: got %u\n", l, k, sizes[l], counts[static_cast<size_t>(l) * fp_bits + k], got);
                failures++;
                return;
            }
        }
}

} // namespace

int main()
{
    std::mt19937 rng(2024);
    const uint32_t widths[] = {32, 64, 160, 1024, 4096};
    for (int rep = 0; rep < 40; rep++)
        for (uint32_t fp_bits : widths) one_case(rng, 1 + rng() % 9, fp_bits, rep % 2 == 1);
    one_case(rng, 300, 1024, true);

    // malformed input: refused, and nothing written
    uint32_t counts[64] = {0}, sizes[2] = {3, 0}, out[2] = {5, 6}, prev[2] = {7, 8};
    counts[4] = 3;
    CHECK(gsim_label_centroids(counts, sizes, 2, 32, prev, out) == GSIM_OK && out[0] == 16u && out[1] == 8u);
    CHECK(gsim_label_centroids(counts, sizes, 2, 32, nullptr, out) == GSIM_OK && out[0] == 16u && out[1] == 0u);
    out[0] = 5;
    out[1] = 6;
    counts[40] = 1; // label 1 is empty: a count above its size
    CHECK(gsim_label_centroids(counts, sizes, 2, 32, prev, out) == GSIM_ERR_INVALID && out[0] == 5u && out[1] == 6u);
    counts[40] = 0;
    counts[4] = 4;
    CHECK(gsim_label_centroids(counts, sizes, 2, 32, prev, out) == GSIM_ERR_INVALID && out[0] == 5u);
    counts[4] = 3;
    CHECK(gsim_label_centroids(nullptr, sizes, 2, 32, prev, out) == GSIM_ERR_INVALID);
    CHECK(gsim_label_centroids(counts, nullptr, 2, 32, prev, out) == GSIM_ERR_INVALID);
    CHECK(gsim_label_centroids(counts, sizes, 2, 32, prev, nullptr) == GSIM_ERR_INVALID);
    CHECK(gsim_label_centroids(counts, sizes, 0, 32, prev, out) == GSIM_ERR_INVALID);
    CHECK(gsim_label_centroids(counts, sizes, 2, 0, prev, out) == GSIM_ERR_INVALID);
    CHECK(gsim_label_centroids(counts, sizes, 2, 48, prev, out) == GSIM_ERR_INVALID);
    CHECK(out[0] == 5u && out[1] == 6u);
    CHECK(gsim_last_error()[0] != 0);

    std::printf("%s kmeans_host_check: %d failures\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
