// popindex_host_check.cpp -- gsim_popcount_bounds with buffers of exactly the fp_bits + 1 floats the header promises.  A stand-alone
// program: tests/test_popindex_host.py compiles it TOGETHER WITH gpusimilarity_amd/csrc/capi_popindex_host.cpp, once plainly and once
// under -fsanitize=address,undefined (that file needs the public header and fail() alone; fail() is defined here), so the sanitizers
// see the function's own reads and writes.  No GPU, no library.
//
// Checked: Tanimoto's closed form (float) min(a, b) / (float) max(a, b) with 0 for 0 / 0, bit for bit; that every score the bound
// was enumerated from stays at or below it (the same arithmetic, written out again here); the hand-worked corners; the errors.
#include "../../include/gpusim_hip.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

namespace gsim_host
{
static std::string last_error;
int fail(int code, const std::string& msg)
{
    last_error = msg;
    return code;
}
} // namespace gsim_host

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);     \
            failures++;                                               \
        }                                                             \
    } while (0)

static bool same_bits(float x, float y) { return std::memcmp(&x, &y, 4) == 0; }

// the library's score from the three counts (gso_score_one's arithmetic)
static float score(int metric, float alpha, float beta, uint32_t a, uint32_t b, uint32_t c)
{
    if (metric == GSIM_METRIC_TVERSKY) {
        const float t1 = alpha * static_cast<float>(static_cast<int>(a - c));
        const float t2 = beta * static_cast<float>(static_cast<int>(b - c));
        return static_cast<float>(c) / ((t1 + t2) + static_cast<float>(c));
    }
    return static_cast<float>(c) / static_cast<float>(static_cast<int>(a + b) - static_cast<int>(c));
}

static void run(uint32_t F, uint32_t a, int metric, float alpha, float beta)
{
    std::unique_ptr<float[]> ub(new float[F + 1]); // exactly as large as promised
    CHECK(gsim_popcount_bounds(F, a, metric, alpha, beta, ub.get()) == GSIM_OK);
    for (uint32_t b = 0; b <= F; b++) {
        if (metric == GSIM_METRIC_TANIMOTO) {
            const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
            const float want = hi ? static_cast<float>(lo) / static_cast<float>(hi) : 0.0f;
            if (!same_bits(ub[b], want)) {
                std::printf("FAILED: Tanimoto F %u a %u b %u: %.9g, want %.9g\n", F, a, b, ub[b], want);
                failures++;
            }
        }
        const uint32_t c0 = a + b > F ? a + b - F : 0u, c1 = a < b ? a : b;
        bool attained = false;
        for (uint32_t c = c0; c <= c1; c++) {
            float s = score(metric, alpha, beta, a, b, c);
            s = s == s ? s : 0.0f;
            if (s > ub[b]) {
                std::printf("FAILED: F %u a %u b %u c %u scores %.9g above the bound %.9g\n", F, a, b, c, s, ub[b]);
                failures++;
            }
            attained = attained || same_bits(s, ub[b]) || s == ub[b];
        }
        CHECK(attained);
    }
}

int main()
{
    const uint32_t widths[] = {32, 64, 160, 1024};
    const float weights[][2] = {{1.0f, 1.0f}, {1.0f, 0.0f}, {0.5f, 0.5f}, {0.3f, 0.2f}, {2.0f, 0.5f}, {0.0f, 0.0f}};
    for (const uint32_t F : widths) {
        const uint32_t pops[] = {0, 1, F / 2, F - 1, F};
        for (const uint32_t a : pops) {
            run(F, a, GSIM_METRIC_TANIMOTO, 0.0f, 0.0f);
            for (const auto& w : weights) run(F, a, GSIM_METRIC_TVERSKY, w[0], w[1]);
        }
    }
    { // hand-worked: a = 10, 64-bit rows
        float ub[65];
        CHECK(gsim_popcount_bounds(64, 10, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, ub) == GSIM_OK);
        CHECK(ub[0] == 0.0f && ub[5] == 0.5f && ub[10] == 1.0f && ub[20] == 0.5f && ub[40] == 0.25f);
        CHECK(same_bits(ub[64], 10.0f / 64.0f)); // a row of all ones shares all ten bits
        // a = 60, b = 60: at least 56 bits are shared -- the bound is still 1, the overlap's floor does not lower it
        CHECK(gsim_popcount_bounds(64, 60, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, ub) == GSIM_OK);
        CHECK(ub[60] == 1.0f && same_bits(ub[64], 60.0f / 64.0f) && ub[0] == 0.0f);
        // Tversky (1, 0): the share of the query's bits that the row has -- 1 from b = a on
        CHECK(gsim_popcount_bounds(64, 10, GSIM_METRIC_TVERSKY, 1.0f, 0.0f, ub) == GSIM_OK);
        CHECK(ub[4] == 0.4f && ub[10] == 1.0f && ub[64] == 1.0f && ub[0] == 0.0f);
    }
    { // the errors
        float ub[33];
        CHECK(gsim_popcount_bounds(32, 0, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, nullptr) == GSIM_ERR_INVALID);
        CHECK(gsim_popcount_bounds(0, 0, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, ub) == GSIM_ERR_INVALID);
        CHECK(gsim_popcount_bounds(33, 0, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, ub) == GSIM_ERR_INVALID);
        CHECK(gsim_popcount_bounds(32800, 0, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, ub) == GSIM_ERR_INVALID);
        CHECK(gsim_popcount_bounds(32, 33, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, ub) == GSIM_ERR_INVALID);
        CHECK(gsim_popcount_bounds(32, 3, 7, 1.0f, 1.0f, ub) == GSIM_ERR_INVALID);
        CHECK(gsim_host::last_error == "unknown metric");
        CHECK(gsim_popcount_bounds(32, 32, GSIM_METRIC_TANIMOTO, 1.0f, 1.0f, ub) == GSIM_OK && ub[32] == 1.0f);
    }
    if (failures) std::printf("%d failures\n", failures);
    else std::printf("ok\n");
    return failures ? 1 : 0;
}
