// rowhash_host_check.cpp -- gsim_row_hash and gsim_duplicates with buffers of exactly the sizes the header promises.  A stand-alone
// program: tests/test_rowhash_host.py compiles it TOGETHER WITH gpusimilarity_amd/csrc/capi_rowhash_host.cpp, once plainly and once
// under -fsanitize=address,undefined (that file needs the public header, gsim_rowhash_hash.h and fail() alone; fail() is defined
// here), so the sanitizers see the functions' own reads and writes.  No GPU, no library.
//
// Checked: the hash against the header's definition written out again here, that it depends on a word's position, the groups of
// small tables against a quadratic comparison, the corners (no rows, one row, all rows identical, zero rows), NULL outputs, the errors.
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

static uint32_t m1(uint32_t x)
{
    x ^= x >> 16, x *= 0x85EBCA6Bu, x ^= x >> 13, x *= 0xC2B2AE35u, x ^= x >> 16;
    return x;
}
static uint32_t m2(uint32_t x)
{
    x ^= x >> 15, x *= 0x2C1B3C6Du, x ^= x >> 12, x *= 0x297A2D39u, x ^= x >> 15;
    return x;
}
// the header's definition
static uint64_t hash_of(const uint32_t* w, uint32_t W)
{
    uint32_t A = 0, B = 0;
    for (uint32_t i = 0; i < W; i++) {
        const uint32_t k = (i + 1u) * 0x9E3779B9u;
        uint32_t a = (w[i] ^ k) * 0x85EBCA6Bu;
        a ^= a >> 15;
        uint32_t b = (((w[i] << 16) | (w[i] >> 16)) + k) * 0xC2B2AE35u;
        b ^= b >> 13;
        A += a, B += b;
    }
    const uint32_t lo = m1(A ^ m2(B));
    const uint32_t hi = m2(B ^ lo);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

static uint32_t rnd_state = 0x1234567u;
static uint32_t rnd()
{
    rnd_state ^= rnd_state << 13, rnd_state ^= rnd_state >> 17, rnd_state ^= rnd_state << 5;
    return rnd_state;
}

// n rows of W words, about a third of them copies of earlier rows; every buffer has exactly the promised size
static void run(uint64_t n, uint32_t W, int kind)
{
    std::unique_ptr<uint32_t[]> rows(new uint32_t[n > 0 ? n * W : 1]);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t* r = rows.get() + i * W;
        for (uint32_t j = 0; j < W; j++) r[j] = kind == 1 ? 0u : kind == 2 ? 0xFFFFFFFFu : (rnd() & rnd());
        if (kind == 0 && i > 0 && rnd() % 3 == 0) std::memcpy(r, rows.get() + (rnd() % i) * W, W * 4);
        if (kind == 3 && i > 0) std::memcpy(r, rows.get(), W * 4), r[i % 2 ? W - 1 : 0] ^= 1u << (i % 32); // differ in the last or the first word only
    }
    std::unique_ptr<uint64_t[]> hash(new uint64_t[n ? n : 1]);
    std::unique_ptr<uint32_t[]> first(new uint32_t[n ? n : 1]), size(new uint32_t[n ? n : 1]), first2(new uint32_t[n ? n : 1]), size2(new uint32_t[n ? n : 1]);
    uint64_t ngroups = 99, groups = 0;
    CHECK(gsim_row_hash(rows.get(), n, W * 32, hash.get()) == GSIM_OK);
    CHECK(gsim_duplicates(rows.get(), n, W * 32, first.get(), size.get(), &ngroups) == GSIM_OK);
    for (uint64_t i = 0; i < n; i++) {
        CHECK(hash[i] == hash_of(rows.get() + i * W, W));
        uint32_t f = static_cast<uint32_t>(i), c = 0;
        for (uint64_t j = 0; j < n; j++)
            if (std::memcmp(rows.get() + i * W, rows.get() + j * W, W * 4) == 0) {
                c++;
                if (j < f) f = static_cast<uint32_t>(j);
            }
        CHECK(first[i] == f && size[i] == c);
        groups += f == i;
    }
    CHECK(ngroups == groups);
    // every output alone
    CHECK(gsim_duplicates(rows.get(), n, W * 32, first2.get(), nullptr, nullptr) == GSIM_OK);
    CHECK(gsim_duplicates(rows.get(), n, W * 32, nullptr, size2.get(), nullptr) == GSIM_OK);
    CHECK(std::memcmp(first.get(), first2.get(), n * 4) == 0 && std::memcmp(size.get(), size2.get(), n * 4) == 0);
    ngroups = 99;
    CHECK(gsim_duplicates(rows.get(), n, W * 32, nullptr, nullptr, &ngroups) == GSIM_OK && ngroups == groups);
}

int main()
{
    for (uint32_t W : {1u, 3u, 5u, 32u, 36u, 1024u})
        for (uint64_t n : {0ull, 1ull, 2ull, 63ull, 200ull})
            for (int kind = 0; kind < 4; kind++)
                if (W < 1024u || n <= 63) run(n, W, kind);
    run(1500, 2, 0); // more rows than half the smallest table: the slots double
    { // the position of a word matters
        uint32_t a[4] = {1, 2, 3, 4}, b[4] = {2, 1, 3, 4};
        uint64_t ha = 0, hb = 0;
        CHECK(gsim_row_hash(a, 1, 128, &ha) == GSIM_OK && gsim_row_hash(b, 1, 128, &hb) == GSIM_OK && ha != hb);
    }
    { // the errors
        uint32_t r[2] = {0, 0}, f[2];
        uint64_t h[2], g = 0;
        CHECK(gsim_row_hash(r, 2, 0, h) == GSIM_ERR_INVALID && gsim_row_hash(r, 2, 33, h) == GSIM_ERR_INVALID);
        CHECK(gsim_row_hash(r, 2, 32800, h) == GSIM_ERR_INVALID && gsim_row_hash(nullptr, 2, 32, h) == GSIM_ERR_INVALID);
        CHECK(gsim_row_hash(r, 2, 32, nullptr) == GSIM_ERR_INVALID && gsim_row_hash(nullptr, 0, 32, nullptr) == GSIM_OK);
        CHECK(gsim_row_hash(r, 0xFFFFFFFFull, 32, h) == GSIM_ERR_INVALID);
        CHECK(gsim_duplicates(r, 2, 0, f, f, &g) == GSIM_ERR_INVALID && gsim_duplicates(nullptr, 2, 32, f, nullptr, &g) == GSIM_ERR_INVALID);
        CHECK(gsim_duplicates(r, 0xFFFFFFFFull, 32, f, nullptr, &g) == GSIM_ERR_INVALID && !gsim_host::last_error.empty());
        CHECK(gsim_duplicates(nullptr, 0, 32, nullptr, nullptr, &g) == GSIM_OK && g == 0);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
