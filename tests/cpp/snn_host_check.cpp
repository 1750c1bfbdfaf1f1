// snn_host_check.cpp -- gsim_snn and gsim_jarvis_patrick on a hand-worked graph of ten lists, with buffers of exactly the sizes the
// header promises.  A stand-alone program: tests/test_jarvis_patrick_host.py compiles it TOGETHER WITH
// gpusimilarity_amd/csrc/capi_snn_host.cpp, once plainly and once under -fsanitize=address,undefined (that file needs the public
// header and fail() alone; fail() is defined here), so the sanitizers see the functions' own reads and writes.  No GPU, no library.
//
// The graph (tests/test_jarvis_patrick_host.py works the same one through the Python rule): rows 0 - 3 list each other (every pair
// mutual, two rows shared); 4 and 5 list each other and share nothing; 6 has an empty list and is listed by 4 alone; 7 and 8 list
// each other and share 9; 7 lists 9, 9 does not list 7, and they share 8; 8 and 9 list each other and share nothing; 9 lists 0.
#include "../../include/gpusim_hip.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

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

// exact-size heap copies: an access one element past any of them is the sanitizer's to see
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v)
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

template <class T> static bool equal(const T* got, const std::vector<T>& want)
{
    return want.empty() || std::memcmp(got, want.data(), want.size() * sizeof(T)) == 0;
}

static const uint32_t M = GSIM_SNN_MUTUAL_BIT;
static const uint64_t N = 10;
static const std::vector<uint64_t> kIndptr = {0, 3, 6, 9, 12, 14, 16, 16, 18, 20, 22};
static const std::vector<uint32_t> kIndices = {3, 1, 2, 0, 3, 2, 1, 0, 3, 2, 1, 0, 6, 5, 7, 4, 9, 8, 7, 9, 8, 0};

struct Level {
    std::vector<uint32_t> cluster_of, first_row, sizes;
};

// one call with nlevels levels; every output is exactly as large as promised, first_row / sizes are pre-filled to see what is untouched
static void run(const std::vector<uint32_t>& kmins, uint32_t flags, const std::vector<Level>& want)
{
    const uint32_t nl = static_cast<uint32_t>(kmins.size());
    auto ip = exact(kIndptr);
    auto ix = exact(kIndices);
    auto km = exact(kmins);
    std::unique_ptr<uint32_t[]> c(new uint32_t[nl * N]), f(new uint32_t[nl * N]), z(new uint32_t[nl * N]), nc(new uint32_t[nl]);
    for (uint64_t t = 0; t < nl * N; t++) f[t] = z[t] = 0xABCDu;
    CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, km.get(), nl, flags, c.get(), f.get(), z.get(), nc.get()) == GSIM_OK);
    for (uint32_t l = 0; l < nl; l++) {
        CHECK(nc[l] == want[l].first_row.size());
        CHECK(equal(c.get() + l * N, want[l].cluster_of));
        CHECK(equal(f.get() + l * N, want[l].first_row));
        CHECK(equal(z.get() + l * N, want[l].sizes));
        for (uint64_t t = want[l].first_row.size(); t < N; t++) CHECK(f[l * N + t] == 0xABCDu && z[l * N + t] == 0xABCDu);
        // the single-level call is the stripe; first_row and sizes may be left out
        std::unique_ptr<uint32_t[]> c1(new uint32_t[N]), n1(new uint32_t[1]);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, km.get() + l, 1, flags, c1.get(), nullptr, nullptr, n1.get()) == GSIM_OK);
        CHECK(n1[0] == nc[l] && std::memcmp(c1.get(), c.get() + l * N, N * 4) == 0);
    }
}

int main()
{
    // the counts
    {
        auto ip = exact(kIndptr);
        auto ix = exact(kIndices);
        std::unique_ptr<uint32_t[]> s(new uint32_t[kIndices.size()]);
        CHECK(gsim_snn(ip.get(), ix.get(), N, 0, s.get()) == GSIM_OK);
        CHECK(equal(s.get(), std::vector<uint32_t>{M | 2, M | 2, M | 2, M | 2, M | 2, M | 2, M | 2, M | 2, M | 2, M | 2, M | 2, M | 2, 0, M, 0, M, 1,
                                                   M | 1, M | 1, M, M, 0}));
        CHECK(gsim_snn(ip.get(), ix.get(), N, GSIM_SNN_CLOSED, s.get()) == GSIM_OK);
        CHECK(equal(s.get(), std::vector<uint32_t>{M | 4, M | 4, M | 4, M | 4, M | 4, M | 4, M | 4, M | 4, M | 4, M | 4, M | 4, M | 4, 1, M | 2, 1,
                                                   M | 2, 2, M | 3, M | 3, M | 2, M | 2, 1}));
        CHECK(gsim_snn(ip.get(), ix.get(), N, GSIM_SNN_EITHER, s.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_host::last_error.find("flags") != std::string::npos);
        CHECK(gsim_snn(ip.get(), ix.get(), N, 0, nullptr) == GSIM_ERR_INVALID);
        // no rows, and no entries
        const std::vector<uint64_t> none = {0};
        auto ip0 = exact(none);
        CHECK(gsim_snn(ip0.get(), nullptr, 0, 0, nullptr) == GSIM_OK);
        const std::vector<uint64_t> empty3 = {0, 0, 0, 0};
        auto ip3 = exact(empty3);
        CHECK(gsim_snn(ip3.get(), nullptr, 3, 0, nullptr) == GSIM_OK);
    }
    const Level all_alone = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1}};
    const Level mutual_graph = {{0, 0, 0, 0, 1, 1, 2, 3, 3, 3}, {0, 4, 6, 7}, {4, 2, 1, 3}};
    const Level one = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0}, {10}};
    // open, mutual: kmin 0 is the mutual graph; at 1 the mutual pairs 4 - 5 and 8 - 9 share too little; at 2 only the clique is left
    run({0, 1, 2, 3}, 0,
        {mutual_graph,
         {{0, 0, 0, 0, 1, 2, 3, 4, 4, 5}, {0, 4, 5, 6, 7, 9}, {4, 1, 1, 1, 2, 1}},
         {{0, 0, 0, 0, 1, 2, 3, 4, 5, 6}, {0, 4, 5, 6, 7, 8, 9}, {4, 1, 1, 1, 1, 1, 1}},
         all_alone});
    // either: at 0 every entry links (4 - 6, 5 - 7, 9 - 0 join everything); at 1 the one-sided pair 7 - 9 (sharing 8) joins 9 to 7 and 8
    run({0, 1, 2, 3}, GSIM_SNN_EITHER,
        {one,
         {{0, 0, 0, 0, 1, 2, 3, 4, 4, 4}, {0, 4, 5, 6, 7}, {4, 1, 1, 1, 3}},
         {{0, 0, 0, 0, 1, 2, 3, 4, 5, 6}, {0, 4, 5, 6, 7, 8, 9}, {4, 1, 1, 1, 1, 1, 1}},
         all_alone});
    // closed: a mutual pair counts 2 more, so 4 - 5 and 8 - 9 (sharing nothing) hold up to kmin 2
    run({0, 1, 2, 3}, GSIM_SNN_CLOSED,
        {mutual_graph, mutual_graph, mutual_graph, {{0, 0, 0, 0, 1, 2, 3, 4, 4, 5}, {0, 4, 5, 6, 7, 9}, {4, 1, 1, 1, 2, 1}}});
    run({0, 1, 2, 3}, GSIM_SNN_CLOSED | GSIM_SNN_EITHER,
        {one, one, mutual_graph, {{0, 0, 0, 0, 1, 2, 3, 4, 4, 5}, {0, 4, 5, 6, 7, 9}, {4, 1, 1, 1, 2, 1}}});
    run({1}, 0, {{{0, 0, 0, 0, 1, 2, 3, 4, 4, 5}, {0, 4, 5, 6, 7, 9}, {4, 1, 1, 1, 2, 1}}});
    run({0, 1, 2, 3, 4, 5, 6, 1000}, 0,
        {mutual_graph,
         {{0, 0, 0, 0, 1, 2, 3, 4, 4, 5}, {0, 4, 5, 6, 7, 9}, {4, 1, 1, 1, 2, 1}},
         {{0, 0, 0, 0, 1, 2, 3, 4, 5, 6}, {0, 4, 5, 6, 7, 8, 9}, {4, 1, 1, 1, 1, 1, 1}},
         all_alone, all_alone, all_alone, all_alone, all_alone});
    // what is refused
    {
        auto ip = exact(kIndptr);
        auto ix = exact(kIndices);
        std::unique_ptr<uint32_t[]> c(new uint32_t[9 * N]), nc(new uint32_t[9]);
        const std::vector<uint32_t> nine = {0, 1, 2, 3, 4, 5, 6, 7, 8}, flat = {1, 1}, down = {2, 1};
        auto k9 = exact(nine);
        auto kf = exact(flat);
        auto kd = exact(down);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, k9.get(), 9, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, k9.get(), 0, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, kf.get(), 2, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, kd.get(), 2, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_host::last_error.find("ascending") != std::string::npos);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, k9.get(), 1, 4, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, nullptr, 1, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, k9.get(), 1, 0, nullptr, nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_jarvis_patrick(ip.get(), ix.get(), N, k9.get(), 1, 0, c.get(), nullptr, nullptr, nullptr) == GSIM_ERR_INVALID);
        // a list that names its own row, a list that names a row twice, a column outside the graph
        std::vector<uint32_t> self = kIndices, twice = kIndices, outside = kIndices;
        self[13] = 4;
        twice[17] = 9;
        outside[21] = 10;
        auto xs = exact(self);
        auto xt = exact(twice);
        auto xo = exact(outside);
        CHECK(gsim_jarvis_patrick(ip.get(), xs.get(), N, k9.get(), 1, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_host::last_error.find("list 4 names its own row") != std::string::npos);
        CHECK(gsim_jarvis_patrick(ip.get(), xt.get(), N, k9.get(), 1, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_host::last_error.find("list 7 names a row twice") != std::string::npos);
        CHECK(gsim_jarvis_patrick(ip.get(), xo.get(), N, k9.get(), 1, 0, c.get(), nullptr, nullptr, nc.get()) == GSIM_ERR_INVALID);
        std::unique_ptr<uint32_t[]> s(new uint32_t[kIndices.size()]);
        CHECK(gsim_snn(ip.get(), xs.get(), N, 0, s.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_snn(ip.get(), xt.get(), N, 0, s.get()) == GSIM_ERR_INVALID);
        CHECK(gsim_snn(ip.get(), xo.get(), N, 0, s.get()) == GSIM_ERR_INVALID);
        // no rows: legal, nothing but nclusters is written
        const std::vector<uint64_t> none = {0};
        auto ip0 = exact(none);
        nc[0] = 7;
        CHECK(gsim_jarvis_patrick(ip0.get(), nullptr, 0, k9.get(), 1, 0, nullptr, nullptr, nullptr, nc.get()) == GSIM_OK && nc[0] == 0);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
