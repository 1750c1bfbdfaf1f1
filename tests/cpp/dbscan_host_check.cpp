// dbscan_host_check.cpp -- gsim_dbscan (host code) through the C ABI, as a stand-alone program: every buffer has exactly the size
// the header promises, so that a build of this file and of capi_dbscan.cpp / capi_pairs.cpp with -fsanitize=address,undefined checks
// the function's reads and writes.  tests/test_dbscan_host.py builds it plainly against the library and runs it.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/gpusim_hip.h"

namespace
{

struct Graph {
    uint64_t n;
    std::vector<uint64_t> indptr;
    std::vector<uint32_t> indices;
    std::vector<float> scores;
};

// a symmetric graph from its pairs
Graph make(uint64_t n, const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, const std::vector<float>& s)
{
    Graph g;
    g.n = n;
    g.indptr.assign(n + 1, 0);
    for (size_t e = 0; e < a.size(); e++) {
        g.indptr[a[e] + 1]++;
        g.indptr[b[e] + 1]++;
    }
    for (uint64_t r = 0; r < n; r++) g.indptr[r + 1] += g.indptr[r];
    g.indices.resize(2 * a.size());
    g.scores.resize(2 * a.size());
    std::vector<uint64_t> at(g.indptr.begin(), g.indptr.end() - 1);
    for (size_t e = 0; e < a.size(); e++) {
        g.indices[at[a[e]]] = b[e];
        g.scores[at[a[e]]++] = s[e];
        g.indices[at[b[e]]] = a[e];
        g.scores[at[b[e]]++] = s[e];
    }
    return g;
}

int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);       \
            failures++;                                              \
        }                                                            \
    } while (0)

void run(const Graph& g, uint32_t min_pts, bool all_outputs)
{
    std::vector<uint32_t> label(g.n), anchor(g.n), first(g.n), sizes(g.n);
    uint64_t nc = 99;
    const int rc = gsim_dbscan(g.indptr.data(), g.indices.empty() ? nullptr : g.indices.data(), g.scores.empty() ? nullptr : g.scores.data(), g.n,
                               min_pts, g.n ? label.data() : nullptr, all_outputs && g.n ? anchor.data() : nullptr,
                               all_outputs && g.n ? first.data() : nullptr, all_outputs && g.n ? sizes.data() : nullptr, &nc);
    CHECK(rc == GSIM_OK);
    CHECK(nc <= g.n);
    uint64_t in_clusters = 0, summed = 0;
    for (uint64_t r = 0; r < g.n; r++) {
        CHECK(label[r] == GSIM_DBSCAN_NOISE || label[r] < nc);
        in_clusters += label[r] != GSIM_DBSCAN_NOISE;
        if (all_outputs) CHECK((label[r] == GSIM_DBSCAN_NOISE) == (anchor[r] == GSIM_DBSCAN_NOISE));
    }
    if (all_outputs) {
        for (uint64_t c = 0; c < nc; c++) {
            CHECK(first[c] < g.n && label[first[c]] == c && anchor[first[c]] == first[c]);
            CHECK(c == 0 || first[c - 1] < first[c]);
            summed += sizes[c];
        }
        CHECK(summed == in_clusters);
    }
}

} // namespace

int main()
{
    // the hand-worked graph of tests/test_dbscan_host.py
    const Graph hand = make(12, {0, 0, 0, 1, 1, 2, 5, 5, 5, 6, 6, 7, 3, 4, 8, 0, 10}, {1, 2, 3, 2, 3, 3, 6, 7, 8, 7, 8, 8, 4, 5, 9, 9, 11},
                            {.75f, .75f, .75f, .75f, .75f, .75f, .5f, .5f, .5f, .5f, .5f, .5f, .25f, .25f, .25f, .125f, .875f});
    for (uint32_t mp = 1; mp <= 6; mp++) {
        run(hand, mp, true);
        run(hand, mp, false);
    }
    run(make(0, {}, {}, {}), 3, true);
    run(make(1, {}, {}, {}), 1, true);
    run(make(5, {}, {}, {}), 2, true);
    // random graphs with tied scores
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (int g = 0; g < 200; g++) {
        const uint32_t n = static_cast<uint32_t>(next() % 60);
        std::vector<uint32_t> a, b;
        std::vector<float> s;
        const uint64_t dens = next() % 8 + 1;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = i + 1; j < n; j++)
                if (next() % 16 < dens) {
                    a.push_back(i);
                    b.push_back(j);
                    s.push_back(0.25f * static_cast<float>(next() % 4 + 1));
                }
        const Graph gr = make(n, a, b, s);
        for (uint32_t mp : {1u, 2u, 3u, 5u, 100u}) run(gr, mp, g % 2 == 0);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
