// hdbscan_host_check.cpp -- gsim_mreach_mst and gsim_mst_hdbscan (host code) through the C ABI, as a stand-alone program: every
// buffer has exactly the size the header promises, so that a build of this file and of capi_hdbscan.cpp / capi_mst.cpp /
// capi_pairs.cpp with -fsanitize=address,undefined checks the functions' reads and writes.  tests/test_hdbscan_host.py builds it
// plainly against the library and runs it.  Prints "ok".
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

void run(const Graph& g, uint32_t min_pts, uint32_t mcs, uint32_t flags, bool all_outputs)
{
    // the forest: at most n - 1 edges
    std::vector<gsim_mst_edge> edges(g.n ? g.n - 1 : 0);
    std::vector<float> core(g.n);
    uint64_t ne = 99;
    int rc = gsim_mreach_mst(g.indptr.data(), g.indices.empty() ? nullptr : g.indices.data(), g.scores.empty() ? nullptr : g.scores.data(), g.n,
                             min_pts, edges.empty() ? nullptr : edges.data(), &ne, all_outputs && g.n ? core.data() : nullptr);
    CHECK(rc == GSIM_OK);
    CHECK(ne <= edges.size());
    if (rc != GSIM_OK || ne > edges.size()) return;
    for (uint64_t e = 0; e < ne; e++) {
        CHECK(edges[e].a < edges[e].b && edges[e].b < g.n);
        CHECK(e == 0 || edges[e].score <= edges[e - 1].score);
        if (all_outputs) CHECK(edges[e].score <= core[edges[e].a] && edges[e].score <= core[edges[e].b]);
    }
    // the selection
    std::vector<uint32_t> label(g.n), first(g.n), sizes(g.n);
    std::vector<float> leave(g.n), birth(g.n);
    std::vector<double> stab(g.n);
    uint64_t nc = 99;
    const float floor = 0.125f; // below every score
    rc = gsim_mst_hdbscan(ne ? edges.data() : nullptr, ne, g.n, floor, mcs, flags, g.n ? label.data() : nullptr, &nc,
                          all_outputs && g.n ? leave.data() : nullptr, all_outputs && g.n ? first.data() : nullptr,
                          all_outputs && g.n ? sizes.data() : nullptr, all_outputs && g.n ? birth.data() : nullptr,
                          all_outputs && g.n ? stab.data() : nullptr);
    CHECK(rc == GSIM_OK);
    CHECK(nc <= g.n / (mcs ? mcs : 1));
    uint64_t in_clusters = 0, summed = 0;
    for (uint64_t r = 0; r < g.n; r++) {
        CHECK(label[r] == GSIM_HDBSCAN_NOISE || label[r] < nc);
        in_clusters += label[r] != GSIM_HDBSCAN_NOISE;
        if (all_outputs) CHECK(leave[r] == 0.0f || leave[r] >= floor);
        if (all_outputs && label[r] != GSIM_HDBSCAN_NOISE) CHECK(leave[r] >= birth[label[r]]);
    }
    if (all_outputs) {
        for (uint64_t c = 0; c < nc; c++) {
            CHECK(first[c] < g.n && label[first[c]] == c);
            CHECK(c == 0 || first[c - 1] < first[c]);
            CHECK(sizes[c] >= mcs && birth[c] >= floor && stab[c] >= 0.0);
            summed += sizes[c];
        }
        CHECK(summed == in_clusters);
    }
}

} // namespace

int main()
{
    // the hand-worked forest of tests/test_hdbscan_host.py: three chains, small pieces at the split
    const Graph hand = make(13, {0, 1, 3, 4, 6, 7, 11, 0, 2, 5, 8, 10}, {1, 2, 4, 5, 7, 8, 12, 10, 3, 6, 9, 11},
                            {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, .75f, .5f, .5f, .5f, .5f, .5f});
    for (uint32_t mp = 1; mp <= 4; mp++)
        for (uint32_t mcs = 2; mcs <= 5; mcs++)
            for (uint32_t flags = 0; flags < 4; flags++) {
                run(hand, mp, mcs, flags, true);
                run(hand, mp, mcs, flags, false);
            }
    run(make(0, {}, {}, {}), 3, 2, 0, true);
    run(make(1, {}, {}, {}), 1, 2, 0, true);
    run(make(5, {}, {}, {}), 2, 2, 1, true);
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
        for (uint32_t mp : {1u, 2u, 3u, 5u, 100u}) run(gr, mp, 2 + g % 5, g % 4, g % 2 == 0);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
