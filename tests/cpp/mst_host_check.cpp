// mst_host_check.cpp -- gsim_mst, gsim_mst_linkage and gsim_mst_cut (capi_mst.cpp, host code) on random and malformed graphs: a
// stand-alone program for a sanitizer build (DESIGN.md section 19 has the command line and the result).  It checks the outputs
// against a Kruskal of its own and exits non-zero on the first difference; the sanitizers report on their own.
#include "../../include/gpusim_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

struct Csr {
    std::vector<uint64_t> indptr;
    std::vector<uint32_t> indices;
    std::vector<float> scores;
};

uint32_t root(std::vector<uint32_t>& p, uint32_t x)
{
    while (p[x] != x) x = p[x] = p[p[x]];
    return x;
}

void random_graph(std::mt19937& rng, uint32_t n, double density, Csr* g, std::vector<gsim_mst_edge>* want)
{
    const float values[6] = {0.125f, 0.25f, 0.5f, 0.625f, 0.75f, 1.0f};
    std::vector<std::vector<std::pair<uint32_t, float>>> adj(n);
    std::vector<gsim_mst_edge> all;
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (uint32_t a = 0; a < n; a++)
        for (uint32_t b = a + 1; b < n; b++)
            if (u(rng) < density) {
                const float s = values[rng() % 6];
                adj[a].push_back({b, s});
                adj[b].push_back({a, s});
                all.push_back({a, b, s});
            }
    g->indptr.assign(1, 0);
    g->indices.clear();
    g->scores.clear();
    for (uint32_t r = 0; r < n; r++) {
        for (const auto& e : adj[r]) {
            g->indices.push_back(e.first);
            g->scores.push_back(e.second);
        }
        g->indptr.push_back(g->indices.size());
    }
    std::sort(all.begin(), all.end(), [](const gsim_mst_edge& x, const gsim_mst_edge& y) {
        return x.score != y.score ? x.score > y.score : x.a != y.a ? x.a < y.a : x.b < y.b;
    });
    std::vector<uint32_t> p(n);
    for (uint32_t r = 0; r < n; r++) p[r] = r;
    want->clear();
    for (const gsim_mst_edge& e : all) {
        const uint32_t x = root(p, e.a), y = root(p, e.b);
        if (x != y) {
            p[std::max(x, y)] = std::min(x, y);
            want->push_back(e);
        }
    }
}

} // namespace

int main()
{
    std::mt19937 rng(0x3157);
    Csr g;
    std::vector<gsim_mst_edge> want;
    for (int it = 0; it < 300; it++) {
        const uint32_t n = rng() % 90;
        const double density = it % 4 == 0 ? 0.6 : it % 4 == 1 ? 0.1 : 2.0 / (n + 1.0);
        random_graph(rng, n, density, &g, &want);
        // exactly the documented capacities: nrows - 1 edges, nedges merges, nrows labels, ncomponents first rows and sizes
        std::vector<gsim_mst_edge> edges(n > 1 ? n - 1 : 0);
        uint64_t ne = 99;
        CHECK(gsim_mst(g.indptr.data(), g.indices.data(), g.scores.data(), n, edges.data(), &ne) == GSIM_OK);
        CHECK(ne == want.size());
        for (uint64_t e = 0; e < ne && e < want.size(); e++)
            CHECK(edges[e].a == want[e].a && edges[e].b == want[e].b && edges[e].score == want[e].score);
        std::vector<gsim_mst_merge> merges(ne);
        CHECK(gsim_mst_linkage(edges.data(), ne, n, merges.data()) == GSIM_OK);
        for (uint64_t m = 0; m < ne; m++) CHECK(merges[m].left != merges[m].right && merges[m].size >= 2 && merges[m].size <= n);
        for (float t : {0.0f, 0.25f, 0.5f, 0.7f, 1.0f, 2.0f}) {
            uint64_t nc = 0, kept = 0;
            for (uint64_t e = 0; e < ne; e++) kept += edges[e].score >= t;
            std::vector<uint32_t> comp(n), first(n - kept), sizes(n - kept);
            CHECK(gsim_mst_cut(edges.data(), ne, n, t, comp.data(), first.data(), sizes.data(), &nc) == GSIM_OK);
            CHECK(nc == n - kept);
            uint64_t sum = 0;
            for (uint64_t c = 0; c < nc; c++) sum += sizes[c];
            CHECK(sum == n);
        }
        // malformed: every check must come before any write or read past the arrays
        if (n >= 3 && !g.indices.empty()) {
            Csr bad = g;
            bad.indices[rng() % bad.indices.size()] = n + rng() % 5;
            CHECK(gsim_mst(bad.indptr.data(), bad.indices.data(), bad.scores.data(), n, edges.data(), &ne) == GSIM_ERR_INVALID);
            bad = g;
            bad.scores[rng() % bad.scores.size()] = std::numeric_limits<float>::quiet_NaN();
            CHECK(gsim_mst(bad.indptr.data(), bad.indices.data(), bad.scores.data(), n, edges.data(), &ne) == GSIM_ERR_INVALID);
            bad = g;
            bad.indptr[1 + rng() % (n - 1)] = bad.indptr[n] + 7;
            CHECK(gsim_mst(bad.indptr.data(), bad.indices.data(), bad.scores.data(), n, edges.data(), &ne) == GSIM_ERR_INVALID);
        }
        if (!want.empty()) {
            std::vector<gsim_mst_edge> bad = want;
            std::vector<uint32_t> comp(n);
            uint64_t nc = 0;
            std::vector<gsim_mst_merge> merges2(bad.size() + 1);
            bad[rng() % bad.size()].b = n + rng() % 3;
            CHECK(gsim_mst_linkage(bad.data(), bad.size(), n, merges2.data()) == GSIM_ERR_INVALID);
            CHECK(gsim_mst_cut(bad.data(), bad.size(), n, 0.5f, comp.data(), nullptr, nullptr, &nc) == GSIM_ERR_INVALID);
            bad = want;
            bad.push_back(bad[rng() % bad.size()]); // an edge twice: a cycle for the dendrogram, harmless to a cut
            if (bad.size() < n) CHECK(gsim_mst_linkage(bad.data(), bad.size(), n, merges2.data()) == GSIM_ERR_INVALID);
            CHECK(gsim_mst_cut(bad.data(), bad.size(), n, 0.5f, comp.data(), nullptr, nullptr, &nc) == GSIM_OK);
            std::reverse(bad.begin(), bad.end());
            CHECK(gsim_mst_linkage(bad.data(), bad.size(), n, merges2.data()) == GSIM_ERR_INVALID);
        }
    }
    std::printf("mst_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
