// capi_mst.cpp -- gsim_db_mst (the exact single-linkage dendrogram of the table as its maximum-similarity spanning forest, by
// Boruvka rounds on the device) and its host companions gsim_mst (the same rule on a scored CSR graph), gsim_mst_linkage and
// gsim_mst_cut.  The argument checks and the round loop of a call; the device side is gsim_mst.hip.  The rule is stated in
// include/gpusim_hip.h.  The round loop (boruvka_forest) also serves gsim_db_mreach_mst (capi_hdbscan.cpp), with another fold
// launcher; so do the edge order, the edge checks and Kruskal on a list of pairs (capi_pairs.h).
#include "capi_front.h"

#include <algorithm>
#include <cmath>

namespace gsim_host
{
namespace
{

// column pieces of one fold launch that run side by side: enough workgroups to fill the device when the owner list is short, and
// several layers of them, so that the partly filled last layer is a small share of the launch (2048 left
// scans of 77 k to 320 k owners at 0.66 of the VALU ceiling, 8192 has them above 0.8)
uint32_t mst_chunks(const KnnLaunch& l)
{
    const uint64_t want = (8192 + l.not_ - 1) / l.not_;
    const uint64_t most = (l.c1 - l.c0 + gsim::kKnnColTile - 1) / gsim::kKnnColTile;
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min(std::min(want, most), uint64_t{65535})));
}

} // namespace

int boruvka_forest(gsim_db* db, Shard& s, float cutoff, int metric, float alpha, float beta, uint32_t row_base, const ForestFold& ff,
                   gsim_mst_edge* edges, uint64_t* nedges, gsim_mst_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    if (st) st->rows = N;
    if (N < 2) {
        if (st) st->wall_ms = ms_since(t0);
        return GSIM_OK;
    }
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;
    const long long knob = db->knobs.mst_launch_pairs;
    uint32_t max_scans = 1; // ceil(log2 N) + 1
    while ((uint64_t{1} << (max_scans - 1)) < N) max_scans++;

    // the first scan's plan is the largest: every row an owner
    const size_t max_launches = plan_knn(N, N, WP, knob).size();
    size_t select_bytes = 0, sort_bytes = 0;
    GSIM_HIP(gsim::mst_select_bytes(N, &select_bytes));
    GSIM_HIP(gsim::mst_sort_bytes(N - 1, &sort_bytes));
    PaddedRows table;
    LaunchClocks clocks;
    DevBuf<uint32_t> comp, parent, own, flag, cscore, eb;
    DevBuf<unsigned long long> best, ckey, ekey, ctl;
    DevBuf<gsim_mst_edge> d_edges;
    DevBuf<> tmp;
    if (const int rc = table.alloc(N, s.W, WP, "the spanning forest (popcounts)", "the spanning forest (the padded rows)")) return rc;
    GSIM_ALLOC(comp, N * 4, "the spanning forest (component ids)");
    GSIM_ALLOC(parent, N * 4, "the spanning forest (component links)");
    GSIM_ALLOC(own, N * 4, "the spanning forest (the owner list)");
    GSIM_ALLOC(flag, N * 4, "the spanning forest (the owner flags)");
    GSIM_ALLOC(cscore, N * 4, "the spanning forest (the components' picks)");
    GSIM_ALLOC(ckey, N * 8, "the spanning forest (the components' picks)");
    GSIM_ALLOC(best, N * 8, "the spanning forest (the rows' held edges)");
    GSIM_ALLOC(ekey, (N - 1) * 8, "the spanning forest (edges)");
    GSIM_ALLOC(eb, (N - 1) * 4, "the spanning forest (edges)");
    GSIM_ALLOC(d_edges, (N - 1) * sizeof(gsim_mst_edge), "the spanning forest (edges)");
    GSIM_ALLOC(ctl, gsim::kMstCtlWords * 8, "the spanning forest (control block)");
    if (const int rc = clocks.own(max_launches, "the spanning forest (clock stamps)")) return rc;
    GSIM_ALLOC(tmp, std::max(select_bytes, sort_bytes), "the spanning forest (select and sort scratch)");

    gsim::MstState m{};
    m.nrows = N;
    m.comp = comp;
    m.parent = parent;
    m.own = own;
    m.flag = flag;
    m.cscore = cscore;
    m.best = best;
    m.ckey = ckey;
    m.ekey = ekey;
    m.eb = eb;
    m.cap = N - 1;
    m.ctl = ctl;
    gsim::MstArgs a{};
    a.comp = comp;
    a.own = own;
    a.nrows = N;
    a.WP = WP;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;
    a.best = best;

    EventPair ev_fold, ev_round, ev_sort, ev_d2h;
    GSIM_HIP(ev_fold.create());
    GSIM_HIP(ev_round.create());
    GSIM_HIP(ev_sort.create());
    GSIM_HIP(ev_d2h.create());
    if (const int rc = table.prepare(s.d_rows, N, stream)) return rc;
    a.rows = table.rows();
    a.pop = table.pop();
    if (ff.prepare)
        if (const int rc = ff.prepare(table, stream)) return rc;
    GSIM_HIP(gsim::launch_mst_init(m, stream));

    gsim_mst_stats ms{};
    ms.rows = N;
    uint64_t total = 0, nown = N;
    for (;;) {
        if (ms.scans >= max_scans) return fail(GSIM_ERR_STATE, "mst: more rounds than a forest of this many rows can take");
        // this round's owners against every row: the fold launches, then the bookkeeping and the next round's owner list
        const std::vector<KnnLaunch> plan = nown ? plan_knn(nown, N, WP, knob) : std::vector<KnnLaunch>();
        if (plan.size() > max_launches) return fail(GSIM_ERR_STATE, "mst: a launch plan larger than the first round's");
        a.nown = static_cast<uint32_t>(nown);
        if (!plan.empty()) GSIM_HIP(clocks.zero(plan.size(), stream));
        GSIM_HIP(hipEventRecord(ev_fold.a, stream));
        for (size_t l = 0; l < plan.size(); l++) {
            a.clk = clocks.at(l);
            GSIM_HIP(ff.fold(a, plan[l].ot0, plan[l].not_, plan[l].c0, plan[l].c1, mst_chunks(plan[l]), stream));
        }
        GSIM_HIP(hipEventRecord(ev_fold.b, stream));
        GSIM_HIP(hipEventRecord(ev_round.a, stream));
        GSIM_HIP(gsim::launch_mst_round(m, tmp, select_bytes, stream));
        GSIM_HIP(hipEventRecord(ev_round.b, stream));
        // the one read of the round: edges so far, owners of the next round
        unsigned long long h_ctl[gsim::kMstCtlWords] = {};
        GSIM_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, stream));
        GSIM_HIP(clocks.fetch(plan.size(), stream));
        GSIM_HIP(hipStreamSynchronize(stream));
        clocks.add(); // (summed over the rounds)
        const double fold_ms = ev_fold.ms();
        ms.scan_owners[ms.scans] = nown;
        ms.scan_kernel_ms[ms.scans] = fold_ms;
        ms.scans++;
        ms.launches += plan.size();
        ms.pairs += nown * N;
        ms.kernel_ms += fold_ms;
        ms.round_ms += ev_round.ms();
        const uint64_t now = h_ctl[gsim::kMstCtlEdges];
        if (now > N - 1 || now < total || h_ctl[gsim::kMstCtlOwners] > N) return fail(GSIM_ERR_STATE, "mst: the device reported an impossible count");
        if (now == total) break; // no component has an outgoing edge
        ms.rounds++;
        ms.owner_rows += nown;
        total = now;
        nown = h_ctl[gsim::kMstCtlOwners];
        if (total == N - 1) break; // one tree: nothing is foreign any more
    }

    GSIM_HIP(hipEventRecord(ev_sort.a, stream));
    GSIM_HIP(gsim::launch_mst_count_roots(m, stream));
    // (the components' picks are dead now: the sort's second buffers)
    GSIM_HIP(gsim::launch_mst_sort(m, total, tmp, sort_bytes, ckey, cscore, row_base, d_edges, stream));
    GSIM_HIP(hipEventRecord(ev_sort.b, stream));
    unsigned long long h_ctl[gsim::kMstCtlWords] = {};
    GSIM_HIP(hipEventRecord(ev_d2h.a, stream));
    GSIM_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, stream));
    if (total) GSIM_HIP(hipMemcpyAsync(edges, d_edges, total * sizeof(gsim_mst_edge), hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipEventRecord(ev_d2h.b, stream));
    GSIM_HIP(hipStreamSynchronize(stream));
    if (h_ctl[gsim::kMstCtlRoots] < 1 || h_ctl[gsim::kMstCtlRoots] > N || total != N - h_ctl[gsim::kMstCtlRoots])
        return fail(GSIM_ERR_STATE, "mst: the edges and the component count do not add up");
    *nedges = total;
    if (st) {
        ms.edges = total;
        ms.sort_ms = ev_sort.ms();
        ms.d2h_ms = ev_d2h.ms();
        ms.clock_mhz = clocks.mhz();
        ms.wall_ms = ms_since(t0);
        *st = ms;
    }
    return GSIM_OK;
}

bool before_in_e(const gsim_mst_edge& x, const gsim_mst_edge& y)
{
    if (x.score != y.score) return x.score > y.score;
    if (x.a != y.a) return x.a < y.a;
    return x.b < y.b;
}

int check_edges(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows)
{
    if (nedges && !edges) return fail(GSIM_ERR_INVALID, "NULL edges");
    if (nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "more than 2^32-1 rows");
    for (uint64_t e = 0; e < nedges; e++) {
        if (!(edges[e].a < edges[e].b) || edges[e].b >= nrows) return fail(GSIM_ERR_INVALID, "mst: an edge needs a < b < nrows");
        if (std::isnan(edges[e].score)) return fail(GSIM_ERR_INVALID, "mst: an edge with a NaN score");
    }
    return GSIM_OK;
}

int check_scored_csr(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows, const gsim_mst_edge* edges,
                     uint64_t* nnz)
{
    if (const int rc = check_csr_offsets(indptr, nrows, nnz)) return rc;
    if (*nnz && (!indices || !scores)) return fail(GSIM_ERR_INVALID, "NULL indices or scores");
    if (nrows > 1 && !edges) return fail(GSIM_ERR_INVALID, "NULL edges");
    if (const int rc = check_csr_indices(indices, *nnz, nrows)) return rc;
    for (uint64_t e = 0; e < *nnz; e++)
        if (std::isnan(scores[e])) return fail(GSIM_ERR_INVALID, "mst: an edge with a NaN score");
    return GSIM_OK;
}

uint64_t kruskal_in_e(std::vector<gsim_mst_edge>& all, uint64_t nrows, gsim_mst_edge* edges)
{
    std::sort(all.begin(), all.end(), before_in_e);
    Forest f(nrows);
    uint64_t n = 0;
    for (const gsim_mst_edge& e : all)
        if (f.unite(e.a, e.b)) edges[n++] = e;
    return n;
}

} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_mst(gsim_db* db, float cutoff, int metric, float alpha, float beta, gsim_mst_edge* edges, uint64_t* nedges, gsim_mst_stats* stats)
{
    if (stats) *stats = gsim_mst_stats{};
    if (nedges) *nedges = 0;
    if (!db || !nedges) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_cutoff("mst", cutoff)) return rc;
    if (const int rc = check_symmetric_metric("mst needs", "mst", metric, alpha, beta)) return rc;
    if (const int rc = check_tile_table(db, "mst")) return rc;
    const uint64_t N = db->nrows;
    if (N > 1 && !edges) return fail(GSIM_ERR_INVALID, "NULL edges");
    if (N == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "mst", false)) return rc;
    ForestFold ff;
    ff.fold = [](const gsim::MstArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t nchunk, hipStream_t st) {
        return gsim::launch_mst_fold(a, ot0, not_, c0, c1, nchunk, st);
    };
    return on_one_shard(db, "host memory for the spanning forest",
                        [&](Shard& s) { return boruvka_forest(db, s, cutoff, metric, alpha, beta, db->row_base, ff, edges, nedges, stats); });
}

int gsim_mst(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows, gsim_mst_edge* edges, uint64_t* nedges)
{
    if (nedges) *nedges = 0;
    if (!indptr || !nedges) return fail(GSIM_ERR_INVALID, "NULL argument");
    uint64_t nnz = 0;
    if (const int rc = check_scored_csr(indptr, indices, scores, nrows, edges, &nnz)) return rc;
    try {
        // every listed pair once per listing, as a < b; Kruskal skips what it has seen
        std::vector<gsim_mst_edge> all;
        all.reserve(nnz);
        for (uint64_t r = 0; r < nrows; r++)
            for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++) {
                const uint32_t i = static_cast<uint32_t>(r), j = indices[e];
                if (i != j) all.push_back({std::min(i, j), std::max(i, j), scores[e]});
            }
        *nedges = kruskal_in_e(all, nrows, edges);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "mst");
    }
    return GSIM_OK;
}

int gsim_mst_linkage(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows, gsim_mst_merge* merges)
{
    if (nedges && !merges) return fail(GSIM_ERR_INVALID, "NULL merges");
    const int rc = check_edges(edges, nedges, nrows);
    if (rc != GSIM_OK) return rc;
    if (nedges && nedges >= nrows) return fail(GSIM_ERR_INVALID, "mst: a forest over nrows rows has fewer than nrows edges");
    if (nrows + nedges > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "mst: cluster ids beyond 2^32-1");
    try {
        Forest f(nrows);
        // of the tree rooted at (= whose smallest row is) r: its cluster id and its size
        std::vector<uint32_t> id(nrows), size(nrows, 1);
        for (uint64_t r = 0; r < nrows; r++) id[r] = static_cast<uint32_t>(r);
        for (uint64_t m = 0; m < nedges; m++) {
            if (m && edges[m].score > edges[m - 1].score) return fail(GSIM_ERR_INVALID, "mst: the scores of a dendrogram's edges must not increase");
            const uint32_t x = f.root(edges[m].a), y = f.root(edges[m].b);
            if (x == y) return fail(GSIM_ERR_INVALID, "mst: an edge whose ends are already connected");
            const uint32_t lo = std::min(x, y), hi = std::max(x, y);
            merges[m] = {id[lo], id[hi], edges[m].score, size[lo] + size[hi]};
            f.parent[hi] = lo;
            id[lo] = static_cast<uint32_t>(nrows + m);
            size[lo] += size[hi];
        }
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "mst");
    }
    return GSIM_OK;
}

int gsim_mst_cut(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows, float t, uint32_t* component_of, uint32_t* first_row,
                 uint32_t* sizes, uint64_t* ncomponents)
{
    if (!ncomponents || (nrows && !component_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (std::isnan(t)) return fail(GSIM_ERR_INVALID, "mst: a NaN threshold");
    const int rc = check_edges(edges, nedges, nrows);
    if (rc != GSIM_OK) return rc;
    try {
        Forest f(nrows);
        for (uint64_t e = 0; e < nedges; e++)
            if (edges[e].score >= t) f.unite(edges[e].a, edges[e].b);
        *ncomponents = number_components(f, nrows, component_of, first_row, sizes);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "mst");
    }
    return GSIM_OK;
}

} // extern "C"
