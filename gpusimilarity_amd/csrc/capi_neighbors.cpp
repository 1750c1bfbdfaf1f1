// capi_neighbors.cpp -- gsim_db_neighbors (every pair of rows at or above a cutoff, as CSR) and gsim_butina (Taylor-Butina
// clustering of such a graph, host code).  The device side is gsim_neighbors.hip.
#include "capi_front.h"

#include <numeric>

namespace gsim_host
{
namespace
{

int neighbors(gsim_db* db, Shard& s, float cutoff, int metric, float alpha, float beta, uint64_t rb, uint64_t re, gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint64_t nout = re - rb;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    const bool tri = rb == 0 && re == N;
    g->indptr.assign(nout + 1, 0);
    if (nout == 0 || N < 2) {
        g->stats.wall_ms = ms_since(t0);
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    // popc of every row, and the rows zero-padded to WP words unless they already are WP words
    PaddedRows table;
    if (const int rc = table.alloc(N, s.W, WP)) return rc;
    if (const int rc = table.prepare(s.d_rows, N, st)) return rc;

    const uint64_t nlt = (nout + gsim::kNbrTile - 1) / gsim::kNbrTile;
    const uint64_t nct = (N + gsim::kNbrTile - 1) / gsim::kNbrTile;
    const std::vector<NbrLaunch> plan = plan_launches(nlt, nct, tri, WP);
    DevBuf<> ctl; // [0] the cursor, [1 + l] the cursor after launch l, then 4 clock stamps per launch
    GSIM_HIP(ctl.grow((1 + 5 * plan.size()) * 8));
    unsigned long long* d_cursor = ctl.as<unsigned long long>();
    unsigned long long* d_snap = d_cursor + 1;
    LaunchClocks clocks;
    clocks.view(d_snap + plan.size());
    gsim::NbrArgs a{};
    a.rows = table.rows();
    a.pop = table.pop();
    a.nrows = N;
    a.row_begin = rb;
    a.row_end = re;
    a.WP = WP;
    a.tri = tri ? 1 : 0;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;

    PairRun run;
    const int rc = run_pair_launches(s, plan.size(), d_cursor, d_snap, [&](size_t l, const PairSink& sink) {
        gsim::NbrArgs al = a;
        al.keys = sink.keys;
        al.vals = sink.vals;
        al.cursor = sink.cursor;
        al.cap = sink.cap;
        al.clk = clocks.at(l);
        GSIM_HIP(gsim::launch_nbr_tiles(al, plan[l].rt0, plan[l].nrt, plan[l].ct0, plan[l].nct, st));
        return static_cast<int>(GSIM_OK);
    }, &run);
    if (rc != GSIM_OK) return rc;
    const uint64_t total = run.total;
    g->stats.launches = plan.size();
    g->stats.launches_rerun = run.rerun;
    g->stats.tile_ms = run.ms;
    g->stats.pairs = tri ? total / 2 : total;
    GSIM_HIP(clocks.fetch(plan.size(), st));
    GSIM_HIP(hipStreamSynchronize(st));
    clocks.add();
    g->stats.clock_mhz = clocks.mhz();
    const int rc2 = build_pair_csr(db, s, total, nout, GSIM_JOIN_BY_ROW, g);
    if (rc2 != GSIM_OK) return rc2;
    g->stats.wall_ms = ms_since(t0);
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_neighbors(gsim_db* db, float cutoff, int metric, float alpha, float beta, uint64_t row_begin, uint64_t row_end,
                      gsim_graph** out)
{
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, "neighbour cutoff must be in (0, 1]");
    // (no prefix: alpha == beta is not checked for finiteness here -- a known quirk)
    if (const int rc = check_symmetric_metric("neighbour lists need", nullptr, metric, alpha, beta)) return rc;
    if (gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "neighbour lists support rows of up to 4096 bits");
    if (row_begin > row_end || row_end > db->nrows) return fail(GSIM_ERR_INVALID, "row range outside the table");
    if (const int rc = check_table_state(db, "neighbour lists", true)) return rc;
    const char* nomem = "host memory for the neighbour lists";
    return on_one_shard(db, nomem, [&](Shard& s) {
        return make_graph(out, nomem, [&](gsim_graph* g) { return neighbors(db, s, cutoff, metric, alpha, beta, row_begin, row_end, g); });
    });
}

int gsim_butina(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, uint32_t* cluster_of, uint32_t* centroids,
                uint64_t* nclusters)
{
    if (!indptr || !cluster_of || !centroids || !nclusters) return fail(GSIM_ERR_INVALID, "NULL argument");
    uint64_t nnz = 0;
    if (const int rc = check_csr_offsets(indptr, nrows, &nnz)) return rc;
    if (const int rc = check_csr_indices(indices, nnz, nrows)) return rc;
    try {
        // candidates: (neighbour count desc, row desc)
        std::vector<uint32_t> order(nrows);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            const uint64_t cx = indptr[x + 1] - indptr[x], cy = indptr[y + 1] - indptr[y];
            return cx != cy ? cx > cy : x > y;
        });
        std::vector<char> assigned(nrows, 0);
        uint32_t nc = 0;
        for (const uint32_t r : order) {
            if (assigned[r]) continue;
            assigned[r] = 1;
            cluster_of[r] = nc;
            centroids[nc] = r;
            for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++) {
                const uint32_t j = indices[e];
                if (!assigned[j]) {
                    assigned[j] = 1;
                    cluster_of[j] = nc;
                }
            }
            nc++;
        }
        *nclusters = nc;
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "butina");
    }
    return GSIM_OK;
}

} // extern "C"
