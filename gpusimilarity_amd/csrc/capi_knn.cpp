// capi_knn.cpp -- gsim_db_knn: each row's k most similar other rows, exactly, as CSR.  The argument checks, the launch plan and the
// CSR build of a call; the device side is gsim_knn.hip (the fold kernel, offsets, compaction).  The rule is stated in
// include/gpusim_hip.h.
#include "capi_pairs.h"

#include <chrono>

namespace gsim_host
{

// The fold launches of a call over `not_total` owner tiles and N candidate rows of WP words.  The fold kernel's unit of
// parallelism is the owner tile alone (a workgroup walks every candidate of its launch), so a launch takes as many owner tiles as
// the tile kernel's budget admits at one column tile each (launch_tile_budget: the same pricing, the same 2.5e11 units) and as many
// column tiles as then still fit -- and never more columns than the budget gives ONE lane when it is spread over the device's
// 65 536 lanes, which bounds the launch of a small owner range, whose few waves walk alone.  `pairs` > 0 (GSIM_KNN_LAUNCH_PAIRS)
// replaces both bounds: at most that many owner x candidate pairs, at least one column tile.  The column pieces of a group of
// owner tiles follow each other in ascending order.
std::vector<KnnLaunch> plan_knn(uint64_t nout, uint64_t N, uint32_t WP, long long pairs)
{
    const uint64_t tile = gsim::kKnnTile, ctile = gsim::kKnnColTile;
    const uint64_t not_total = (nout + tile - 1) / tile;
    const uint64_t max_tiles = launch_tile_budget(WP);
    const uint64_t group = std::min<uint64_t>(std::min(not_total, max_tiles), 1u << 30);
    std::vector<KnnLaunch> out;
    for (uint64_t t0 = 0; t0 < not_total; t0 += group) {
        const uint64_t nt = std::min(group, not_total - t0);
        uint64_t cols;
        if (pairs > 0) {
            const uint64_t owners = std::min(nt * tile, nout - t0 * tile);
            cols = static_cast<uint64_t>(pairs) / owners / ctile * ctile;
        } else {
            cols = std::min(max_tiles / nt * ctile, max_tiles / ctile * ctile);
        }
        cols = std::max(cols, ctile);
        for (uint64_t c0 = 0; c0 < N; c0 += cols)
            out.push_back({static_cast<uint32_t>(t0), static_cast<uint32_t>(nt), c0, std::min(c0 + cols, N)});
    }
    return out;
}

namespace
{

int knn(gsim_db* db, Shard& s, uint32_t k, float cutoff, int metric, float alpha, float beta, uint64_t rb, uint64_t re, gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint64_t nout = re - rb;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    g->kind = gsim_graph::Kind::kKnn;
    g->knn.rows = nout;
    g->indptr.assign(nout + 1, 0);
    auto wall = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (nout == 0 || N < 2) {
        g->knn.wall_ms = g->stats.wall_ms = wall();
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const std::vector<KnnLaunch> plan = plan_knn(nout, N, WP, db->knobs.knn_launch_pairs);

    // popc of every row, and the rows zero-padded to WP words unless they already are WP words; the lists and their lengths
    // (one more length, zero: the scan's last output is the total); [0] the insert counter, then 4 clock stamps per launch
    PaddedRows table;
    DevBuf<> ctl, tmp;
    DevBuf<gsim::KnnEntry> lists;
    DevBuf<uint32_t> len, d_indices;
    DevBuf<float> d_scores;
    DevBuf<uint64_t> d_indptr;
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::knn_scan_bytes(nout + 1, &tmp_bytes));
    if (const int rc = table.alloc(N, s.W, WP, "the k-nearest-neighbour lists (popcounts)", "the k-nearest-neighbour lists (padded rows)")) return rc;
    GSIM_ALLOC(lists, nout * k * sizeof(gsim::KnnEntry), "the k-nearest-neighbour lists");
    GSIM_ALLOC(len, (nout + 1) * 4, "the k-nearest-neighbour lists (lengths)");
    GSIM_ALLOC(d_indptr, (nout + 1) * 8, "the k-nearest-neighbour lists (row offsets)");
    GSIM_ALLOC(ctl, (1 + 4 * plan.size()) * 8, "the k-nearest-neighbour lists (control block)");
    GSIM_ALLOC(tmp, tmp_bytes, "the k-nearest-neighbour lists (scan scratch)");
    unsigned long long* d_inserts = ctl.as<unsigned long long>();
    LaunchClocks clocks;
    clocks.view(d_inserts + 1);
    GSIM_HIP(hipMemsetAsync(len, 0, (nout + 1) * 4, st));
    GSIM_HIP(hipMemsetAsync(ctl, 0, (1 + 4 * plan.size()) * 8, st));
    if (const int rc = table.prepare(s.d_rows, N, st)) return rc;

    gsim::KnnArgs a{};
    a.rows = table.rows();
    a.pop = table.pop();
    a.nrows = N;
    a.row_begin = rb;
    a.row_end = re;
    a.WP = WP;
    a.k = k;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;
    a.lists = lists;
    a.len = len;
    a.inserts = d_inserts;

    EventPair ev_fold, ev_csr, ev_d2h;
    GSIM_HIP(ev_fold.create());
    GSIM_HIP(ev_csr.create());
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipEventRecord(ev_fold.a, st));
    for (size_t l = 0; l < plan.size(); l++) {
        a.clk = clocks.at(l);
        GSIM_HIP(gsim::launch_knn_fold(a, plan[l].ot0, plan[l].not_, plan[l].c0, plan[l].c1, st));
    }
    GSIM_HIP(hipEventRecord(ev_fold.b, st));

    // indptr on the device; its last entry sizes the compacted arrays
    GSIM_HIP(hipEventRecord(ev_csr.a, st));
    GSIM_HIP(gsim::launch_knn_offsets(tmp, tmp_bytes, len, nout + 1, d_indptr, st));
    std::vector<unsigned long long> h_ctl(1 + 4 * plan.size());
    GSIM_HIP(hipMemcpyAsync(g->indptr.data(), d_indptr, (nout + 1) * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(h_ctl.data(), ctl, h_ctl.size() * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    const uint64_t total = g->indptr[nout];
    if (total > nout * k) return fail(GSIM_ERR_STATE, "knn: the device reported impossible list lengths");
    GSIM_ALLOC(d_indices, total * 4, "the k-nearest-neighbour CSR");
    GSIM_ALLOC(d_scores, total * 4, "the k-nearest-neighbour CSR");
    GSIM_HIP(gsim::launch_knn_compact(lists, len, d_indptr, nout, k, db->row_base, d_indices, d_scores, st));
    GSIM_HIP(hipEventRecord(ev_csr.b, st));
    g->indices.resize(total);
    g->scores.resize(total);
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    if (total) {
        GSIM_HIP(hipMemcpyAsync(g->indices.data(), d_indices, total * 4, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipMemcpyAsync(g->scores.data(), d_scores, total * 4, hipMemcpyDeviceToHost, st));
    }
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st));

    clocks.add(h_ctl.data() + 1, plan.size()); // (read with the insert counter, in one copy)
    gsim_knn_stats& ks = g->knn;
    ks.launches = plan.size();
    ks.pairs = nout * N;
    ks.inserts = h_ctl[0];
    ks.entries = total;
    ks.kernel_ms = ev_fold.ms();
    // (the events of the CSR build span the host's look at the total: offsets, one small read, compaction)
    ks.csr_ms = ev_csr.ms();
    ks.d2h_ms = ev_d2h.ms();
    ks.clock_mhz = clocks.mhz();
    ks.wall_ms = wall();
    g->stats.launches = ks.launches;
    g->stats.pairs = total;
    g->stats.tile_ms = ks.kernel_ms;
    g->stats.csr_ms = ks.csr_ms;
    g->stats.d2h_ms = ks.d2h_ms;
    g->stats.clock_mhz = ks.clock_mhz;
    g->stats.wall_ms = ks.wall_ms;
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_knn(gsim_db* db, uint32_t k, float cutoff, int metric, float alpha, float beta, uint64_t row_begin, uint64_t row_end,
                gsim_graph** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (k < 1 || k > GSIM_KNN_MAX_K) return fail(GSIM_ERR_INVALID, "knn: k must be in [1, GSIM_KNN_MAX_K = 128]");
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, "knn: the cutoff must be in (0, 1]");
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (metric == GSIM_METRIC_TVERSKY && !(std::isfinite(alpha) && std::isfinite(beta) && alpha >= 0.0f && beta >= 0.0f))
        return fail(GSIM_ERR_INVALID, "knn: Tversky alpha and beta must be finite and >= 0");
    if (row_begin > row_end || row_end > db->nrows) return fail(GSIM_ERR_INVALID, "row range outside the table");
    if (db->fp_bits > 4096 || gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "knn: rows wider than 4096 bits");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "knn: tables of 2^32 rows or more");
    if (!db->finalized) return fail(GSIM_ERR_STATE, "table not finalized (no rows on a GPU)");
    if (db->shards.size() != 1) return fail(GSIM_ERR_STATE, "knn needs a single-shard handle");
    if (db->fold > 1) return fail(GSIM_ERR_STATE, "knn does not support folded tables");
    std::lock_guard<std::mutex> guard(db->search_mutex);
    gsim_graph* g = new (std::nothrow) gsim_graph;
    if (!g) return fail(GSIM_ERR_NOMEM, "graph");
    int rc;
    try {
        rc = knn(db, db->shards[0], k, cutoff, metric, alpha, beta, row_begin, row_end, g);
    } catch (const std::bad_alloc&) {
        rc = fail(GSIM_ERR_NOMEM, "host memory for the k-nearest-neighbour lists");
    }
    if (rc != GSIM_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return GSIM_OK;
}

} // extern "C"
