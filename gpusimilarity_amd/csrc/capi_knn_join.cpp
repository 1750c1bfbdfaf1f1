// capi_knn_join.cpp -- gsim_db_knn_join / gsim_db_knn_queries: for every left row its k most similar rows of the table, exactly,
// as CSR.  Two thin fronts of one core that takes "left rows in device memory, nl of them", as the threshold joins; the argument
// checks, the plan (column segments and launches) and the CSR build of a call.  The device side is gsim_knn_join.hip (the
// two-table, segmented fold and the merge) and gsim_knn.hip's offsets and compaction.  The rule is stated in include/gpusim_hip.h.
#include "capi_pairs.h"

#include <chrono>
#include <cmath>

namespace gsim_host
{

// The column segments and the fold launches of a call over nl owner rows and N table rows of WP words on a device of num_cus
// compute units.
// Segments: the fold kernel's workgroups are (owner tile, segment).  S = 1 when the owner tiles alone give the device two
// workgroups per CU; otherwise S = ceil(2 x CUs / owner tiles), so that they do.  `segments` > 0 (GSIM_KNN_JOIN_SEGMENTS) is S
// instead.  Either way S is at most the table's column tiles and kKnnJoinMaxSegments, and 1 for 2^31 owners or more (the merge's
// grid).  Under the automatic rule the partial lists hold nl x S x k entries <= (2 x CUs + owner tiles) x 256 x k, i.e. less than
// 2 x (2 x CUs) x 256 x k x 8 bytes: 256 MiB at k = 128 on 256 CUs.
// Launches: plan_knn's, with a workgroup per (owner tile, segment) where plan_knn has one per owner tile -- as many owner
// tiles as the tile budget admits at one column tile per segment each, as many columns PER SEGMENT as then still fit, never more
// than the budget gives one lane when it is spread over the device's 65 536 lanes; `pairs` > 0 (GSIM_KNN_JOIN_LAUNCH_PAIRS)
// replaces both bounds: at most that many owner x candidate pairs over all segments, at least one column tile per segment.  A
// launch covers the rows [r0, r1) of every segment, counted from the segment's first row; the pieces of a group of owner tiles
// follow each other in ascending order.  With S == 1 this is plan_knn.
KnnJoinPlan plan_knn_join(uint64_t nl, uint64_t N, uint32_t WP, int num_cus, int segments, long long pairs)
{
    const uint64_t tile = gsim::kKnnTile, ctile = gsim::kKnnColTile;
    const uint64_t not_total = (nl + tile - 1) / tile, nct = (N + ctile - 1) / ctile;
    const uint64_t want = 2u * static_cast<uint64_t>(std::max(num_cus, 1));
    uint64_t S = segments > 0 ? static_cast<uint64_t>(segments) : not_total >= want || not_total == 0 ? 1 : (want + not_total - 1) / not_total;
    S = std::max<uint64_t>(std::min(std::min(S, nct), static_cast<uint64_t>(gsim::kKnnJoinMaxSegments)), 1);
    if (nl > 0x7FFFFFFFull) S = 1;
    KnnJoinPlan out;
    out.segments = static_cast<uint32_t>(S);
    const uint64_t seg_rows = gsim::knn_join_seg_begin(1, S, N); // the longest segment: segment 0
    const uint64_t max_tiles = launch_tile_budget(WP);
    const uint64_t group = std::min<uint64_t>(std::min(not_total, std::max<uint64_t>(max_tiles / S, 1)), 1u << 30);
    for (uint64_t t0 = 0; t0 < not_total; t0 += group) {
        const uint64_t nt = std::min(group, not_total - t0);
        uint64_t cols;
        if (pairs > 0) {
            const uint64_t owners = std::min(nt * tile, nl - t0 * tile);
            cols = static_cast<uint64_t>(pairs) / owners / S / ctile * ctile;
        } else {
            cols = std::min(max_tiles / (nt * S) * ctile, max_tiles / ctile * ctile);
        }
        cols = std::max(cols, ctile);
        for (uint64_t r0 = 0; r0 < seg_rows; r0 += cols)
            out.launches.push_back({static_cast<uint32_t>(t0), static_cast<uint32_t>(nt), r0, std::min(r0 + cols, seg_rows)});
    }
    return out;
}

namespace
{

struct KnnJoinCall {
    uint32_t k;
    float cutoff;
    int metric;
    float alpha, beta;
    uint64_t self0; // GSIM_KNN_EXCLUDE_SELF: left row o is table row self0 + o; ~0: no pair is excluded
};

// left rows d_left[0 .. nl) (W words each, on s's device; `left_in_table`: they are the table's own rows left_row0 ...) against s's table
int knn_join(gsim_db* db, Shard& s, const uint32_t* d_left, uint64_t nl, bool left_in_table, uint64_t left_row0, const KnnJoinCall& c,
             gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint32_t k = c.k;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    g->kind = gsim_graph::Kind::kKnnJoin;
    gsim_knn_join_stats& ks = g->knn_join;
    ks.left_rows = nl;
    ks.table_rows = N;
    g->indptr.assign(nl + 1, 0);
    auto wall = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (nl == 0 || N == 0) {
        ks.wall_ms = g->stats.wall_ms = wall();
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const KnnJoinPlan plan = plan_knn_join(nl, N, WP, s.num_cus, db->knobs.knn_join_segments, db->knobs.knn_join_launch_pairs);
    const uint64_t S = plan.segments;
    const size_t nlaunch = plan.launches.size();

    // popc of every table row, and the rows of either side zero-padded to WP words unless they already are WP words; the partial
    // lists and their lengths; with more than one segment the final lists and theirs (one more length, zero: the scan's last
    // output is the total); [0] the insert counter, [1] the entries of the partial lists, then 4 clock stamps per launch
    PaddedRows table, left;
    DevBuf<> ctl, tmp;
    DevBuf<gsim::KnnEntry> parts, merged;
    DevBuf<uint32_t> part_len, merged_len, d_indices;
    DevBuf<float> d_scores;
    DevBuf<uint64_t> d_indptr;
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::knn_scan_bytes(nl + 1, &tmp_bytes));
    if (const int rc = table.alloc(N, s.W, WP, "the k-nearest-neighbour join (popcounts)", "the k-nearest-neighbour join (padded rows)")) return rc;
    GSIM_ALLOC(parts, nl * S * k * sizeof(gsim::KnnEntry), "the k-nearest-neighbour join's lists");
    GSIM_ALLOC(part_len, (nl * S + 1) * 4, "the k-nearest-neighbour join's lists (lengths)");
    if (S > 1) {
        GSIM_ALLOC(merged, nl * k * sizeof(gsim::KnnEntry), "the k-nearest-neighbour join's merged lists");
        GSIM_ALLOC(merged_len, (nl + 1) * 4, "the k-nearest-neighbour join's merged lists (lengths)");
    }
    GSIM_ALLOC(d_indptr, (nl + 1) * 8, "the k-nearest-neighbour join's lists (row offsets)");
    GSIM_ALLOC(ctl, (2 + 4 * nlaunch) * 8, "the k-nearest-neighbour join's lists (control block)");
    GSIM_ALLOC(tmp, tmp_bytes, "the k-nearest-neighbour join's lists (scan scratch)");
    unsigned long long* d_ctl = ctl.as<unsigned long long>();
    LaunchClocks clocks;
    clocks.view(d_ctl + 2);
    GSIM_HIP(hipMemsetAsync(part_len, 0, (nl * S + 1) * 4, st));
    if (S > 1) GSIM_HIP(hipMemsetAsync(merged_len, 0, (nl + 1) * 4, st));
    GSIM_HIP(hipMemsetAsync(ctl, 0, (2 + 4 * nlaunch) * 8, st));
    if (const int rc = table.prepare(s.d_rows, N, st)) return rc;
    // (the kernel counts the left rows' bits itself: only their padded copy is wanted, where the table's does not hold them)
    const uint32_t* lrows = d_left;
    if (WP != s.W) {
        if (left_in_table) {
            lrows = table.rows() + left_row0 * WP;
        } else {
            if (const int rc = left.alloc(nl, s.W, WP, "the k-nearest-neighbour join (popcounts of the left rows)", "the k-nearest-neighbour join (padded left rows)")) return rc;
            if (const int rc = left.prepare(d_left, nl, st)) return rc;
            lrows = left.rows();
        }
    }

    gsim::KnnJoinArgs a{};
    a.rows = table.rows();
    a.pop = table.pop();
    a.nrows = N;
    a.lrows = lrows;
    a.nl = nl;
    a.self0 = c.self0;
    a.WP = WP;
    a.k = k;
    a.nseg = static_cast<uint32_t>(S);
    a.metric = c.metric;
    a.alpha = c.alpha;
    a.beta = c.beta;
    a.cutoff = c.cutoff;
    a.lists = parts;
    a.len = part_len;
    a.inserts = d_ctl;

    EventPair ev_fold, ev_merge, ev_csr, ev_d2h;
    GSIM_HIP(ev_fold.create());
    GSIM_HIP(ev_merge.create());
    GSIM_HIP(ev_csr.create());
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipEventRecord(ev_fold.a, st));
    for (size_t l = 0; l < nlaunch; l++) {
        const KnnJoinLaunch& p = plan.launches[l];
        a.clk = clocks.at(l);
        GSIM_HIP(gsim::launch_knn_join_fold(a, p.ot0, p.not_, p.r0, p.r1, st));
    }
    GSIM_HIP(hipEventRecord(ev_fold.b, st));
    // one segment: the partial lists are the final lists
    GSIM_HIP(hipEventRecord(ev_merge.a, st));
    if (S > 1) GSIM_HIP(gsim::launch_knn_join_merge(parts, part_len, nl, a.nseg, k, merged, merged_len, d_ctl + 1, st));
    GSIM_HIP(hipEventRecord(ev_merge.b, st));
    const gsim::KnnEntry* lists = S > 1 ? merged : parts;
    const uint32_t* len = S > 1 ? merged_len : part_len;

    // indptr on the device; its last entry sizes the compacted arrays
    GSIM_HIP(hipEventRecord(ev_csr.a, st));
    GSIM_HIP(gsim::launch_knn_offsets(tmp, tmp_bytes, len, nl + 1, d_indptr, st));
    std::vector<unsigned long long> h_ctl(2 + 4 * nlaunch);
    GSIM_HIP(hipMemcpyAsync(g->indptr.data(), d_indptr, (nl + 1) * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(h_ctl.data(), ctl, h_ctl.size() * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    const uint64_t total = g->indptr[nl];
    if (total > nl * k) return fail(GSIM_ERR_STATE, "knn join: the device reported impossible list lengths");
    GSIM_ALLOC(d_indices, total * 4, "the k-nearest-neighbour join's CSR");
    GSIM_ALLOC(d_scores, total * 4, "the k-nearest-neighbour join's CSR");
    GSIM_HIP(gsim::launch_knn_compact(lists, len, d_indptr, nl, k, db->row_base, d_indices, d_scores, st));
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

    clocks.add(h_ctl.data() + 2, nlaunch); // (read with the counters, in one copy)
    ks.segments = S;
    ks.fold_launches = nlaunch;
    ks.merge_launches = S > 1 ? 1 : 0;
    ks.pairs = nl * N;
    ks.inserts = h_ctl[0];
    ks.partial_entries = S > 1 ? h_ctl[1] : total;
    ks.entries = total;
    ks.kernel_ms = ev_fold.ms();
    ks.merge_ms = S > 1 ? ev_merge.ms() : 0.0;
    // (the events of the CSR build span the host's look at the total: offsets, one small read, compaction)
    ks.csr_ms = ev_csr.ms();
    ks.d2h_ms = ev_d2h.ms();
    ks.clock_mhz = clocks.mhz();
    ks.wall_ms = wall();
    g->stats.launches = ks.fold_launches + ks.merge_launches;
    g->stats.pairs = total;
    g->stats.tile_ms = ks.kernel_ms + ks.merge_ms;
    g->stats.csr_ms = ks.csr_ms;
    g->stats.d2h_ms = ks.d2h_ms;
    g->stats.clock_mhz = ks.clock_mhz;
    g->stats.wall_ms = ks.wall_ms;
    return GSIM_OK;
}

// what both entry points check before any device state
int check_knn_join_args(gsim_db* db, gsim_graph** out, uint64_t nl, const KnnJoinCall& c, uint32_t flags)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (c.k < 1 || c.k > GSIM_KNN_MAX_K) return fail(GSIM_ERR_INVALID, "knn join: k must be in [1, GSIM_KNN_MAX_K = 128]");
    if (!(c.cutoff > 0.0f && c.cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, "knn join: the cutoff must be in (0, 1]");
    if (c.metric != GSIM_METRIC_TANIMOTO && c.metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (c.metric == GSIM_METRIC_TVERSKY && !(std::isfinite(c.alpha) && std::isfinite(c.beta) && c.alpha >= 0.0f && c.beta >= 0.0f))
        return fail(GSIM_ERR_INVALID, "knn join: Tversky alpha and beta must be finite and >= 0");
    if (flags & ~GSIM_KNN_EXCLUDE_SELF) return fail(GSIM_ERR_INVALID, "knn join: unknown flag bits");
    if (nl > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "knn join: 2^32 left rows or more");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "knn join: tables of 2^32 rows or more");
    if (db->fp_bits > 4096 || gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "knn join: rows wider than 4096 bits");
    return GSIM_OK;
}

int check_knn_join_state(const gsim_db* db, const char* which)
{
    if (!db->finalized) return fail(GSIM_ERR_STATE, std::string(which) + " not finalized (no rows on a GPU)");
    if (db->shards.size() != 1) return fail(GSIM_ERR_STATE, std::string("knn joins need single-shard handles: ") + which);
    if (db->fold > 1) return fail(GSIM_ERR_STATE, std::string("knn joins do not support folded tables: ") + which);
    return GSIM_OK;
}

int run_knn_join(gsim_db* db, const uint32_t* d_left, uint64_t nl, bool left_in_table, uint64_t left_row0, const KnnJoinCall& c, gsim_graph** out)
{
    gsim_graph* g = new (std::nothrow) gsim_graph;
    if (!g) return fail(GSIM_ERR_NOMEM, "graph");
    int rc;
    try {
        rc = knn_join(db, db->shards[0], d_left, nl, left_in_table, left_row0, c, g);
    } catch (const std::bad_alloc&) {
        rc = fail(GSIM_ERR_NOMEM, "host memory for the k-nearest-neighbour join's lists");
    }
    if (rc != GSIM_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_knn_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, uint32_t k, float cutoff, int metric, float alpha, float beta,
                        gsim_graph** out)
{
    const KnnJoinCall c{k, cutoff, metric, alpha, beta, ~0ull};
    int rc = check_knn_join_args(db, out, nq, c, 0);
    if (rc != GSIM_OK) return rc;
    if (nq && !queries) return fail(GSIM_ERR_INVALID, "NULL queries");
    rc = check_knn_join_state(db, "table");
    if (rc != GSIM_OK) return rc;
    std::lock_guard<std::mutex> guard(db->search_mutex);
    Shard& s = db->shards[0];
    DevBuf<> d_left;
    if (nq) {
        GSIM_HIP(set_device(s.device));
        const size_t bytes = static_cast<size_t>(nq) * s.W * 4;
        GSIM_ALLOC(d_left, bytes, "the k-nearest-neighbour join's left rows");
        GSIM_HIP(hipMemcpyAsync(d_left, queries, bytes, hipMemcpyHostToDevice, s.stream));
    }
    return run_knn_join(db, d_left.as<uint32_t>(), nq, false, 0, c, out);
}

int gsim_db_knn_join(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint32_t k, float cutoff, int metric, float alpha,
                     float beta, uint32_t flags, gsim_graph** out)
{
    if (lrow_begin > lrow_end) {
        if (out) *out = nullptr;
        return fail(GSIM_ERR_INVALID, "left row range: begin past end");
    }
    const bool exclude = (flags & GSIM_KNN_EXCLUDE_SELF) != 0;
    const KnnJoinCall c{k, cutoff, metric, alpha, beta, exclude ? lrow_begin : ~0ull};
    int rc = check_knn_join_args(db, out, lrow_end - lrow_begin, c, flags);
    if (rc != GSIM_OK) return rc;
    if (!left) return fail(GSIM_ERR_INVALID, "NULL left handle");
    if (exclude && left != db) return fail(GSIM_ERR_INVALID, "knn join: GSIM_KNN_EXCLUDE_SELF needs left == db");
    if (lrow_end > left->nrows) return fail(GSIM_ERR_INVALID, "left row range outside the left table");
    if (left->fp_bits != db->fp_bits) return fail(GSIM_ERR_INVALID, "the two handles have different fp_bits");
    rc = check_knn_join_state(db, "table");
    if (rc == GSIM_OK && left != db) rc = check_knn_join_state(left, "left table");
    if (rc != GSIM_OK) return rc;
    if (left->shards[0].device != db->shards[0].device) return fail(GSIM_ERR_STATE, "the two handles are on different devices");
    // one call at a time on either handle
    std::unique_lock<std::mutex> g1(db->search_mutex, std::defer_lock), g2(left->search_mutex, std::defer_lock);
    if (left != db) std::lock(g1, g2);
    else g1.lock();
    const uint32_t* d_left = static_cast<const uint32_t*>(left->shards[0].d_rows) + lrow_begin * left->shards[0].W;
    return run_knn_join(db, d_left, lrow_end - lrow_begin, left == db, lrow_begin, c, out);
}

int gsim_graph_get_knn_join_stats(const gsim_graph* g, gsim_knn_join_stats* out)
{
    if (!g || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (g->kind != gsim_graph::Kind::kKnnJoin) return fail(GSIM_ERR_INVALID, "not the result of gsim_db_knn_join / gsim_db_knn_queries");
    *out = g->knn_join;
    return GSIM_OK;
}

} // extern "C"
