// capi_knn_join.cpp -- gsim_db_knn_join / gsim_db_knn_queries: for every left row its k most similar rows of the table, exactly,
// as CSR.  The family's argument checks, the plan (column segments and launches, gsim_db_knn's too) and one core that takes a
// front's LeftSide (capi_front.h), as the threshold joins; the lists become CSR in capi_pairs.cpp (build_knn_csr).  The device side
// is gsim_knn_join.hip (the two-table, segmented fold and the merge) and gsim_knn.hip's offsets and compaction.  The rule is stated
// in include/gpusim_hip.h.
#include "capi_front.h"

namespace gsim_host
{

// The column segments and the fold launches of a call over nl owner rows and N table rows of WP words on a device of num_cus
// compute units.
// Segments: the fold kernel's workgroups are (owner tile, segment).  S = 1 when the owner tiles alone give the device two
// workgroups per CU; otherwise S = ceil(2 x CUs / owner tiles), so that they do.  `segments` > 0 (GSIM_KNN_JOIN_SEGMENTS) is S
// instead.  Either way S is at most the table's column tiles and kKnnJoinMaxSegments, and 1 for 2^31 owners or more (the merge's
// grid).  Under the automatic rule the partial lists hold nl x S x k entries <= (2 x CUs + owner tiles) x 256 x k, i.e. less than
// 2 x (2 x CUs) x 256 x k x 8 bytes: 256 MiB at k = 128 on 256 CUs.
// Launches: the fold kernels' unit of parallelism is the (owner tile, segment) alone (a workgroup walks every candidate of its
// launch), so a launch takes as many owner tiles as the tile kernel's budget admits at one column tile per segment each
// (launch_tile_budget: the same pricing, the same 2.5e11 units) and as many columns PER SEGMENT as then still fit -- and never more
// columns than the budget gives ONE lane when it is spread over the device's 65 536 lanes, which bounds the launch of a small
// owner range, whose few waves walk alone.  `pairs` > 0 (GSIM_KNN_JOIN_LAUNCH_PAIRS, GSIM_KNN_LAUNCH_PAIRS) replaces both
// bounds: at most that many owner x candidate pairs over all segments, at least one column tile per segment.  A launch covers
// the rows [r0, r1) of every segment, counted from the segment's first row; the pieces of a group of owner tiles follow each
// other in ascending order.
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

// gsim_db_knn and gsim_db_mst: one segment, the whole table (the device's size then plays no part)
std::vector<KnnLaunch> plan_knn(uint64_t nout, uint64_t N, uint32_t WP, long long pairs)
{
    std::vector<KnnLaunch> out;
    for (const KnnJoinLaunch& l : plan_knn_join(nout, N, WP, 1, 1, pairs).launches) out.push_back({l.ot0, l.not_, l.r0, l.r1});
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

// the left rows (W words each, on s's device) against s's table
int knn_join(gsim_db* db, Shard& s, const LeftSide& ls, const KnnJoinCall& c, gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows, nl = ls.nl;
    const uint32_t k = c.k;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    g->kind = gsim_graph::Kind::kKnnJoin;
    gsim_knn_join_stats& ks = g->knn_join;
    ks.left_rows = nl;
    ks.table_rows = N;
    g->indptr.assign(nl + 1, 0);
    auto wall = [&] { return ms_since(t0); };
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
    DevBuf<uint32_t> part_len, merged_len;
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
    const uint32_t* lrows = ls.rows;
    if (WP != s.W) {
        if (ls.in_table) {
            lrows = table.rows() + ls.row0 * WP;
        } else {
            if (const int rc = left.alloc(nl, s.W, WP, "the k-nearest-neighbour join (popcounts of the left rows)", "the k-nearest-neighbour join (padded left rows)")) return rc;
            if (const int rc = left.prepare(ls.rows, nl, st)) return rc;
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

    EventPair ev_fold, ev_merge;
    GSIM_HIP(ev_fold.create());
    GSIM_HIP(ev_merge.create());
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
    KnnCsr csr;
    if (const int rc = build_knn_csr(db, s, S > 1 ? merged : parts, S > 1 ? merged_len : part_len, nl, k, tmp, d_indptr, ctl,
                                     "the k-nearest-neighbour join's CSR", "knn join", g, &csr))
        return rc;

    clocks.add(csr.ctl.data() + 2, nlaunch); // (read with the counters, in one copy)
    ks.segments = S;
    ks.fold_launches = nlaunch;
    ks.merge_launches = S > 1 ? 1 : 0;
    ks.pairs = nl * N;
    ks.inserts = csr.ctl[0];
    ks.partial_entries = S > 1 ? csr.ctl[1] : csr.total;
    ks.entries = csr.total;
    ks.kernel_ms = ev_fold.ms();
    ks.merge_ms = S > 1 ? ev_merge.ms() : 0.0;
    ks.csr_ms = csr.csr_ms;
    ks.d2h_ms = csr.d2h_ms;
    ks.clock_mhz = clocks.mhz();
    ks.wall_ms = wall();
    mirror_graph_stats(ks, ks.fold_launches + ks.merge_launches, ks.kernel_ms + ks.merge_ms, &g->stats);
    return GSIM_OK;
}

// what both entry points check before any device state
int check_knn_join_args(gsim_db* db, gsim_graph** out, uint64_t nl, const KnnJoinCall& c, uint32_t flags)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_k_cutoff("knn join", c.k, c.cutoff)) return rc;
    if (const int rc = check_metric("knn join", c.metric, c.alpha, c.beta)) return rc;
    if (flags & ~GSIM_KNN_EXCLUDE_SELF) return fail(GSIM_ERR_INVALID, "knn join: unknown flag bits");
    if (nl > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "knn join: 2^32 left rows or more");
    return check_tile_table(db, "knn join"); // (width first: the shared order)
}

int run_knn_join(gsim_db* db, const LeftSide& left, const KnnJoinCall& c, gsim_graph** out)
{
    return make_graph(out, "host memory for the k-nearest-neighbour join's lists",
                      [&](gsim_graph* g) { return knn_join(db, db->shards[0], left, c, g); });
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
    LeftSide left;
    rc = left.from_queries(db, queries, nq, "knn joins", "the k-nearest-neighbour join's left rows");
    if (rc != GSIM_OK) return rc;
    return run_knn_join(db, left, c, out);
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
    if (exclude && left && left != db) return fail(GSIM_ERR_INVALID, "knn join: GSIM_KNN_EXCLUDE_SELF needs left == db");
    rc = check_left_handle(db, left, lrow_end);
    if (rc != GSIM_OK) return rc;
    LeftSide ls;
    rc = ls.from_handle(db, left, lrow_begin, lrow_end, "knn joins");
    if (rc != GSIM_OK) return rc;
    return run_knn_join(db, ls, c, out);
}

int gsim_graph_get_knn_join_stats(const gsim_graph* g, gsim_knn_join_stats* out)
{
    if (!g || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (g->kind != gsim_graph::Kind::kKnnJoin) return fail(GSIM_ERR_INVALID, "not the result of gsim_db_knn_join / gsim_db_knn_queries");
    *out = g->knn_join;
    return GSIM_OK;
}

} // extern "C"
