// capi_group.cpp -- gsim_db_search_group: exact top-k of the table by the MAX, MIN or MEAN of a row's scores against a set of
// queries.  The argument checks and the launch sequence of a call; the device side is gsim_group.hip (the scan, cut into
// launches; `which` behind the tail's rebuilt hits) and the four-kernel pipeline's own tail (capi_query.cpp enqueue_scan_tail).
// The rule is stated in include/gpusim_hip.h.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

// Every pair score has to lie in [0, 1]: alpha, beta >= 0 give den >= common in f32 (the header has the argument)
bool group_weights_ok(float alpha, float beta)
{
    return std::isfinite(alpha) && std::isfinite(beta) && alpha >= 0.0f && beta >= 0.0f && static_cast<double>(alpha) + static_cast<double>(beta) >= 1.0;
}

// Row x query pairs of one launch where GSIM_GROUP_LAUNCH_PAIRS is not set: a launch is bounded by its WORK, not by its pairs.
// Measured on an MI355X, a pair of the register kernels takes at most 0.11 ns x (W + 14) / 1000 -- the inner
// product's W word pairs plus the score, the reduction and the row's share of the offer -- so kGroupLaunchWork / (W + 14) pairs
// keep a launch at or under 5 ms at every specialised width.  The word loop (every lane reads its own row again for every query,
// W x 4 bytes apart from its neighbour's) is up to 19 times slower per pair: 1 / kGroupWordLoopCost of that.
constexpr uint64_t kGroupLaunchWork = 45000000000ull;
constexpr uint64_t kGroupPairOverhead = 14;
constexpr uint64_t kGroupWordLoopCost = 20;
uint64_t group_launch_pairs(const gsim_db* db, uint32_t W, bool word_loop)
{
    if (db->knobs.group_launch_pairs > 0) return static_cast<uint64_t>(db->knobs.group_launch_pairs);
    return kGroupLaunchWork / (W + kGroupPairOverhead) / (word_loop ? kGroupWordLoopCost : 1u);
}

int search_group(gsim_db* db, Shard& s, const uint32_t* queries, uint32_t nq, int mode, uint32_t kout, float cutoff, int metric, float alpha, float beta,
                 gsim_group_hit* hits, uint32_t* count, uint64_t* approx, gsim_group_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t k = static_cast<uint32_t>(std::min<uint64_t>(kout, s.nrows)); // (as gsim_db_search: never more hits than rows)
    *count = 0;
    if (approx) *approx = 0;
    if (st) st->queries = nq;
    if (s.nrows == 0) return GSIM_OK;
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;
    const gsim::ScanGeometry g = gsim::group_geometry(s.nrows, s.W, s.num_cus);
    int rc = ensure_subset_scratch(s, g);
    if (rc == GSIM_OK) rc = ensure_result_capacity(s, k);
    if (rc == GSIM_OK) rc = rezero_dirty_state(s);
    if (rc != GSIM_OK) return rc;

    // the call's queries (16-byte aligned rows when W % 4 == 0) and, behind them, their popcounts: in the shard's own buffer, which
    // only grows, so that a screening loop pays no allocation per call (the previous call has drained the stream before it returned)
    const size_t qwords = static_cast<size_t>(nq) * s.W;
    GSIM_ALLOC(s.d_gqueries, (qwords + nq) * 4, "the queries of a group search");
    GSIM_HIP(s.h_gqpop.grow(static_cast<size_t>(GSIM_GROUP_MAX_QUERIES) * 4));
    for (uint32_t q = 0; q < nq; q++) s.h_gqpop[q] = popcount_words(queries + static_cast<size_t>(q) * s.W, s.W);
    uint32_t* const d_q = s.d_gqueries;
    GSIM_HIP(hipMemcpyAsync(d_q, queries, qwords * 4, hipMemcpyHostToDevice, stream));
    GSIM_HIP(hipMemcpyAsync(d_q + qwords, s.h_gqpop, static_cast<size_t>(nq) * 4, hipMemcpyHostToDevice, stream));

    // (query / query_dev: the first query -- the tail's rebuilt hits read W words there; launch_group_which overwrites what they make of it)
    gsim::ScanArgs a = scan_args(s, queries, d_q, d_q, k, cutoff, metric, alpha, beta);
    gsim::GroupArgs ga{};
    ga.queries = d_q;
    ga.qpop = d_q + qwords;
    ga.nq = nq;
    ga.mode = mode;

    Event e0, e1, e2;
    if (st) {
        GSIM_HIP(e0.create());
        GSIM_HIP(e1.create());
        GSIM_HIP(e2.create());
        GSIM_HIP(hipEventRecord(e0, stream));
    }
    // The pass, cut into launches of at most group_launch_pairs row x query pairs (whole chunks, at least one)
    const bool specialised = s.W == 4 || s.W == 8 || s.W == 16 || s.W == 32 || s.W == 64; // (launch_group_scan's switch)
    const uint64_t pairs_per_launch = group_launch_pairs(db, s.W, !specialised);
    const uint64_t chunks_per_launch = std::max<uint64_t>(pairs_per_launch / nq / g.chunk_rows, 1u);
    uint64_t launches = 0;
    for (uint64_t c0 = 0; c0 < g.nchunks; c0 += chunks_per_launch) {
        ga.c0 = c0;
        ga.c1 = std::min(c0 + chunks_per_launch, g.nchunks);
        ga.first = c0 == 0 ? 1u : 0u;
        GSIM_HIP(gsim::launch_group_scan(a, g, ga, stream));
        launches++;
    }
    if (st) GSIM_HIP(hipEventRecord(e1, stream));
    const uint32_t row_base = db->row_base + static_cast<uint32_t>(s.first_row);
    rc = enqueue_scan_tail(db, s, a, g, row_base, s.nrows, s.d_result);
    if (rc != GSIM_OK) return rc;
    const bool large = k > static_cast<uint32_t>(gsim::kSelectCap);
    launches += 2 + (large ? 2 : 0); // compaction, select -- or the large-k select and the sort's two
    // `which` where the tail rebuilt the hits (always above kSelectCap; below it only behind heavy ties: decided on the device)
    // (group_which_kernel is a word loop at every width: one hit per thread)
    const uint64_t hits_per_launch = large ? std::max<uint64_t>(group_launch_pairs(db, s.W, true) / nq, 256u) : k;
    for (uint64_t h0 = 0; h0 < k; h0 += hits_per_launch) {
        GSIM_HIP(gsim::launch_group_which(a, ga, row_base, s.d_result, static_cast<uint32_t>(h0), static_cast<uint32_t>(std::min<uint64_t>(h0 + hits_per_launch, k)), stream));
        launches++;
    }
    if (st) GSIM_HIP(hipEventRecord(e2, stream));
    GSIM_HIP(hipMemcpyAsync(s.h_result, s.d_result, gsim_result_block_bytes(k), hipMemcpyDeviceToHost, stream));
    rc = wait_stream(stream);
    if (rc != GSIM_OK) return rc;
    const gsim_result_header* h = s.h_result.as<const gsim_result_header>();
    const uint32_t n = std::min(h->count, k);
    std::memcpy(hits, h + 1, sizeof(gsim_group_hit) * n);
    *count = n;
    if (approx) *approx = h->approx;
    if (st) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) st->scan_ms = ms;
        if (hipEventElapsedTime(&ms, e0, e2) == hipSuccess) st->kernel_ms = ms;
        st->launches = launches;
        st->pairs = s.nrows * nq;
        st->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_search_group(gsim_db* db, const uint32_t* queries, uint32_t nq, int mode, uint32_t k, float cutoff, int metric, float alpha, float beta,
                         gsim_group_hit* hits, uint32_t* count, uint64_t* approx, gsim_group_stats* stats)
{
    static_assert(sizeof(gsim_group_hit) == sizeof(gsim_hit) && sizeof(gsim_group_hit) == 12, "a group hit has gsim_hit's layout");
    if (stats) *stats = gsim_group_stats{};
    if (!db || !queries || !hits || !count) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nq == 0) return fail(GSIM_ERR_INVALID, "group search: no queries");
    if (nq > GSIM_GROUP_MAX_QUERIES) return fail(GSIM_ERR_INVALID, "group search: more than " + std::to_string(GSIM_GROUP_MAX_QUERIES) + " queries");
    if (mode != GSIM_GROUP_MAX && mode != GSIM_GROUP_MIN && mode != GSIM_GROUP_MEAN) return fail(GSIM_ERR_INVALID, "unknown group mode");
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (metric == GSIM_METRIC_TVERSKY && !group_weights_ok(alpha, beta))
        return fail(GSIM_ERR_INVALID, "group search: Tversky needs finite alpha >= 0, beta >= 0 and alpha + beta >= 1 (pair scores within [0, 1])");
    if (db->fp_bits > 4096) return fail(GSIM_ERR_INVALID, "group search: rows wider than 4096 bits");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "group search: tables of 2^32 rows or more");
    if (const int rc = check_table_state(db, "group searches", true)) return rc;
    return on_one_shard(db, "host memory for a group search", [&](Shard& s) {
        return search_group(db, s, queries, nq, mode, k, cutoff, metric, alpha, beta, hits, count, approx, stats);
    });
}

} // extern "C"
