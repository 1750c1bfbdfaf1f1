// capi_popindex.cpp -- popcount indexes (gsim_popindex_*) and gsim_db_search_bounded: gsim_db_search's answer from a window of the
// table's popcount order.  The index's lifecycle, the argument checks, the windows and the two-stage driver of a query; the device
// side is gsim_popindex.hip (the build's kernels, the bound table, the window scan), gsim_subset.hip's gather for an index without
// the copy of the rows, and the four-kernel pipeline's own scan and tail (capi_query.cpp).  The bound on the host is
// capi_popindex_host.cpp.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 34.
#include "capi_front.h"

#include <map>

namespace gsim_host
{
namespace
{

// bits that hold every popcount of rows of fp_bits bits: the radix sort's key width
uint32_t popcount_key_bits(uint32_t fp_bits)
{
    uint32_t bits = 1;
    while ((1u << bits) <= fp_bits) bits++;
    return bits;
}

int build_popindex(gsim_db* db, uint32_t flags, gsim_popindex* ix)
{
    Shard& s = db->shards[0];
    const uint64_t N = s.nrows;
    const uint32_t nbins = db->fp_bits + 1;
    ix->owner = db;
    ix->device = s.device;
    ix->nrows = N;
    ix->fp_bits = db->fp_bits;
    ix->row_base = db->row_base;
    ix->flags = flags;
    ix->first.assign(static_cast<size_t>(nbins) + 1, 0);
    if (N == 0) return GSIM_OK;
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    DevBuf<uint16_t> d_popc, d_popc2; // (the build's temporaries are freed on return)
    DevBuf<uint32_t> d_hist, d_first;
    DevBuf<> d_tmp;
    GSIM_ALLOC(ix->d_order, N * 4, "the popcount index's order");
    GSIM_ALLOC(d_popc, N * 2, "the popcount index's popcounts");
    GSIM_ALLOC(d_popc2, N * 2, "the popcount index's sorted popcounts");
    GSIM_ALLOC(d_hist, (static_cast<size_t>(nbins) + 1) * 4, "the popcount index's histogram");
    GSIM_ALLOC(d_first, (static_cast<size_t>(nbins) + 1) * 4, "the popcount index's bucket starts");
    const uint32_t key_bits = popcount_key_bits(db->fp_bits);
    size_t sort_bytes = 0, scan_bytes = 0;
    GSIM_HIP(gsim::popindex_sort_bytes(N, key_bits, &sort_bytes));
    GSIM_HIP(gsim::scan_u32_bytes(static_cast<uint64_t>(nbins) + 1, &scan_bytes));
    GSIM_ALLOC(d_tmp, std::max(sort_bytes, scan_bytes), "the popcount index's sort");
    GSIM_HIP(hipMemsetAsync(d_hist, 0, (static_cast<size_t>(nbins) + 1) * 4, st));
    GSIM_HIP(gsim::launch_popindex_popc(s.d_rows, N, s.W, d_popc, d_hist, s.num_cus, st));
    GSIM_HIP(gsim::launch_scan_u32(d_tmp, scan_bytes, d_hist, d_first, static_cast<uint64_t>(nbins) + 1, st));
    std::vector<uint32_t> h_first(static_cast<size_t>(nbins) + 1);
    GSIM_HIP(hipMemcpyAsync(h_first.data(), d_first, h_first.size() * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(gsim::launch_popindex_sort(d_tmp, sort_bytes, d_popc, d_popc2, ix->d_order, N, key_bits, st));
    if (flags & GSIM_POPINDEX_ROWS) {
        GSIM_ALLOC(ix->d_rows, static_cast<size_t>(N) * s.W * 4, "the popcount index's copy of the rows");
        GSIM_HIP(gsim::launch_lsum_gather(static_cast<const uint32_t*>(s.d_rows), s.W, s.W, ix->d_order, N, ix->d_rows, st));
    }
    GSIM_HIP(hipStreamSynchronize(st));
    for (size_t b = 0; b < h_first.size(); b++) ix->first[b] = h_first[b];
    if (ix->first[nbins] != N) return fail(GSIM_ERR_STATE, "popcount index: the device reported an impossible count");
    return GSIM_OK;
}

// ---- the rule's host half: windows over the buckets [b0, b1] (inclusive; b0 > b1: none) ----

struct Hull {
    uint32_t b0 = 1, b1 = 0;
    bool empty() const { return b0 > b1; }
    void take(uint32_t b)
    {
        if (empty()) b0 = b1 = b;
        else b0 = std::min(b0, b), b1 = std::max(b1, b);
    }
    bool operator==(const Hull& o) const { return b0 == o.b0 && b1 == o.b1; }
};

struct Window {
    const gsim_popindex* ix;
    uint64_t lo(const Hull& h) const { return h.empty() ? 0 : ix->first[h.b0]; }
    uint64_t rows(const Hull& h) const { return h.empty() ? 0 : ix->first[h.b1 + 1] - ix->first[h.b0]; }
};

// the hull of the buckets of `in` whose bound is at least t
Hull hull_at_least(const float* ub, const Hull& in, float t)
{
    Hull h;
    for (uint32_t b = in.b0; !in.empty() && b <= in.b1; b++)
        if (ub[b] >= t) h.take(b);
    return h;
}

// stage 1: the smallest hull of the window's buckets, taken in (ub descending, b ascending) order, that holds at least `target` rows
Hull stage1_hull(const float* ub, const Hull& window, const Window& w, uint64_t target, std::vector<uint32_t>& by_ub)
{
    by_ub.clear();
    for (uint32_t b = window.b0; b <= window.b1; b++) by_ub.push_back(b);
    std::stable_sort(by_ub.begin(), by_ub.end(), [&](uint32_t x, uint32_t y) { return ub[x] > ub[y]; });
    Hull h;
    for (const uint32_t b : by_ub) {
        h.take(b);
        if (w.rows(h) >= target) break;
    }
    return h;
}

// Tversky weights for which every score lies in [0, 1] (gsim_db_search_group's condition)
bool unit_scores(int metric, float alpha, float beta)
{
    if (metric != GSIM_METRIC_TVERSKY) return true;
    return std::isfinite(alpha) && std::isfinite(beta) && alpha >= 0.0f && beta >= 0.0f && static_cast<double>(alpha) + static_cast<double>(beta) >= 1.0;
}

enum class ScanRoute { kStream, kGather, kPlain };

struct BoundedCall {
    gsim_db* db;
    Shard& s;
    const gsim_popindex* ix;
    uint32_t k;
    float cutoff;
    int metric;
    float alpha, beta;
    gsim_popindex_stats* st;
    EventPair ev;

    ScanRoute route(uint64_t n) const
    {
        if (ix->flags & GSIM_POPINDEX_ROWS) return n * 4 <= s.nrows * 3 ? ScanRoute::kStream : ScanRoute::kPlain;
        return subset_gather_applies(db, s, n) ? ScanRoute::kGather : ScanRoute::kPlain;
    }

    // One scan and its tail: the slots [lo, lo + n) of the order (n >= 1), or the whole table; waits for the block in s.h_result.
    int scan(ScanRoute r, const uint32_t* query, uint32_t* dq, uint64_t lo, uint64_t n)
    {
        const hipStream_t stream = s.stream;
        const uint32_t kk = static_cast<uint32_t>(std::min<uint64_t>(k, r == ScanRoute::kPlain ? s.nrows : n)); // (never more hits than rows offered)
        const gsim::ScanGeometry g = r == ScanRoute::kPlain    ? s.geo
                                     : r == ScanRoute::kStream ? gsim::popindex_scan_geometry(n, s.W, s.num_cus)
                                                               : gsim::subset_gather_geometry(n, s.W, s.num_cus);
        // (a.rows, a.nrows stay the table's: the tail rebuilds hits from it)
        const auto enqueue = [&](gsim::ScanArgs& a, uint32_t& launches) {
            bool sampled = false;
            if (r == ScanRoute::kPlain) { // the four-kernel pipeline as the ordinary search enqueues it, seed included
                GSIM_HIP(gsim::launch_sample(a, g, 4, stream, &sampled));
                GSIM_HIP(gsim::launch_scan(a, g, stream));
            } else if (r == ScanRoute::kStream) { // no seed: gtau starts at 0
                gsim::ScanArgs w = a;
                w.rows = ix->d_rows;
                GSIM_HIP(gsim::launch_popindex_scan(w, g, ix->d_order, lo, static_cast<uint32_t>(n), stream));
            } else {
                GSIM_HIP(gsim::launch_subset_gather(a, g, ix->d_order + lo, static_cast<uint32_t>(n), stream));
            }
            launches += sampled ? 2u : 1u;
            return static_cast<int>(GSIM_OK);
        };
        ScanStepCost cost;
        // (the tail reads the same copy of the query)
        const int rc = run_restricted_scan(db, s, scan_args(s, query, dq, dq, kk, cutoff, metric, alpha, beta), g, s.nrows, st ? &ev : nullptr, enqueue, &cost);
        if (rc != GSIM_OK) return rc;
        if (st) {
            st->kernel_ms += cost.kernel_ms;
            st->launches += cost.launches;
            st->rows_scanned += r == ScanRoute::kPlain ? s.nrows : n;
        }
        return GSIM_OK;
    }
};

int search_bounded(gsim_db* db, Shard& s, const gsim_popindex* ix, const uint32_t* queries, uint32_t nq, uint32_t kout, float cutoff, int metric,
                   float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx, gsim_popindex_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint32_t F = ix->fp_bits;
    BoundedCall call{db, s, ix, static_cast<uint32_t>(std::min<uint64_t>(kout, N)), cutoff, metric, alpha, beta, st, {}};
    for (uint32_t q = 0; q < nq; q++) {
        counts[q] = 0;
        if (approx) approx[q] = 0;
    }
    if (N == 0 || nq == 0) {
        if (st) st->queries_one_stage = nq, st->wall_ms = ms_since(t0);
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;
    int rc = rezero_dirty_state(s);
    if (rc != GSIM_OK) return rc;
    // the call's queries (16-byte aligned rows when W % 4 == 0) and the bound table: in the shard's own buffers, which only grow, so that
    // a screening loop pays no allocation per call (only this call uses them, and it has drained the stream before it returned)
    DevBuf<uint32_t>& d_q = s.d_pqueries;
    DevBuf<float>& d_ub = s.d_pbounds;
    HostBuf<float>& h_ub = s.h_pbounds;
    GSIM_ALLOC(d_q, static_cast<size_t>(nq) * s.W * 4, "the queries of a bounded search");
    GSIM_ALLOC(d_ub, (static_cast<size_t>(F) + 1) * 4, "the bound table of a bounded search");
    GSIM_HIP(h_ub.grow((static_cast<size_t>(F) + 1) * 4));
    GSIM_HIP(hipMemcpyAsync(d_q, queries, static_cast<size_t>(nq) * s.W * 4, hipMemcpyHostToDevice, stream));
    EventPair evb;
    if (st) {
        GSIM_HIP(call.ev.create());
        GSIM_HIP(evb.create());
    }
    std::map<uint32_t, std::vector<float>> tables; // the bound table of every query popcount met so far
    std::vector<uint32_t> by_ub;
    const Window w{ix};
    const bool narrow_ok = call.k >= 1 && (cutoff <= 0.0f || !approx) && unit_scores(metric, alpha, beta);
    const uint64_t target = std::max<uint64_t>(static_cast<uint64_t>(call.k) * 4u, 4096u);
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t* query = queries + static_cast<size_t>(q) * s.W;
        uint32_t* dq = d_q + static_cast<size_t>(q) * s.W;
        const uint32_t qa = popcount_words(query, s.W);
        auto it = tables.find(qa);
        if (it == tables.end()) {
            if (st) GSIM_HIP(hipEventRecord(evb.a, stream));
            GSIM_HIP(gsim::launch_popindex_bounds(F, qa, metric, alpha, beta, d_ub, stream));
            GSIM_HIP(hipMemcpyAsync(h_ub, d_ub, (static_cast<size_t>(F) + 1) * 4, hipMemcpyDeviceToHost, stream));
            if (st) GSIM_HIP(hipEventRecord(evb.b, stream));
            rc = wait_stream(stream);
            if (rc != GSIM_OK) return rc;
            it = tables.emplace(qa, std::vector<float>(static_cast<const float*>(h_ub), static_cast<const float*>(h_ub) + F + 1)).first;
            if (st) st->bounds_ms += evb.ms(), st->launches += 1;
        }
        const float* ub = it->second.data();
        Hull all;
        all.b0 = 0, all.b1 = F;
        const Hull window = cutoff > 0.0f ? hull_at_least(ub, all, cutoff) : all;
        if (st) st->rows_window += w.rows(window);
        gsim_hit* out = hits + static_cast<size_t>(q) * kout;
        // what a scan left in the pinned block becomes the query's answer
        auto take = [&]() {
            const uint32_t n = take_scan_result(s, call.k, out, &counts[q], approx ? &approx[q] : nullptr);
            if (approx && !(cutoff > 0.0f)) approx[q] = N; // (the tail reports the rows it was told of: the table's)
            return n;
        };
        if (w.rows(window) == 0) { // no row can reach the cutoff (or none has such a popcount): zero hits, approx 0, no launch
            if (st) st->queries_one_stage++;
            continue;
        }
        const bool narrow = narrow_ok && w.rows(window) > target;
        Hull h1 = narrow ? stage1_hull(ub, window, w, target, by_ub) : window;
        ScanRoute r = call.route(w.rows(h1));
        rc = call.scan(r, query, dq, w.lo(h1), w.rows(h1));
        if (rc != GSIM_OK) return rc;
        uint32_t n = take();
        if (r == ScanRoute::kPlain) {
            if (st) st->queries_plain++;
            continue;
        }
        bool done = h1 == window;
        if (!done && n == call.k) {
            const float sk = out[n - 1].score;
            done = true;
            for (uint32_t b = window.b0; b <= window.b1 && done; b++)
                if ((b < h1.b0 || b > h1.b1) && !(ub[b] < sk)) done = false;
        }
        if (done) {
            if (st) st->queries_one_stage++;
            continue;
        }
        const Hull h2 = n == call.k ? hull_at_least(ub, window, out[n - 1].score) : window;
        r = call.route(w.rows(h2));
        rc = call.scan(r, query, dq, w.lo(h2), w.rows(h2));
        if (rc != GSIM_OK) return rc;
        n = take();
        if (st) (r == ScanRoute::kPlain ? st->queries_plain : st->queries_two_stage) += 1;
    }
    if (st) st->wall_ms = ms_since(t0);
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_popindex_create(gsim_db* db, uint32_t flags, gsim_popindex** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (flags & ~GSIM_POPINDEX_ROWS) return fail(GSIM_ERR_INVALID, "unknown popcount-index flags");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "popcount indexes: tables of 2^32 rows or more");
    if (const int rc = check_table_state(db, "popcount indexes", true)) return rc;
    return on_one_shard(db, "host memory for a popcount index", [&](Shard&) {
        std::unique_ptr<gsim_popindex> ix(new (std::nothrow) gsim_popindex);
        if (!ix) return fail(GSIM_ERR_NOMEM, "popcount index");
        const int rc = build_popindex(db, flags, ix.get());
        if (rc == GSIM_OK) *out = ix.release();
        return rc;
    });
}

int gsim_popindex_first(const gsim_popindex* ix, uint64_t* first)
{
    if (!ix || !first) return fail(GSIM_ERR_INVALID, "NULL argument");
    std::memcpy(first, ix->first.data(), ix->first.size() * 8);
    return GSIM_OK;
}

int gsim_popindex_order(const gsim_popindex* ix, uint32_t* order)
{
    if (!ix || (!order && ix->nrows)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (ix->nrows == 0) return GSIM_OK;
    GSIM_HIP(set_device(ix->device));
    GSIM_HIP(hipMemcpy(order, ix->d_order, static_cast<size_t>(ix->nrows) * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < ix->nrows; i++) order[i] += ix->row_base;
    return GSIM_OK;
}

int gsim_popindex_destroy(gsim_popindex* ix)
{
    if (!ix) return GSIM_OK;
    (void) set_device(ix->device);
    delete ix;
    return GSIM_OK;
}

int gsim_db_search_bounded(gsim_db* db, const gsim_popindex* ix, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, int metric,
                           float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx, gsim_popindex_stats* stats)
{
    if (stats) *stats = gsim_popindex_stats{};
    if (!db || !ix || !queries || !hits || !counts) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (ix->owner != db) return fail(GSIM_ERR_INVALID, "the popcount index was made for another handle");
    if (const int rc = check_table_state(db, "bounded searches", true)) return rc;
    if (ix->nrows != db->nrows) return fail(GSIM_ERR_STATE, "the table changed after the popcount index was made");
    return on_one_shard(db, "host memory for a bounded search", [&](Shard& s) {
        return search_bounded(db, s, ix, queries, nq, k, cutoff, metric, alpha, beta, hits, counts, approx, stats);
    });
}

} // extern "C"
