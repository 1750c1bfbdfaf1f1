// capi_subset.cpp -- row sets (gsim_rowset_*) and gsim_db_search_rows: exact top-k restricted to a subset of the table.  The
// row-set lifecycle, the argument checks and the route choice per call; the device side is gsim_subset.hip (the two scans, the
// kernels that build a set) and the four-kernel pipeline's own tail (capi_query.cpp enqueue_scan_tail).  The rule is stated in
// include/gpusim_hip.h.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

// what both constructors check after their own arguments, in this order
int check_rowset_state(const gsim_db* db)
{
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "row sets: tables of 2^32 rows or more");
    return check_table_state(db, "row sets", true);
}

// The set on the device: `rows` marked into a zeroed bitmap, or the caller's `bits`; inverted for an exclusion set; then the list.
int build_rowset(gsim_db* db, const uint32_t* rows, uint64_t n, const uint32_t* bits, bool exclude, gsim_rowset* rs)
{
    Shard& s = db->shards[0];
    const uint64_t N = s.nrows;
    const uint64_t nwords = gsim::rowset_words(N), nalloc = nwords + gsim::kRowsetPadWords;
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    rs->owner = db;
    rs->device = s.device;
    rs->nrows = N;
    rs->row_base = db->row_base;
    DevBuf<uint32_t>& d_bits = rs->d_bits; // (the set keeps these two; the others are freed on return)
    DevBuf<uint32_t>& d_list = rs->d_list;
    DevBuf<uint32_t> d_in, d_popc, d_offs;
    DevBuf<> d_tmp;
    GSIM_ALLOC(d_bits, nalloc * 4, "the row set's bitmap");
    GSIM_ALLOC(d_popc, (nwords + 1) * 4, "the row set's word counts");
    GSIM_ALLOC(d_offs, (nwords + 1) * 4, "the row set's word offsets");
    if (bits) {
        GSIM_ALLOC(d_in, nwords * 4, "the caller's bitmap");
        GSIM_HIP(hipMemcpyAsync(d_in, bits, nwords * 4, hipMemcpyHostToDevice, st));
    } else {
        GSIM_HIP(hipMemsetAsync(d_bits, 0, nalloc * 4, st));
        if (n) {
            GSIM_ALLOC(d_in, n * 4, "the caller's rows");
            GSIM_HIP(hipMemcpyAsync(d_in, rows, n * 4, hipMemcpyHostToDevice, st));
            GSIM_HIP(gsim::launch_rowset_mark(d_in, n, db->row_base, N, d_bits, st));
        }
    }
    GSIM_HIP(gsim::launch_rowset_finish(d_bits, bits ? d_in.as<uint32_t>() : nullptr, N, nalloc, exclude ? 1 : 0,
                                        d_popc, st));
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::scan_u32_bytes(nwords + 1, &tmp_bytes));
    GSIM_ALLOC(d_tmp, tmp_bytes, "the row set's prefix sums");
    GSIM_HIP(gsim::launch_scan_u32(d_tmp, tmp_bytes, d_popc, d_offs, nwords + 1, st));
    uint32_t count = 0;
    GSIM_HIP(hipMemcpyAsync(&count, d_offs + nwords, 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    // (a full 2^32 - 1-row table selected whole still fits: the sum is < 2^32)
    GSIM_ALLOC(d_list, static_cast<size_t>(count) * 4, "the row set's list");
    GSIM_HIP(gsim::launch_rowset_list(d_bits, d_offs, nwords, d_list, st));
    GSIM_HIP(hipStreamSynchronize(st)); // (the temporaries are freed on return)
    rs->count = count;
    return GSIM_OK;
}

int make_rowset(gsim_db* db, const uint32_t* rows, uint64_t n, const uint32_t* bits, uint32_t flags, gsim_rowset** out)
{
    std::lock_guard<std::mutex> guard(db->search_mutex);
    gsim_rowset* rs = new (std::nothrow) gsim_rowset;
    if (!rs) return fail(GSIM_ERR_NOMEM, "row set");
    const int rc = build_rowset(db, rows, n, bits, (flags & GSIM_ROWSET_EXCLUDE) != 0, rs);
    if (rc != GSIM_OK) {
        delete rs;
        return rc;
    }
    *out = rs;
    return GSIM_OK;
}

} // namespace

// The candidate scratch of the four-kernel pipeline (allocated on first use, as the classic route does), grown where a row-set
// geometry has more waves or slots than the shard's own (widths whose masked scan takes another loop than launch_scan's; a
// gather grid's rounding; a group query's grid) -- larger buffers are invisible to the classic kernels, which address them with
// their own geometry.
int ensure_subset_scratch(Shard& s, const gsim::ScanGeometry& g)
{
    const int rc = ensure_classic_scratch(s);
    if (rc != GSIM_OK) return rc;
    const uint64_t have = std::max<uint64_t>(static_cast<uint64_t>(s.geo.nwaves) * s.geo.seg_cap, s.cand_slots);
    const uint32_t have_waves = std::max(s.geo.nwaves, s.seg_waves);
    const uint64_t need = static_cast<uint64_t>(g.nwaves) * g.seg_cap;
    if (need <= have && g.nwaves <= have_waves) return GSIM_OK;
    GSIM_HIP(hipStreamSynchronize(s.stream)); // (nothing of this handle is in flight under the lock -- but a free must not overtake a kernel)
    if (need > have) { // (allocate, then swap: a failure leaves the classic route's scratch standing)
        if (s.d_cand.grow_keep(static_cast<size_t>(need) * 8) != hipSuccess || s.d_cand_cb.grow_keep(static_cast<size_t>(need) * 4) != hipSuccess)
            return fail(GSIM_ERR_NOMEM, "device memory for the candidate segments of a row-set search");
        s.cand_slots = need;
    }
    if (g.nwaves > have_waves) {
        if (s.d_seg_count.grow_keep(static_cast<size_t>(g.nwaves) * 4) != hipSuccess)
            return fail(GSIM_ERR_NOMEM, "device memory for the segment counts of a row-set search");
        s.seg_waves = g.nwaves;
    }
    return GSIM_OK;
}

// The two halves of run_restricted_scan (capi_internal.h) around the caller's scan.  In front: the scratch and the result block for
// geometry g and a.k hits, a's scratch pointers (the checks may have moved them), the first event.
int begin_restricted_scan(Shard& s, gsim::ScanArgs& a, const gsim::ScanGeometry& g, EventPair* ev)
{
    int rc = ensure_subset_scratch(s, g);
    if (rc == GSIM_OK) rc = ensure_result_capacity(s, a.k);
    if (rc != GSIM_OK) return rc;
    a.cand = s.d_cand, a.cand_cb = s.d_cand_cb, a.seg_count = s.d_seg_count;
    if (ev) GSIM_HIP(hipEventRecord(ev->a, s.stream));
    return GSIM_OK;
}

// Behind: the pipeline's tail into s.h_result, the second event, the wait; the kernel time and the tail's launches are added to *cost.
int finish_restricted_scan(gsim_db* db, Shard& s, const gsim::ScanArgs& a, const gsim::ScanGeometry& g, uint64_t all_rows, EventPair* ev,
                           ScanStepCost* cost)
{
    int rc = enqueue_scan_tail(db, s, a, g, db->row_base + static_cast<uint32_t>(s.first_row), all_rows, s.h_result);
    if (rc != GSIM_OK) return rc;
    if (ev) GSIM_HIP(hipEventRecord(ev->b, s.stream));
    rc = wait_stream(s.stream);
    if (rc != GSIM_OK) return rc;
    if (ev) cost->kernel_ms += ev->ms();
    cost->launches += 2 + (a.k > static_cast<uint32_t>(gsim::kSelectCap) ? 2 : 0); // compaction, select -- or the large-k select and the sort's two
    return GSIM_OK;
}

uint32_t take_scan_result(const Shard& s, uint32_t k, gsim_hit* hits, uint32_t* count, uint64_t* approx)
{
    const gsim_result_header* h = s.h_result.as<const gsim_result_header>();
    const uint32_t n = std::min(h->count, k);
    std::memcpy(hits, h + 1, sizeof(gsim_hit) * n);
    *count = n;
    if (approx) *approx = h->approx;
    return n;
}

// gather when selected x max(row bytes, 128) x 1000 <= permille x N x row bytes (gsim_db_bit_counts decides by the same rule)
bool subset_gather_applies(const gsim_db* db, const Shard& s, uint64_t selected)
{
    const uint64_t permille = static_cast<uint64_t>(db->knobs.subset_gather_max_permille);
    if (permille == 0) return false;
    if (permille >= 1000) return true;
    const uint64_t row_bytes = static_cast<uint64_t>(s.W) * 4u;
    return selected * std::max<uint64_t>(row_bytes, 128u) * 1000u <= permille * s.nrows * row_bytes; // (< 2^32 x 2^12 x 2^10: no overflow)
}

namespace
{

int search_rows(gsim_db* db, Shard& s, const gsim_rowset* rs, const uint32_t* queries, uint32_t nq, uint32_t kout, float cutoff, int metric,
                float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx, gsim_rowset_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t sel = rs->count;
    const uint32_t k = static_cast<uint32_t>(std::min<uint64_t>(kout, sel)); // (as gsim_db_search: never more hits than rows)
    if (st) st->selected = sel;
    if (sel == 0 || nq == 0) { // the empty set: zero hits, approx 0
        for (uint32_t q = 0; q < nq; q++) {
            counts[q] = 0;
            if (approx) approx[q] = 0;
        }
        if (st) st->wall_ms = ms_since(t0);
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;
    const bool gather = subset_gather_applies(db, s, sel);
    const gsim::ScanGeometry g = gather ? gsim::subset_gather_geometry(sel, s.W, s.num_cus) : gsim::subset_scan_geometry(s.nrows, s.W, s.num_cus);
    int rc = rezero_dirty_state(s);
    if (rc != GSIM_OK) return rc;
    DevBuf<uint32_t> d_q; // the call's queries (16-byte aligned rows when W % 4 == 0)
    GSIM_ALLOC(d_q, static_cast<size_t>(nq) * s.W * 4, "the queries of a row-set search");
    GSIM_HIP(hipMemcpyAsync(d_q, queries, static_cast<size_t>(nq) * s.W * 4, hipMemcpyHostToDevice, stream));
    EventPair ev;
    if (st) GSIM_HIP(ev.create());
    // No seed: sample_kernel's threshold counts rows of the whole table and may lie above the set's k-th best (DESIGN.md
    // section 12); both scans start from gtau = 0 and raise it through the histogram of SELECTED rows.
    const auto enqueue = [&](gsim::ScanArgs& a, uint32_t& launches) {
        if (gather) GSIM_HIP(gsim::launch_subset_gather(a, g, rs->d_list, static_cast<uint32_t>(sel), stream));
        else GSIM_HIP(gsim::launch_subset_scan(a, g, rs->d_bits, stream));
        a.nrows = sel; // (the tail's "all rows" -- approx without a cutoff -- is the set)
        launches += 1;
        return static_cast<int>(GSIM_OK);
    };
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t* query = queries + static_cast<size_t>(q) * s.W;
        uint32_t* dq = d_q + static_cast<size_t>(q) * s.W; // (the tail reads the same copy: nothing to write)
        ScanStepCost cost;
        rc = run_restricted_scan(db, s, scan_args(s, query, dq, dq, k, cutoff, metric, alpha, beta), g, sel, st ? &ev : nullptr, enqueue, &cost);
        if (rc != GSIM_OK) return rc;
        take_scan_result(s, k, hits + static_cast<size_t>(q) * kout, &counts[q], approx ? &approx[q] : nullptr);
        if (st) {
            st->kernel_ms += cost.kernel_ms;
            st->launches += cost.launches;
            (gather ? st->queries_gather : st->queries_stream) += 1;
        }
    }
    if (st) st->wall_ms = ms_since(t0);
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_rowset_from_rows(gsim_db* db, const uint32_t* rows, uint64_t n, uint32_t flags, gsim_rowset** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (n && !rows) return fail(GSIM_ERR_INVALID, "NULL rows");
    if (flags & ~GSIM_ROWSET_EXCLUDE) return fail(GSIM_ERR_INVALID, "unknown row-set flags");
    if (n > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "row sets: 2^32 rows or more given");
    for (uint64_t i = 0; i < n; i++)
        if (rows[i] < db->row_base || static_cast<uint64_t>(rows[i]) - db->row_base >= db->nrows)
            return fail(GSIM_ERR_INVALID, "row set: row " + std::to_string(rows[i]) + " outside the table");
    const int rc = check_rowset_state(db);
    if (rc != GSIM_OK) return rc;
    return make_rowset(db, rows, n, nullptr, flags, out);
}

int gsim_rowset_from_bitmap(gsim_db* db, const uint32_t* bits, uint32_t flags, gsim_rowset** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (!bits) return fail(GSIM_ERR_INVALID, "NULL bitmap");
    if (flags & ~GSIM_ROWSET_EXCLUDE) return fail(GSIM_ERR_INVALID, "unknown row-set flags");
    const int rc = check_rowset_state(db);
    if (rc != GSIM_OK) return rc;
    return make_rowset(db, nullptr, 0, bits, flags, out);
}

int gsim_rowset_count(const gsim_rowset* rs, uint64_t* n)
{
    if (!rs || !n) return fail(GSIM_ERR_INVALID, "NULL argument");
    *n = rs->count;
    return GSIM_OK;
}

int gsim_rowset_rows(const gsim_rowset* rs, uint32_t* rows)
{
    if (!rs || (!rows && rs->count)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (rs->count == 0) return GSIM_OK;
    GSIM_HIP(set_device(rs->device));
    GSIM_HIP(hipMemcpy(rows, rs->d_list, static_cast<size_t>(rs->count) * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < rs->count; i++) rows[i] += rs->row_base;
    return GSIM_OK;
}

int gsim_rowset_destroy(gsim_rowset* rs)
{
    if (!rs) return GSIM_OK;
    (void) set_device(rs->device);
    delete rs;
    return GSIM_OK;
}

int gsim_db_search_rows(gsim_db* db, const gsim_rowset* rs, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, int metric,
                        float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx, gsim_rowset_stats* stats)
{
    if (stats) *stats = gsim_rowset_stats{};
    if (!db || !rs || !queries || !hits || !counts) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (rs->owner != db) return fail(GSIM_ERR_INVALID, "the row set was made for another handle");
    if (const int rc = check_table_state(db, "row-set searches", true)) return rc;
    if (rs->nrows != db->nrows) return fail(GSIM_ERR_STATE, "the table changed after the row set was made");
    return on_one_shard(db, "host memory for a row-set search", [&](Shard& s) {
        return search_rows(db, s, rs, queries, nq, k, cutoff, metric, alpha, beta, hits, counts, approx, stats);
    });
}

} // extern "C"
