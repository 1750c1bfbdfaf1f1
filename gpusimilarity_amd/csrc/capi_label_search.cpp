// capi_label_search.cpp -- label sets (gsim_labelset_*) and gsim_db_search_labels: the best hit and the hit count of every label, per
// query, in one pass over the table.  The label-set lifecycle, the argument checks, the plan (tile, route, launch cut) and the
// launch sequence of a call; the device side is gsim_label_search.hip.  The rule is stated in include/gpusim_hip.h; DESIGN.md
// section 30 has the routes and the measurements.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

// Queries of a tile: the call's device memory is bounded by one tile (tile x nlabels x 24 bytes + the rank's scratch), and the
// queries of a tile share table passes.  Sixteen inner products per row keep the scan near the rate the rows arrive at on 1024-bit
// rows (the multi-query scan's figure); kLabelTileCells bounds tile x nlabels where nlabels is large.
constexpr uint32_t kLabelTile = 16;
constexpr uint64_t kLabelTileCells = 1ull << 27;
// launch_rows = 0: a launch is bounded by its work, with gsim_db_search_group's price of a row x query pair (capi_group.cpp,
// DESIGN.md section 13): kLabelLaunchWork / (W + 14) pairs, a twentieth of that for the word loop
constexpr uint64_t kLabelLaunchWork = 45000000000ull;
constexpr uint64_t kLabelPairOverhead = 14;
constexpr uint64_t kLabelWordLoopCost = 20;

// How a call runs: `tile` queries at a time hold device memory, `pass` of them share a table pass; route LDS (the pass's table in
// every workgroup's LDS) while ONE query's table fits kLabelLdsBudget -- then as many queries per pass as fit --, else route
// global with the whole tile in one pass.
struct LabelPlan {
    uint32_t tile = 1, pass = 1;
    uint32_t cell_bytes = 8; // per (query, label): the key, + 4 when the kept rows are counted
    bool lds = false;
};
LabelPlan plan_label_search(uint32_t nq, uint32_t nlabels, bool counting)
{
    LabelPlan p;
    p.cell_bytes = counting ? 12u : 8u;
    p.tile = static_cast<uint32_t>(std::min<uint64_t>({nq, kLabelTile, std::max<uint64_t>(kLabelTileCells / nlabels, 1u)}));
    const uint64_t per_query = static_cast<uint64_t>(nlabels) * p.cell_bytes;
    p.lds = per_query <= gsim::kLabelLdsBudget;
    p.pass = p.lds ? static_cast<uint32_t>(std::min<uint64_t>(p.tile, gsim::kLabelLdsBudget / per_query)) : p.tile;
    return p;
}

struct LabelCall {
    const gsim_labelset* ls;
    const uint32_t* queries;
    uint32_t nq, k;
    float cutoff;
    int metric;
    float alpha, beta;
    uint64_t launch_rows;
    gsim_hit* hits;
    uint32_t* hit_labels;
    uint32_t* counts;
    uint64_t* approx;
    uint64_t* rows_kept;
    gsim_hit* label_best;
    uint32_t* label_kept;
};

int search_labels(gsim_db* db, Shard& s, const LabelCall& c, gsim_label_search_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    const gsim_labelset* ls = c.ls;
    const uint32_t nlabels = ls->nlabels;
    gsim_label_search_stats ss{};
    ss.queries = c.nq;
    ss.labels = nlabels;
    for (uint32_t q = 0; q < c.nq; q++) {
        c.counts[q] = 0;
        if (c.approx) c.approx[q] = 0;
        if (c.rows_kept) c.rows_kept[q] = 0;
    }
    if (c.nq == 0 || s.nrows == 0) {
        const gsim_hit none{0xFFFFFFFFu, 0.0f, 0, 0};
        if (c.label_best) std::fill(c.label_best, c.label_best + static_cast<size_t>(c.nq) * nlabels, none);
        if (c.label_kept) std::fill(c.label_kept, c.label_kept + static_cast<size_t>(c.nq) * nlabels, 0u);
        ss.wall_ms = ms_since(t0);
        if (stats) *stats = ss;
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const bool has_cutoff = c.cutoff > 0.0f;
    const bool counting = has_cutoff && (c.rows_kept || c.label_kept); // (without a cutoff the kept rows are the label's rows)
    const LabelPlan plan = plan_label_search(c.nq, nlabels, counting);
    const uint32_t kk = std::min(c.k, nlabels); // (never more hits than labels)
    const uint32_t row_base = db->row_base + static_cast<uint32_t>(s.first_row);

    const size_t cells = static_cast<size_t>(plan.tile) * nlabels;
    DevBuf<uint32_t> d_q;
    DevBuf<unsigned long long> d_best, d_totals, d_sorted;
    DevBuf<uint32_t> d_kept, d_hit_labels;
    DevBuf<gsim_hit> d_label_best, d_hits;
    DevBuf<> d_tmp;
    size_t tmp_bytes = 0;
    GSIM_ALLOC(d_q, static_cast<size_t>(plan.tile) * (s.W + 1u) * 4, "the queries of a label search");
    GSIM_ALLOC(d_best, cells * 8, "the label table of a label search");
    if (counting) GSIM_ALLOC(d_kept, cells * 4, "the label counts of a label search");
    GSIM_ALLOC(d_label_best, cells * sizeof(gsim_hit), "the label hits of a label search");
    GSIM_ALLOC(d_totals, static_cast<size_t>(plan.tile) * 16, "the totals of a label search");
    if (kk) {
        GSIM_HIP(gsim::label_rank_bytes(nlabels, &tmp_bytes));
        GSIM_ALLOC(d_sorted, static_cast<size_t>(nlabels) * 8, "the ranked labels of a label search");
        GSIM_ALLOC(d_tmp, tmp_bytes, "the rank's scratch of a label search");
        GSIM_ALLOC(d_hits, static_cast<size_t>(plan.tile) * kk * sizeof(gsim_hit), "the hits of a label search");
        GSIM_ALLOC(d_hit_labels, static_cast<size_t>(plan.tile) * kk * 4, "the hit labels of a label search");
    }
    Event ev[4];
    for (Event& e : ev) GSIM_HIP(e.create());
    std::vector<uint32_t> h_q;
    std::vector<unsigned long long> h_totals(static_cast<size_t>(plan.tile) * 2);
    // a failure between the launches: nothing of this call may still run when its buffers go
    auto drain = [&](int rc) {
        (void) hipStreamSynchronize(st);
        return rc;
    };

    gsim::LabelSearchArgs a{};
    a.rows = s.d_rows;
    a.nrows = s.nrows;
    a.W = s.W;
    a.labels = ls->d_labels;
    a.nlabels = nlabels;
    a.cutoff = c.cutoff;
    a.metric = c.metric;
    a.alpha = c.alpha;
    a.beta = c.beta;
    const uint32_t chunk_rows = gsim::label_chunk_rows(s.W);
    const uint64_t nchunks = (s.nrows + chunk_rows - 1) / chunk_rows;
    const bool word_loop = !(s.W == 4 || s.W == 8 || s.W == 16 || s.W == 32 || s.W == 64); // (launch_label_scan's switch)

    for (uint32_t q0 = 0; q0 < c.nq; q0 += plan.tile) {
        const uint32_t T = std::min(plan.tile, c.nq - q0);
        const size_t qwords = static_cast<size_t>(T) * s.W;
        h_q.assign(c.queries + static_cast<size_t>(q0) * s.W, c.queries + static_cast<size_t>(q0) * s.W + qwords);
        for (uint32_t q = 0; q < T; q++) h_q.push_back(popcount_words(h_q.data() + static_cast<size_t>(q) * s.W, s.W));
        GSIM_HIP(hipMemcpyAsync(d_q, h_q.data(), h_q.size() * 4, hipMemcpyHostToDevice, st));
        GSIM_HIP(hipMemsetAsync(d_best, 0, static_cast<size_t>(T) * nlabels * 8, st));
        if (counting) GSIM_HIP(hipMemsetAsync(d_kept, 0, static_cast<size_t>(T) * nlabels * 4, st));
        GSIM_HIP(hipMemsetAsync(d_totals, 0, static_cast<size_t>(T) * 16, st));
        GSIM_HIP(hipEventRecord(ev[0], st));
        for (uint32_t p0 = 0; p0 < T; p0 += plan.pass) {
            const uint32_t P = std::min(plan.pass, T - p0);
            a.queries = d_q + static_cast<size_t>(p0) * s.W;
            a.qpop = d_q + qwords + p0;
            a.nq = P;
            a.best = d_best + static_cast<size_t>(p0) * nlabels;
            a.kept = counting ? d_kept + static_cast<size_t>(p0) * nlabels : nullptr;
            a.lds_bytes = plan.lds ? P * nlabels * plan.cell_bytes : 0u;
            a.block = gsim::label_block_threads(a.lds_bytes);
            const uint32_t wpb = a.block / 64u;
            const uint64_t nw = std::min<uint64_t>(static_cast<uint64_t>(s.num_cus) * gsim::kLabelScanWavesPerCu, nchunks);
            a.nwaves = static_cast<uint32_t>((nw + wpb - 1) / wpb * wpb);
            const uint64_t rows_per_launch =
                c.launch_rows ? c.launch_rows : kLabelLaunchWork / (s.W + kLabelPairOverhead) / (word_loop ? kLabelWordLoopCost : 1u) / P;
            const uint64_t chunks_per_launch = std::max<uint64_t>(rows_per_launch / chunk_rows, 1u);
            for (uint64_t c0 = 0; c0 < nchunks; c0 += chunks_per_launch) {
                a.c0 = c0;
                a.c1 = std::min(c0 + chunks_per_launch, nchunks);
                const hipError_t e = gsim::launch_label_scan(a, st);
                if (e != hipSuccess) return drain(fail_hip(e, "launch_label_scan"));
                ss.launches++;
            }
            ss.passes++;
            (plan.lds ? ss.passes_lds : ss.passes_global)++;
        }
        GSIM_HIP(hipEventRecord(ev[1], st));
        a.queries = d_q;
        a.qpop = d_q + qwords;
        a.nq = T;
        a.best = d_best;
        a.kept = counting ? d_kept.as<uint32_t>() : nullptr;
        hipError_t e = gsim::launch_label_finish(a, row_base, d_label_best, d_totals, st);
        ss.launches++;
        for (uint32_t q = 0; q < T && kk && e == hipSuccess; q++) {
            e = gsim::launch_label_rank(d_tmp, tmp_bytes, d_best + static_cast<size_t>(q) * nlabels, d_sorted, nlabels, st);
            if (e == hipSuccess)
                e = gsim::launch_label_emit(d_sorted, ls->d_labels, d_label_best + static_cast<size_t>(q) * nlabels, kk, d_hits + static_cast<size_t>(q) * kk,
                                            d_hit_labels + static_cast<size_t>(q) * kk, st);
            ss.launches += 2; // (the sort counts as one)
        }
        if (e != hipSuccess) return drain(fail_hip(e, "the finish of a label search"));
        GSIM_HIP(hipEventRecord(ev[2], st));
        e = hipMemcpyAsync(h_totals.data(), d_totals, static_cast<size_t>(T) * 16, hipMemcpyDeviceToHost, st);
        for (uint32_t q = 0; q < T && kk && e == hipSuccess; q++) {
            e = hipMemcpyAsync(c.hits + static_cast<size_t>(q0 + q) * c.k, d_hits + static_cast<size_t>(q) * kk, static_cast<size_t>(kk) * sizeof(gsim_hit),
                               hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(c.hit_labels + static_cast<size_t>(q0 + q) * c.k, d_hit_labels + static_cast<size_t>(q) * kk, static_cast<size_t>(kk) * 4,
                                   hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess && c.label_best)
            e = hipMemcpyAsync(c.label_best + static_cast<size_t>(q0) * nlabels, d_label_best, static_cast<size_t>(T) * nlabels * sizeof(gsim_hit),
                               hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && c.label_kept && counting)
            e = hipMemcpyAsync(c.label_kept + static_cast<size_t>(q0) * nlabels, d_kept, static_cast<size_t>(T) * nlabels * 4, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return drain(fail_hip(e, "the copies of a label search"));
        GSIM_HIP(hipEventRecord(ev[3], st));
        const int rc = wait_stream(st);
        if (rc != GSIM_OK) return rc;
        for (uint32_t q = 0; q < T; q++) {
            const uint64_t found = h_totals[2 * q];
            c.counts[q0 + q] = static_cast<uint32_t>(std::min<uint64_t>(found, c.k));
            if (c.approx) c.approx[q0 + q] = found;
            if (c.rows_kept) c.rows_kept[q0 + q] = has_cutoff ? h_totals[2 * q + 1] : ls->labelled;
            if (c.label_kept && !has_cutoff) std::copy(ls->sizes.begin(), ls->sizes.end(), c.label_kept + static_cast<size_t>(q0 + q) * nlabels);
        }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) ss.scan_ms += ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) ss.finish_ms += ms;
        if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) ss.d2h_ms += ms;
    }
    ss.wall_ms = ms_since(t0);
    if (stats) *stats = ss;
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_labelset_create(gsim_db* db, const uint32_t* labels, uint32_t nlabels, gsim_labelset** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nlabels == 0) return fail(GSIM_ERR_INVALID, "label set: nlabels == 0");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "label sets: tables of 2^32 rows or more");
    const uint64_t n = db->nrows;
    if (n && !labels) return fail(GSIM_ERR_INVALID, "label set: NULL labels");
    for (uint64_t i = 0; i < n; i++)
        if (labels[i] >= nlabels && labels[i] != GSIM_LABEL_NONE)
            return fail(GSIM_ERR_INVALID, "label set: the label of row " + std::to_string(i) + " is not below nlabels");
    if (const int rc = check_table_state(db, "label sets", true)) return rc;
    std::unique_ptr<gsim_labelset> ls(new (std::nothrow) gsim_labelset);
    if (!ls) return fail(GSIM_ERR_NOMEM, "label set");
    const int rc = on_one_shard(db, "host memory for a label set", [&](Shard& s) {
        ls->owner = db;
        ls->device = s.device;
        ls->nrows = n;
        ls->nlabels = nlabels;
        ls->sizes.assign(nlabels, 0u);
        for (uint64_t i = 0; i < n; i++)
            if (labels[i] != GSIM_LABEL_NONE) ls->sizes[labels[i]]++;
        for (uint32_t l = 0; l < nlabels; l++) {
            ls->labelled += ls->sizes[l];
            ls->nonempty += ls->sizes[l] ? 1u : 0u;
        }
        GSIM_HIP(set_device(s.device));
        GSIM_ALLOC(ls->d_labels, n * 4, "the label set");
        if (n) {
            GSIM_HIP(hipMemcpyAsync(ls->d_labels, labels, n * 4, hipMemcpyHostToDevice, s.stream));
            GSIM_HIP(hipStreamSynchronize(s.stream));
        }
        return GSIM_OK;
    });
    if (rc != GSIM_OK) return rc;
    *out = ls.release();
    return GSIM_OK;
}

int gsim_labelset_sizes(const gsim_labelset* ls, uint32_t* sizes, uint64_t* labelled, uint64_t* nonempty)
{
    if (!ls || !sizes) return fail(GSIM_ERR_INVALID, "NULL argument");
    std::copy(ls->sizes.begin(), ls->sizes.end(), sizes);
    if (labelled) *labelled = ls->labelled;
    if (nonempty) *nonempty = ls->nonempty;
    return GSIM_OK;
}

int gsim_labelset_destroy(gsim_labelset* ls)
{
    if (!ls) return GSIM_OK;
    (void) set_device(ls->device);
    delete ls;
    return GSIM_OK;
}

int gsim_db_search_labels(gsim_db* db, const gsim_labelset* ls, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, int metric, float alpha,
                          float beta, uint64_t launch_rows, gsim_hit* hits, uint32_t* hit_labels, uint32_t* counts, uint64_t* approx, uint64_t* rows_kept,
                          gsim_hit* label_best, uint32_t* label_kept, gsim_label_search_stats* stats)
{
    if (!db || !ls || !hits || !hit_labels || !counts) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nq && !queries) return fail(GSIM_ERR_INVALID, "label search: NULL queries");
    if (ls->owner != db) return fail(GSIM_ERR_INVALID, "the label set was made for another handle");
    if (const int rc = check_metric("label search", metric, alpha, beta)) return rc;
    if (db->fp_bits > 4096) return fail(GSIM_ERR_INVALID, "label search: rows wider than 4096 bits");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "label search: tables of 2^32 rows or more");
    if (const int rc = check_table_state(db, "label searches", true)) return rc;
    if (ls->nrows != db->nrows) return fail(GSIM_ERR_STATE, "the table changed after the label set was made");
    if (stats) *stats = gsim_label_search_stats{};
    const LabelCall call{ls, queries, nq, k, cutoff, metric, alpha, beta, launch_rows, hits, hit_labels, counts, approx, rows_kept, label_best, label_kept};
    return on_one_shard(db, "host memory for a label search", [&](Shard& s) { return search_labels(db, s, call, stats); });
}

} // extern "C"
