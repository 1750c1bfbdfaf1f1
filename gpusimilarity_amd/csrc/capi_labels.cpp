// capi_labels.cpp -- centroid clustering: gsim_db_assign (the nearest of m centres for every row of a range), gsim_db_label_counts
// (the column counts of every label in one pass), gsim_label_centroids (host: the majority votes) and gsim_db_kmeans (the loop over
// the three, labels resident on the device).  The argument checks, the slabs and launch cuts and the copies of a call; the device
// side is gsim_assign.hip and gsim_labels.hip.  The rules are stated in include/gpusim_hip.h; DESIGN.md section 21 has the routes.
// The label sort (LabelSort, declared in capi_front.h) is also the first step of gsim_db_label_sums (capi_label_sums.cpp).
#include "capi_front.h"

namespace gsim_host
{

int LabelSort::alloc(uint64_t n, uint32_t nlabels, const char* what)
{
    const std::string w = std::string("device memory for ") + what;
    GSIM_HIP(gsim::labels_sort_bytes(n, nlabels, &tmp_bytes));
    if (keys.grow(n * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (sort keys)");
    if (vals.grow(n * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (row numbers)");
    if (keys2.grow(n * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (sorted keys)");
    if (vals2.grow(n * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (sorted row numbers)");
    if (tmp.grow(tmp_bytes) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (the sort's scratch)");
    if (first.grow((static_cast<size_t>(nlabels) + 1) * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (segment starts)");
    h_first.assign(static_cast<size_t>(nlabels) + 1, 0);
    return GSIM_OK;
}

int LabelSort::enqueue(const uint32_t* h_labels, uint32_t* d_labels, uint64_t n, uint32_t nlabels, uint64_t r0, hipStream_t st)
{
    if (h_labels) GSIM_HIP(hipMemcpyAsync(d_labels, h_labels, n * 4, hipMemcpyHostToDevice, st));
    GSIM_HIP(gsim::launch_labels_keys(d_labels, n, nlabels, static_cast<uint32_t>(r0), keys, vals, st));
    GSIM_HIP(gsim::launch_labels_sort(tmp, tmp_bytes, keys, keys2, vals, vals2, n, nlabels, st));
    GSIM_HIP(gsim::launch_labels_bounds(keys2, n, nlabels, first, st));
    GSIM_HIP(hipMemcpyAsync(h_first.data(), first, h_first.size() * 4, hipMemcpyDeviceToHost, st));
    return GSIM_OK;
}

namespace
{

// Pairs of one launch of the assign kernel: the matrix kernel's price per pair (capi_scores.cpp) -- the same
// contraction and divide, a smaller store -- so the same budget: about 5 ms a launch at every width.
constexpr double kAssignLaunchBudget = 5.6e11;
constexpr double kAssignPairFloor = 120.0;
// Rows of one slab: its popcounts and, for rows that are not whole 256-bit groups, its zero-padded copy are the call's only
// per-row temporaries besides the outputs (at most 512 MB + 4 MB at 4064 bits)
constexpr uint64_t kAssignSlabRows = 1ull << 20;
static_assert(kAssignSlabRows % gsim::kScoresTile == 0, "slabs are whole row blocks");
// Bytes of table rows one launch of the counting kernel reads at most (GSIM_LABELS_LAUNCH_ROWS = 0): as capi_profile.cpp
constexpr uint64_t kLabelsLaunchBytes = (256ull << 20) * 128ull;

// table rows of one assign launch: whole row blocks within the pair budget, at least one
uint64_t assign_launch_rows(const gsim_db* db, uint32_t m, uint32_t WP)
{
    const long long knob = db->knobs.assign_launch_pairs;
    const double budget = knob > 0 ? static_cast<double>(knob) : kAssignLaunchBudget / (WP + kAssignPairFloor);
    const uint64_t blocks = static_cast<uint64_t>(budget / (static_cast<double>(m) * gsim::kScoresTile));
    return std::max<uint64_t>(blocks, 1) * gsim::kScoresTile;
}

struct AssignCall {
    uint64_t r0, nr; // the table rows [r0, r0 + nr), nr > 0
    int metric;
    float alpha, beta;
};

// d_centres[0 .. m) (W words each, on s's device) against the rows of c: d_label / d_score [0 .. c.nr).  Adds to ss; returns with
// the stream idle.
int assign_device(gsim_db* db, Shard& s, const uint32_t* d_centres, uint32_t m, const AssignCall& c, uint32_t* d_label, float* d_score,
                  gsim_assign_stats& ss)
{
    const hipStream_t st = s.stream;
    const uint32_t W = s.W, WP = gsim::scores_padded_words(W);
    const uint64_t slab = std::min(kAssignSlabRows, c.nr), per = assign_launch_rows(db, m, WP);
    PaddedRows centres, rows_of_slab;
    LaunchClocks clocks;
    if (const int rc = centres.alloc(m, W, WP, "the assignment (popcounts of the centres)", "the assignment (padded centres)")) return rc;
    if (const int rc = rows_of_slab.alloc(slab, W, WP, "the assignment (popcounts of a slab of rows)", "the assignment (a slab of padded rows)")) return rc;
    size_t nlaunch = 0;
    for (uint64_t f = 0; f < c.nr; f += slab) nlaunch += (std::min(slab, c.nr - f) + per - 1) / per;
    if (const int rc = clocks.own(nlaunch, "the assignment (clock stamps)")) return rc;
    GSIM_HIP(clocks.zero(nlaunch, st));
    EventPair ev_prep, ev_run;
    GSIM_HIP(ev_prep.create());
    GSIM_HIP(ev_run.create());

    gsim::AssignArgs a{};
    a.m = m;
    a.WP = WP;
    a.metric = c.metric;
    a.alpha = c.alpha;
    a.beta = c.beta;
    size_t launched = 0;
    for (uint64_t f = 0; f < c.nr; f += slab) {
        const uint64_t rows = std::min(slab, c.nr - f);
        const uint32_t* d_rows = static_cast<const uint32_t*>(s.d_rows) + (c.r0 + f) * W;
        GSIM_HIP(hipEventRecord(ev_prep.a, st));
        if (f == 0) { // the centres: once, with the first slab
            if (const int rc = centres.prepare(d_centres, m, st)) return rc;
            a.centres = centres.rows();
            a.cpop = centres.pop();
        }
        if (const int rc = rows_of_slab.prepare(d_rows, rows, st)) return rc;
        GSIM_HIP(hipEventRecord(ev_prep.b, st));
        a.rows = rows_of_slab.rows();
        a.rpop = rows_of_slab.pop();
        a.nr = rows;
        a.label = d_label + f;
        a.score = d_score + f;
        GSIM_HIP(hipEventRecord(ev_run.a, st));
        for (uint64_t r = 0; r < rows; r += per) {
            a.clk = clocks.at(launched++);
            GSIM_HIP(gsim::launch_assign(a, r, std::min(r + per, rows), st));
        }
        GSIM_HIP(hipEventRecord(ev_run.b, st));
        // (one slab at a time: the next one's prepare overwrites the slab's buffers only in stream order, but the events are reused)
        GSIM_HIP(hipStreamSynchronize(st));
        ss.prepare_ms += ev_prep.ms();
        ss.kernel_ms += ev_run.ms();
    }
    ss.launches += nlaunch;
    GSIM_HIP(clocks.fetch(nlaunch, st));
    GSIM_HIP(hipStreamSynchronize(st));
    clocks.add();
    ss.clock_mhz = clocks.mhz();
    return GSIM_OK;
}

// The labels of the n > 0 rows from table row r0 on -- h_labels (copied into d_labels first) or d_labels as it is -- into counts
// (host, nlabels x fp_bits; nullptr: the sizes alone, nothing is counted) and sizes (host, nlabels, or nullptr).  Adds to ls; returns
// with the stream idle.
int label_counts_device(gsim_db* db, Shard& s, const uint32_t* h_labels, uint32_t* d_labels, uint64_t n, uint32_t nlabels, uint64_t r0, uint32_t* counts,
                        uint32_t* sizes, gsim_label_stats& ls)
{
    const hipStream_t st = s.stream;
    const uint32_t F = db->fp_bits;
    const size_t ncount = static_cast<size_t>(nlabels) * F;
    LabelSort sort;
    DevBuf<uint32_t> d_counts;
    if (const int rc = sort.alloc(n, nlabels, "the label counts")) return rc;
    if (counts) GSIM_ALLOC(d_counts, ncount * 4, "the label counters");
    EventPair ev_sort, ev_run, ev_d2h;
    GSIM_HIP(ev_sort.create());
    GSIM_HIP(ev_run.create());
    GSIM_HIP(ev_d2h.create());

    GSIM_HIP(hipEventRecord(ev_sort.a, st));
    if (const int rc = sort.enqueue(h_labels, d_labels, n, nlabels, r0, st)) return rc;
    const std::vector<uint32_t>& h_first = sort.h_first;
    if (counts) GSIM_HIP(hipMemsetAsync(d_counts, 0, ncount * 4, st));
    GSIM_HIP(hipEventRecord(ev_sort.b, st));
    GSIM_HIP(hipStreamSynchronize(st));
    ls.sort_ms += ev_sort.ms();
    const uint64_t counted = h_first[nlabels]; // (GSIM_LABEL_NONE sorts behind every label)
    ls.rows_read += n;
    ls.rows_counted += counted;
    if (sizes)
        for (uint32_t l = 0; l < nlabels; l++) sizes[l] = h_first[l + 1] - h_first[l];
    if (!counts) return GSIM_OK;

    gsim::LabelCountArgs a{};
    a.rows = static_cast<const uint32_t*>(s.d_rows);
    a.W = s.W;
    a.keys = sort.keys2;
    a.list = sort.vals2;
    a.counts = d_counts;
    a.nlabels = nlabels;
    const uint64_t knob = static_cast<uint64_t>(db->knobs.labels_launch_rows);
    const uint64_t per = std::max<uint64_t>(knob > 0 ? knob : kLabelsLaunchBytes / (static_cast<uint64_t>(s.W) * 4u), 1);
    GSIM_HIP(hipEventRecord(ev_run.a, st));
    for (uint64_t i = 0; i < counted; i += per) {
        GSIM_HIP(gsim::launch_labels_count(a, i, std::min(i + per, counted), s.num_cus, st));
        ls.launches++;
    }
    GSIM_HIP(hipEventRecord(ev_run.b, st));
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    GSIM_HIP(hipMemcpyAsync(counts, d_counts, ncount * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st)); // (the temporaries are freed on return)
    ls.kernel_ms += ev_run.ms();
    ls.d2h_ms += ev_d2h.ms();
    return GSIM_OK;
}

// ---- what the entry points check before any device state ----
int check_range(const gsim_db* db, uint64_t row_begin, uint64_t row_end, const char* what)
{
    if (const int rc = check_row_range(db, row_begin, row_end)) return rc;
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, std::string(what) + ": tables of 2^32 rows or more");
    if (db->fp_bits > 4096) return fail(GSIM_ERR_INVALID, std::string(what) + " supports rows of up to 4096 bits");
    return GSIM_OK;
}

int check_assign_args(const gsim_db* db, uint32_t m, uint64_t row_begin, uint64_t row_end, int metric, float alpha, float beta)
{
    if (!db) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (m == 0 || m > GSIM_ASSIGN_MAX_CENTRES) return fail(GSIM_ERR_INVALID, "assign: the number of centres must be 1 ... GSIM_ASSIGN_MAX_CENTRES");
    if (const int rc = check_metric("assign", metric, alpha, beta)) return rc;
    return check_range(db, row_begin, row_end, "assign");
}

int assign(gsim_db* db, Shard& s, const uint32_t* centres, uint32_t m, const AssignCall& c, uint32_t* label, float* score, gsim_assign_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    gsim_assign_stats ss{};
    ss.rows = c.nr;
    ss.centres = m;
    ss.pairs = static_cast<uint64_t>(m) * c.nr;
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    DevBuf<uint32_t> d_centres, d_label;
    DevBuf<float> d_score;
    const size_t cbytes = static_cast<size_t>(m) * s.W * 4;
    GSIM_ALLOC(d_centres, cbytes, "the assignment's centres");
    GSIM_ALLOC(d_label, c.nr * 4, "the assignment's labels");
    GSIM_ALLOC(d_score, c.nr * 4, "the assignment's scores");
    GSIM_HIP(hipMemcpyAsync(d_centres, centres, cbytes, hipMemcpyHostToDevice, st));
    const int rc = assign_device(db, s, d_centres, m, c, d_label, d_score, ss);
    if (rc != GSIM_OK) {
        (void) hipStreamSynchronize(st); // (nothing of the call is still running when its buffers go)
        return rc;
    }
    EventPair ev_d2h;
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    GSIM_HIP(hipMemcpyAsync(label, d_label, c.nr * 4, hipMemcpyDeviceToHost, st));
    if (score) GSIM_HIP(hipMemcpyAsync(score, d_score, c.nr * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st));
    ss.d2h_ms = ev_d2h.ms();
    ss.wall_ms = ms_since(t0);
    if (stats) *stats = ss;
    return GSIM_OK;
}

int label_counts(gsim_db* db, Shard& s, const uint32_t* labels, uint32_t nlabels, uint64_t rb, uint64_t re, uint32_t* counts, uint32_t* sizes,
                 gsim_label_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    gsim_label_stats ls{};
    ls.labels = nlabels;
    GSIM_HIP(set_device(s.device));
    DevBuf<uint32_t> d_labels;
    GSIM_ALLOC(d_labels, (re - rb) * 4, "the label counts (labels)");
    const int rc = label_counts_device(db, s, labels, d_labels, re - rb, nlabels, rb, counts, sizes, ls);
    if (rc != GSIM_OK) {
        (void) hipStreamSynchronize(s.stream);
        return rc;
    }
    ls.wall_ms = ms_since(t0);
    if (stats) *stats = ls;
    return GSIM_OK;
}

int kmeans(gsim_db* db, Shard& s, const uint32_t* init, uint32_t m, uint32_t max_iter, int metric, float alpha, float beta, uint32_t* centres,
           uint32_t* label, float* score, uint32_t* sizes, gsim_kmeans_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = db->nrows;
    const uint32_t W = s.W, F = db->fp_bits;
    const size_t cwords = static_cast<size_t>(m) * W;
    gsim_kmeans_stats ks{};
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    DevBuf<uint32_t> d_centres, d_lab[2];
    DevBuf<float> d_score;
    DevBuf<unsigned long long> d_changed;
    GSIM_ALLOC(d_centres, cwords * 4, "k-means (centres)");
    GSIM_ALLOC(d_lab[0], N * 4, "k-means (labels)");
    GSIM_ALLOC(d_lab[1], N * 4, "k-means (the previous labels)");
    GSIM_ALLOC(d_score, N * 4, "k-means (scores)");
    GSIM_ALLOC(d_changed, 8, "k-means (the changed-label count)");
    std::vector<uint32_t> cur(init, init + cwords), next(cwords), counts(static_cast<size_t>(m) * F), sz(m);
    const AssignCall call{0, N, metric, alpha, beta};
    bool sizes_valid = false; // sz holds the sizes of the labels last assigned
    uint32_t t = 0;
    auto drain = [&](int rc) {
        (void) hipStreamSynchronize(st);
        return rc;
    };
    for (;; t++) {
        auto tu = std::chrono::steady_clock::now();
        GSIM_HIP(hipMemcpyAsync(d_centres, cur.data(), cwords * 4, hipMemcpyHostToDevice, st));
        GSIM_HIP(hipStreamSynchronize(st));
        ks.update_ms += ms_since(tu);
        gsim_assign_stats as{};
        int rc = assign_device(db, s, d_centres, m, call, d_lab[t & 1], d_score, as);
        if (rc != GSIM_OK) return drain(rc);
        ks.assign_ms += as.prepare_ms + as.kernel_ms;
        ks.iterations = t + 1;
        ks.changed_last = N;
        if (t > 0) {
            unsigned long long changed = 0;
            GSIM_HIP(hipMemsetAsync(d_changed, 0, 8, st));
            GSIM_HIP(gsim::launch_labels_changed(d_lab[0], d_lab[1], N, d_changed, st));
            GSIM_HIP(hipMemcpyAsync(&changed, d_changed, 8, hipMemcpyDeviceToHost, st));
            GSIM_HIP(hipStreamSynchronize(st));
            ks.changed_last = changed;
            ks.converged = changed == 0 ? 1 : 0; // (equal labels: sz, counted from the previous ones, holds these labels' sizes too)
        }
        if (ks.converged || t + 1 == max_iter) break;
        gsim_label_stats ls{};
        rc = label_counts_device(db, s, nullptr, d_lab[t & 1], N, m, 0, counts.data(), sz.data(), ls);
        if (rc != GSIM_OK) return drain(rc);
        ks.counts_ms += ls.sort_ms + ls.kernel_ms + ls.d2h_ms;
        tu = std::chrono::steady_clock::now();
        rc = gsim_label_centroids(counts.data(), sz.data(), m, F, cur.data(), next.data());
        if (rc != GSIM_OK) return rc;
        cur.swap(next);
        ks.update_ms += ms_since(tu);
        sizes_valid = true;
    }
    if (sizes && !(ks.converged && sizes_valid)) { // the last labels were never counted
        gsim_label_stats ls{};
        const int rc = label_counts_device(db, s, nullptr, d_lab[t & 1], N, m, 0, nullptr, sz.data(), ls);
        if (rc != GSIM_OK) return drain(rc);
        ks.counts_ms += ls.sort_ms;
    }
    GSIM_HIP(hipMemcpyAsync(label, d_lab[t & 1], N * 4, hipMemcpyDeviceToHost, st));
    if (score) GSIM_HIP(hipMemcpyAsync(score, d_score, N * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    std::copy(cur.begin(), cur.end(), centres);
    if (sizes) std::copy(sz.begin(), sz.end(), sizes);
    ks.wall_ms = ms_since(t0);
    if (stats) *stats = ks;
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_assign(gsim_db* db, const uint32_t* centres, uint32_t m, uint64_t row_begin, uint64_t row_end, int metric, float alpha, float beta,
                   uint32_t* label, float* score, gsim_assign_stats* stats)
{
    int rc = check_assign_args(db, m, row_begin, row_end, metric, alpha, beta);
    if (rc != GSIM_OK) return rc;
    if (row_begin < row_end && (!centres || !label)) return fail(GSIM_ERR_INVALID, "assign: NULL centres or label");
    rc = check_table_state(db, "assign", false);
    if (rc != GSIM_OK) return rc;
    if (stats) {
        *stats = gsim_assign_stats{};
        stats->centres = m;
    }
    if (row_begin == row_end) return GSIM_OK;
    return on_one_shard(db, "host memory for the assignment", [&](Shard& s) {
        return assign(db, s, centres, m, AssignCall{row_begin, row_end - row_begin, metric, alpha, beta}, label, score, stats);
    });
}

int gsim_db_label_counts(gsim_db* db, const uint32_t* labels, uint32_t nlabels, uint64_t row_begin, uint64_t row_end, uint32_t* counts, uint32_t* sizes,
                         gsim_label_stats* stats)
{
    if (!db || !counts) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nlabels == 0) return fail(GSIM_ERR_INVALID, "label counts: nlabels == 0");
    int rc = check_range(db, row_begin, row_end, "label counts");
    if (rc != GSIM_OK) return rc;
    const uint64_t n = row_end - row_begin;
    if (n && !labels) return fail(GSIM_ERR_INVALID, "label counts: NULL labels");
    for (uint64_t i = 0; i < n; i++)
        if (labels[i] >= nlabels && labels[i] != GSIM_LABEL_NONE)
            return fail(GSIM_ERR_INVALID, "label counts: the label of row " + std::to_string(row_begin + i) + " is not below nlabels");
    if (db->nrows != 0) { // (an empty table has nothing to read: zeros)
        rc = check_table_state(db, "label counts", false);
        if (rc != GSIM_OK) return rc;
    }
    if (stats) {
        *stats = gsim_label_stats{};
        stats->labels = nlabels;
    }
    if (n == 0) {
        std::fill(counts, counts + static_cast<size_t>(nlabels) * db->fp_bits, 0u);
        if (sizes) std::fill(sizes, sizes + nlabels, 0u);
        return GSIM_OK;
    }
    return on_one_shard(db, "host memory for the label counts",
                        [&](Shard& s) { return label_counts(db, s, labels, nlabels, row_begin, row_end, counts, sizes, stats); });
}

int gsim_label_centroids(const uint32_t* counts, const uint32_t* sizes, uint32_t nlabels, uint32_t fp_bits, const uint32_t* previous, uint32_t* centres)
{
    if (!counts || !sizes || !centres) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nlabels == 0) return fail(GSIM_ERR_INVALID, "label centroids: nlabels == 0");
    if (fp_bits == 0 || fp_bits % 32) return fail(GSIM_ERR_INVALID, "label centroids: fp_bits must be a positive multiple of 32");
    const uint32_t W = fp_bits / 32;
    for (uint32_t l = 0; l < nlabels; l++) // (nothing is written when anything is refused)
        for (uint32_t k = 0; k < fp_bits; k++)
            if (counts[static_cast<size_t>(l) * fp_bits + k] > sizes[l])
                return fail(GSIM_ERR_INVALID, "label centroids: a count of label " + std::to_string(l) + " is above its size");
    for (uint32_t l = 0; l < nlabels; l++) {
        uint32_t* out = centres + static_cast<size_t>(l) * W;
        const uint32_t* c = counts + static_cast<size_t>(l) * fp_bits;
        if (sizes[l] == 0) {
            for (uint32_t w = 0; w < W; w++) out[w] = previous ? previous[static_cast<size_t>(l) * W + w] : 0u;
            continue;
        }
        for (uint32_t w = 0; w < W; w++) {
            uint32_t word = 0;
            for (uint32_t b = 0; b < 32; b++)
                if (2ull * c[w * 32 + b] >= sizes[l]) word |= 1u << b;
            out[w] = word;
        }
    }
    return GSIM_OK;
}

int gsim_db_kmeans(gsim_db* db, const uint32_t* init, uint32_t m, uint32_t max_iter, int metric, float alpha, float beta, uint32_t* centres,
                   uint32_t* label, float* score, uint32_t* sizes, gsim_kmeans_stats* stats)
{
    int rc = check_assign_args(db, m, 0, db ? db->nrows : 0, metric, alpha, beta);
    if (rc != GSIM_OK) return rc;
    if (max_iter == 0) return fail(GSIM_ERR_INVALID, "k-means: max_iter == 0");
    if (!init || !centres || (db->nrows && !label)) return fail(GSIM_ERR_INVALID, "k-means: NULL init, centres or label");
    rc = check_table_state(db, "k-means", false);
    if (rc != GSIM_OK) return rc;
    if (db->nrows == 0) return fail(GSIM_ERR_STATE, "k-means: the table has no rows");
    return on_one_shard(db, "host memory for k-means", [&](Shard& s) {
        return kmeans(db, s, init, m, max_iter, metric, alpha, beta, centres, label, score, sizes, stats);
    });
}

} // extern "C"
