// capi_front.h -- what a call does before and after its launches, where several entry points had each carried a copy: the metric
// check, the state check and the left side of the two-table families (threshold joins, k-NN joins, histograms, score matrices), the
// wrapper of the graph-returning calls, the checks and the runner of the calls on one table, and the labelling tail of the forest
// calls.  Each family keeps the argument checks that are its own.  Implemented in capi_front.cpp (the score core: capi_scores.cpp;
// the label sort: capi_labels.cpp); DESIGN.md sections 24, 25 and 33.  Internal.
#pragma once

#include "capi_pairs.h"

namespace gsim_host
{

// INVALID "unknown metric", then "<prefix>: Tversky alpha and beta must be finite and >= 0"
int check_metric(const char* prefix, int metric, float alpha, float beta);

// The STATE errors of a two-table family (`plural`: "joins", "knn joins", "histograms", "score matrices") about one side (`which`:
// "table", "left table"), in one order: not finalized, folded, more than one shard.
int check_pair_state(const gsim_db* db, const char* plural, const char* which);

// The INVALID errors of a left handle, in this order: NULL, a range past its rows, fp_bits other than the table's.
int check_left_handle(const gsim_db* db, const gsim_db* left, uint64_t lrow_end);

// The left rows of a two-table call: a front fills it, the family's core reads it.  It owns the uploaded copy and the lock or
// locks (one call at a time on either handle), so it lives as long as the call.
struct LeftSide {
    const uint32_t* rows = nullptr; // nl rows of the table's W words, on the table's device
    uint64_t nl = 0;
    bool in_table = false;          // they are the table's own rows row0 ...: a core that pads the table need not pad them again
    uint64_t row0 = 0;

    // The rows [lrow_begin, lrow_end) of `left`, which check_left_handle has passed.  STATE: the table's state, the left
    // table's where it is another handle, "different devices"; then the locks.
    int from_handle(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, const char* plural);
    // nq host rows, copied on the shard's stream into device memory of the name `what` ("the join's left rows"; not at all with
    // `upload` false, for a core that will not read them).  INVALID "NULL queries" when nq > 0, the table's state, the lock.
    int from_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, const char* plural, const char* what, bool upload = true);

private:
    std::unique_lock<std::mutex> lock_db, lock_left;
    DevBuf<> d_left; // (freed before the locks go)
};

// A graph-returning call: fn(g) fills a new graph, which becomes *out when it returns GSIM_OK.  NOMEM `nomem_what` when it
// runs out of host memory.
template <class Fn> int make_graph(gsim_graph** out, const char* nomem_what, Fn&& fn)
{
    std::unique_ptr<gsim_graph> g(new (std::nothrow) gsim_graph);
    if (!g) return fail(GSIM_ERR_NOMEM, "graph");
    int rc;
    try {
        rc = fn(g.get());
    } catch (const std::bad_alloc&) {
        rc = fail(GSIM_ERR_NOMEM, nomem_what);
    }
    if (rc == GSIM_OK) *out = g.release();
    return rc;
}

// ---- the calls on one table ----

// The STATE errors of a single-table call, in one order: not finalized, "<subject> does not|do not support folded tables",
// "<subject> needs|need a single-shard handle".
int check_table_state(const gsim_db* db, const char* subject, bool plural);

// INVALID "unknown metric", then "<needs> a symmetric metric (Tversky with alpha == beta)" (`needs`: "maxmin needs", "components
// need"), then "<prefix>: Tversky alpha = beta must be finite and >= 0" -- not with prefix == nullptr: gsim_db_neighbors has never
// had that line.
int check_symmetric_metric(const char* needs, const char* prefix, int metric, float alpha, float beta);

// INVALID "row range: begin past end", then "row range outside the table"
int check_row_range(const gsim_db* db, uint64_t row_begin, uint64_t row_end);

// INVALID "NULL seeds", then per seed "seed row outside the table" and "repeated seed row"; NOMEM `nomem_what`
int check_seeds(const gsim_db* db, const uint32_t* seeds, uint32_t nseeds, const char* nomem_what);

// INVALID "<name>: rows wider than 4096 bits" (wider than the tile kernels hold), then "<name>: tables of 2^32 rows or more"
int check_tile_table(const gsim_db* db, const char* name);
// INVALID "<name>: the cutoff must be in (0, 1]"; with k, "<name>: k must be in [1, GSIM_KNN_MAX_K = 128]" in front of it
int check_cutoff(const char* name, float cutoff);
int check_k_cutoff(const char* name, uint32_t k, float cutoff);

// The call on the handle's one shard, which check_table_state has passed: one call at a time per handle; NOMEM `nomem_what` when
// core(shard) runs out of host memory; a failed core may have stopped between its launches, so the shard is marked and the next
// enqueue re-zeroes the search state (rezero_dirty_state).
template <class Fn> int on_one_shard(gsim_db* db, const char* nomem_what, Fn&& core)
{
    std::lock_guard<std::mutex> guard(db->search_mutex);
    Shard& s = db->shards[0];
    int rc;
    try {
        rc = core(s);
    } catch (const std::bad_alloc&) {
        rc = fail(GSIM_ERR_NOMEM, nomem_what);
    }
    if (rc != GSIM_OK) s.state_dirty = true;
    return rc;
}

// ---- the labelling tail of gsim_db_components and gsim_db_jarvis_patrick: nlevels flattened forests of N rows -> the outputs ----

struct ForestLabels {
    DevBuf<uint32_t> d_comp, d_first, d_sizes, d_ncomp, d_flag, d_num;
    uint32_t ncomp[gsim::kCompMaxLevels] = {}; // trees per level
    uint64_t unions = 0;                       // N - ncomp[l], summed: what the caller's hook counter must say
    std::vector<unsigned long long> ctl;       // the caller's control block, read back with the counts
    EventPair ev_label, ev_d2h;                // around the label launches; around the copies

    // NOMEM "device memory for <prefix> (<of>)", "(first_row)", "(sizes)" -- the two where asked for --, "(the counts)", "(label scratch)"
    int alloc(uint64_t N, uint32_t nlevels, bool first_row, bool sizes, const char* prefix, const char* of);
    // The sizes' memset and the label launches (scratch `tmp`: scan_u32_bytes(N)); the copies of the counts, of d_ctl's ctl_words
    // words and of the labels; the wait; STATE "<prefix>: the device reported an impossible count"; the first ncomp[l] entries of
    // first_row and sizes per level (the rest of a stripe is left untouched); the second wait.
    int run(const uint32_t* parent, uint64_t N, uint32_t nlevels, uint32_t row_base, void* tmp, size_t tmp_bytes, const void* d_ctl,
            size_t ctl_words, uint32_t* labels, uint32_t* first_row, uint32_t* sizes, hipStream_t st, const char* prefix);
};

// ---- the core of the score matrices (capi_scores.cpp), which gsim_db_linkage (capi_linkage.cpp) fills its matrix with ----

struct ScoresCall {
    uint64_t r0, nr; // the table rows [r0, r0 + nr)
    int metric;
    float alpha, beta;
    float* out;      // host output (nullptr: the device call)
    float* d_out;    // device output
    uint64_t ld;
    gsim_scores_stats* stats;
};

// left rows d_left[0 .. nl) (W words each, on s's device) against s's table rows [c.r0, c.r0 + c.nr): the launch plan, the
// launches and -- with host output -- the staging slabs; waits for the stream
int scores(gsim_db* db, Shard& s, const uint32_t* d_left, uint64_t nl, const ScoresCall& c);

// ---- the label sort of gsim_db_label_counts and gsim_db_label_sums (capi_labels.cpp; the device side is gsim_labels.hip) ----

// keys = min(label, nlabels) and row numbers, one stable radix sort, the segment starts: the rows of a label become one ascending
// segment of vals2, GSIM_LABEL_NONE sorts behind every label.  The call's 16 bytes a row beside the labels themselves.
struct LabelSort {
    DevBuf<uint32_t> keys, vals; // before the sort
    DevBuf<uint32_t> keys2;      // the label of every sorted position ...
    DevBuf<uint32_t> vals2;      // ... and its table row (r0 + the index into the labels)
    DevBuf<uint32_t> first;      // nlabels + 1 segment starts; first[nlabels]: the labelled rows
    DevBuf<> tmp;
    size_t tmp_bytes = 0;
    std::vector<uint32_t> h_first; // first on the host, once the stream has been waited for

    // NOMEM "device memory for <what> (sort keys)", ... in the order above
    int alloc(uint64_t n, uint32_t nlabels, const char* what);
    // The labels of the n > 0 rows from table row r0 on -- h_labels (copied into d_labels first) or d_labels as it is: enqueues the
    // keys, the sort, the starts and their copy into h_first
    int enqueue(const uint32_t* h_labels, uint32_t* d_labels, uint64_t n, uint32_t nlabels, uint64_t r0, hipStream_t st);
};

} // namespace gsim_host
