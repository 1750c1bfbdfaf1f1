// capi_front.cpp -- the shared fronts of capi_front.h.
#include "capi_front.h"

#include <unordered_set>

namespace gsim_host
{

int check_metric(const char* prefix, int metric, float alpha, float beta)
{
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (metric == GSIM_METRIC_TVERSKY && !(std::isfinite(alpha) && alpha >= 0.0f && std::isfinite(beta) && beta >= 0.0f))
        return fail(GSIM_ERR_INVALID, std::string(prefix) + ": Tversky alpha and beta must be finite and >= 0");
    return GSIM_OK;
}

int check_pair_state(const gsim_db* db, const char* plural, const char* which)
{
    if (!db->finalized) return fail(GSIM_ERR_STATE, std::string(which) + " not finalized (no rows on a GPU)");
    if (db->fold > 1) return fail(GSIM_ERR_STATE, std::string(plural) + " do not support folded tables: " + which);
    if (db->shards.size() != 1) return fail(GSIM_ERR_STATE, std::string(plural) + " need single-shard handles: " + which);
    return GSIM_OK;
}

int check_left_handle(const gsim_db* db, const gsim_db* left, uint64_t lrow_end)
{
    if (!left) return fail(GSIM_ERR_INVALID, "NULL left handle");
    if (lrow_end > left->nrows) return fail(GSIM_ERR_INVALID, "left row range outside the left table");
    if (left->fp_bits != db->fp_bits) return fail(GSIM_ERR_INVALID, "the two handles have different fp_bits");
    return GSIM_OK;
}

int LeftSide::from_handle(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, const char* plural)
{
    int rc = check_pair_state(db, plural, "table");
    if (rc == GSIM_OK && left != db) rc = check_pair_state(left, plural, "left table");
    if (rc != GSIM_OK) return rc;
    if (left->shards[0].device != db->shards[0].device) return fail(GSIM_ERR_STATE, "the two handles are on different devices");
    // One call at a time on either handle.  std::lock takes the two mutexes without an order of its own: f(A, left = B) beside
    // f(B, left = A) on two threads cannot deadlock, as they would if each took `db` first.
    lock_db = std::unique_lock<std::mutex>(db->search_mutex, std::defer_lock);
    if (left != db) {
        lock_left = std::unique_lock<std::mutex>(left->search_mutex, std::defer_lock);
        std::lock(lock_db, lock_left);
    } else {
        lock_db.lock();
    }
    rows = static_cast<const uint32_t*>(left->shards[0].d_rows) + lrow_begin * left->shards[0].W;
    nl = lrow_end - lrow_begin;
    in_table = left == db;
    row0 = lrow_begin;
    return GSIM_OK;
}

int LeftSide::from_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, const char* plural, const char* what, bool upload)
{
    if (nq && !queries) return fail(GSIM_ERR_INVALID, "NULL queries");
    const int rc = check_pair_state(db, plural, "table");
    if (rc != GSIM_OK) return rc;
    lock_db = std::unique_lock<std::mutex>(db->search_mutex);
    Shard& s = db->shards[0];
    if (nq && upload) {
        GSIM_HIP(set_device(s.device));
        const size_t bytes = static_cast<size_t>(nq) * s.W * 4;
        if (d_left.grow(bytes) != hipSuccess) return fail(GSIM_ERR_NOMEM, std::string("device memory for ") + what);
        GSIM_HIP(hipMemcpyAsync(d_left, queries, bytes, hipMemcpyHostToDevice, s.stream));
    }
    rows = d_left.as<uint32_t>();
    nl = nq;
    return GSIM_OK;
}

int check_table_state(const gsim_db* db, const char* subject, bool plural)
{
    if (!db->finalized) return fail(GSIM_ERR_STATE, "table not finalized (no rows on a GPU)");
    if (db->fold > 1) return fail(GSIM_ERR_STATE, std::string(subject) + (plural ? " do not" : " does not") + " support folded tables");
    if (db->shards.size() != 1) return fail(GSIM_ERR_STATE, std::string(subject) + (plural ? " need" : " needs") + " a single-shard handle");
    return GSIM_OK;
}

int check_symmetric_metric(const char* needs, const char* prefix, int metric, float alpha, float beta)
{
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (metric != GSIM_METRIC_TVERSKY) return GSIM_OK;
    if (!(alpha == beta)) return fail(GSIM_ERR_INVALID, std::string(needs) + " a symmetric metric (Tversky with alpha == beta)");
    if (prefix && !(std::isfinite(alpha) && alpha >= 0.0f))
        return fail(GSIM_ERR_INVALID, std::string(prefix) + ": Tversky alpha = beta must be finite and >= 0");
    return GSIM_OK;
}

int check_row_range(const gsim_db* db, uint64_t row_begin, uint64_t row_end)
{
    if (row_begin > row_end) return fail(GSIM_ERR_INVALID, "row range: begin past end");
    if (row_end > db->nrows) return fail(GSIM_ERR_INVALID, "row range outside the table");
    return GSIM_OK;
}

int check_tile_table(const gsim_db* db, const char* name)
{
    if (db->fp_bits > 4096 || gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, std::string(name) + ": rows wider than 4096 bits");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, std::string(name) + ": tables of 2^32 rows or more");
    return GSIM_OK;
}

int check_cutoff(const char* name, float cutoff)
{
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, std::string(name) + ": the cutoff must be in (0, 1]");
    return GSIM_OK;
}

int check_k_cutoff(const char* name, uint32_t k, float cutoff)
{
    if (k < 1 || k > GSIM_KNN_MAX_K) return fail(GSIM_ERR_INVALID, std::string(name) + ": k must be in [1, GSIM_KNN_MAX_K = 128]");
    return check_cutoff(name, cutoff);
}

int ForestLabels::alloc(uint64_t N, uint32_t nlevels, bool first_row, bool sizes, const char* prefix, const char* of)
{
    const std::string w = std::string("device memory for ") + prefix;
    const size_t stripe = static_cast<size_t>(N) * 4, all = stripe * nlevels;
    if (d_comp.grow(all) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (" + of + ")");
    if (first_row && d_first.grow(all) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (first_row)");
    if (sizes && d_sizes.grow(all) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (sizes)");
    if (d_ncomp.grow(gsim::kCompMaxLevels * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (the counts)");
    if (d_flag.grow(stripe) != hipSuccess || d_num.grow(stripe) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + " (label scratch)");
    return GSIM_OK;
}

int ForestLabels::run(const uint32_t* parent, uint64_t N, uint32_t nlevels, uint32_t row_base, void* tmp, size_t tmp_bytes, const void* d_ctl,
                      size_t ctl_words, uint32_t* labels, uint32_t* first_row, uint32_t* sizes, hipStream_t st, const char* prefix)
{
    const size_t all = static_cast<size_t>(N) * 4 * nlevels;
    GSIM_HIP(ev_label.create());
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipEventRecord(ev_label.a, st));
    if (sizes) GSIM_HIP(hipMemsetAsync(d_sizes, 0, all, st));
    for (uint32_t l = 0; l < nlevels; l++)
        GSIM_HIP(gsim::launch_comp_label(tmp, tmp_bytes, parent + l * N, N, row_base, d_flag, d_num, d_comp + l * N,
                                         first_row ? d_first + l * N : nullptr, sizes ? d_sizes + l * N : nullptr, d_ncomp + l, st));
    GSIM_HIP(hipEventRecord(ev_label.b, st));
    ctl.assign(ctl_words, 0);
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    GSIM_HIP(hipMemcpyAsync(ncomp, d_ncomp, nlevels * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(ctl.data(), d_ctl, ctl_words * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(labels, d_comp, all, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    for (uint32_t l = 0; l < nlevels; l++) {
        if (ncomp[l] < 1 || ncomp[l] > N) return fail(GSIM_ERR_STATE, std::string(prefix) + ": the device reported an impossible count");
        unions += N - ncomp[l];
        if (first_row) GSIM_HIP(hipMemcpyAsync(first_row + l * N, d_first + l * N, static_cast<size_t>(ncomp[l]) * 4, hipMemcpyDeviceToHost, st));
        if (sizes) GSIM_HIP(hipMemcpyAsync(sizes + l * N, d_sizes + l * N, static_cast<size_t>(ncomp[l]) * 4, hipMemcpyDeviceToHost, st));
    }
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st));
    return GSIM_OK;
}

int check_seeds(const gsim_db* db, const uint32_t* seeds, uint32_t nseeds, const char* nomem_what)
{
    if (nseeds && !seeds) return fail(GSIM_ERR_INVALID, "NULL seeds");
    try {
        std::unordered_set<uint32_t> seen;
        for (uint32_t j = 0; j < nseeds; j++) {
            if (seeds[j] < db->row_base || static_cast<uint64_t>(seeds[j]) >= db->row_base + db->nrows)
                return fail(GSIM_ERR_INVALID, "seed row outside the table");
            if (!seen.insert(seeds[j]).second) return fail(GSIM_ERR_INVALID, "repeated seed row");
        }
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, nomem_what);
    }
    return GSIM_OK;
}

} // namespace gsim_host
