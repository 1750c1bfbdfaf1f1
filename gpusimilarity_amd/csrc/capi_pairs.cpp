// capi_pairs.cpp -- the host side that gsim_db_neighbors and the threshold joins share (capi_pairs.h), and the accessors of
// their result object.
#include "capi_pairs.h"

namespace gsim_host
{

// Entries (one per listed pair) the pair buffer holds on a handle's first call; it grows to the exact size a call needed
// and stays with the handle.
constexpr uint64_t kNbrInitCap = 1ull << 20;
// Work per tile-kernel launch, in units of one word-pair of the VALU engine: a pair costs WP + 8 (inner product and keep
// test) when it is dropped; priced here for the case where EVERY pair of the launch is kept -- both passes of the tile,
// 2 (WP + 8), plus kNbrEmitCost for its 24 bytes of stores -- so that no launch comes near 50 ms at any table size and
// any output density (measured on tables of identical rows).  ~2.5 ms per launch on sparse output.
constexpr double kNbrLaunchBudget = 2.5e11;
constexpr double kNbrEmitCost = 150.0;

// Consecutive tile rows share a launch while their tiles fit the budget; a tile row longer than the budget is cut into
// column pieces.  Triangle: tile row r holds the tiles r .. nct - 1 (the grid of a group starts at its first row's diagonal;
// the tiles left of a later row's diagonal return at once).
uint64_t launch_tile_budget(uint32_t WP)
{
    const double per_tile = static_cast<double>(gsim::kNbrTile) * gsim::kNbrTile * (2.0 * (WP + 8) + kNbrEmitCost);
    return std::max<uint64_t>(1, static_cast<uint64_t>(kNbrLaunchBudget / per_tile));
}

std::vector<NbrLaunch> plan_launches(uint64_t nlt, uint64_t nct, bool tri, uint32_t WP)
{
    return plan_launches(nlt, nct, tri, WP, 0);
}

std::vector<NbrLaunch> plan_launches(uint64_t nlt, uint64_t nct, bool tri, uint32_t WP, uint64_t pair_budget)
{
    const uint64_t tile_pairs = static_cast<uint64_t>(gsim::kNbrTile) * gsim::kNbrTile;
    const uint64_t max_tiles = pair_budget ? std::max<uint64_t>(1, pair_budget / tile_pairs) : launch_tile_budget(WP);
    std::vector<NbrLaunch> out;
    uint64_t rt = 0;
    while (rt < nlt) {
        const uint64_t c_lo = tri ? rt : 0;
        const uint64_t ncols = nct - c_lo;
        if (ncols >= max_tiles) {
            for (uint64_t c = c_lo; c < nct; c += max_tiles)
                out.push_back({static_cast<uint32_t>(rt), 1, static_cast<uint32_t>(c), static_cast<uint32_t>(std::min(max_tiles, nct - c))});
            rt++;
            continue;
        }
        uint64_t real = 0, r1 = rt;
        while (r1 < nlt && r1 - rt < 65535) {
            const uint64_t cols = nct - (tri ? r1 : 0);
            if (r1 > rt && real + cols > max_tiles) break;
            real += cols;
            r1++;
        }
        out.push_back({static_cast<uint32_t>(rt), static_cast<uint32_t>(r1 - rt), static_cast<uint32_t>(c_lo), static_cast<uint32_t>(ncols)});
        rt = r1;
    }
    return out;
}

namespace
{

int run_from(Shard& s, size_t first, size_t n, unsigned long long* d_cursor, unsigned long long* d_snap, const PairLaunchFn& launch)
{
    const PairSink sink{s.d_nbr_keys, s.d_nbr_vals, d_cursor, s.nbr_cap};
    for (size_t l = first; l < n; l++) {
        const int rc = launch(l, sink);
        if (rc != GSIM_OK) return rc;
        GSIM_HIP(gsim::launch_nbr_snap(d_cursor, d_snap + l, s.stream));
    }
    return GSIM_OK;
}

int fail_alloc(hipError_t e, const char* what)
{
    if (e == hipErrorOutOfMemory) {
        (void) hipGetLastError();
        return fail(GSIM_ERR_NOMEM, std::string(what) + ": out of device memory");
    }
    return fail_hip(e, what);
}

uint32_t bit_width(uint64_t x)
{
    uint32_t b = 0;
    while (x) {
        b++;
        x >>= 1;
    }
    return b;
}

} // namespace

int run_pair_launches(Shard& s, size_t n, unsigned long long* d_cursor, unsigned long long* d_snap, const PairLaunchFn& launch, PairRun* out)
{
    const hipStream_t st = s.stream;
    *out = PairRun{};
    if (n == 0) return GSIM_OK;
    if (s.nbr_cap == 0) {
        hipError_t e = s.d_nbr_keys.grow_keep(kNbrInitCap * 8);
        if (e == hipSuccess) e = s.d_nbr_vals.grow_keep(kNbrInitCap * 4);
        if (e != hipSuccess) return fail_alloc(e, "the pair buffer");
        s.nbr_cap = kNbrInitCap;
    }
    EventPair ev, ev_rerun;
    GSIM_HIP(ev.create());
    GSIM_HIP(hipMemsetAsync(d_cursor, 0, 8, st));
    GSIM_HIP(hipEventRecord(ev.a, st));
    int rc = run_from(s, 0, n, d_cursor, d_snap, launch);
    if (rc != GSIM_OK) return rc;
    GSIM_HIP(hipEventRecord(ev.b, st));
    std::vector<unsigned long long> snap(n);
    GSIM_HIP(hipMemcpyAsync(snap.data(), d_snap, n * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    const uint64_t total = snap.back();
    out->total = total;
    out->ms = ev.ms();
    if (total <= s.nbr_cap) return GSIM_OK;
    // the launches from the first one that overflowed on: grow the buffer to the exact size, keep what the launches
    // before them appended, run them once more
    size_t lf = 0;
    while (snap[lf] <= s.nbr_cap) lf++;
    const unsigned long long kept = lf ? snap[lf - 1] : 0;
    DevBuf<unsigned long long> nk;
    DevBuf<float> nv;
    hipError_t e = nk.grow(total * 8);
    if (e == hipSuccess) e = nv.grow(total * 4);
    if (e == hipSuccess && kept) e = hipMemcpyAsync(nk, s.d_nbr_keys, kept * 8, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && kept) e = hipMemcpyAsync(nv, s.d_nbr_vals, kept * 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail_alloc(e, "growing the pair buffer"); // (the buffer is as it was)
    s.d_nbr_keys = std::move(nk);
    s.d_nbr_vals = std::move(nv);
    s.nbr_cap = total;
    GSIM_HIP(ev_rerun.create());
    if (lf) GSIM_HIP(hipMemcpyAsync(d_cursor, d_snap + lf - 1, 8, hipMemcpyDeviceToDevice, st));
    else GSIM_HIP(hipMemsetAsync(d_cursor, 0, 8, st));
    GSIM_HIP(hipEventRecord(ev_rerun.a, st));
    rc = run_from(s, lf, n, d_cursor, d_snap, launch);
    if (rc != GSIM_OK) return rc;
    GSIM_HIP(hipEventRecord(ev_rerun.b, st));
    GSIM_HIP(hipMemcpyAsync(snap.data(), d_snap, n * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    if (snap.back() != total) return fail(GSIM_ERR_STATE, "the launches found a different number of pairs when run again");
    out->rerun = n - lf;
    out->ms += ev_rerun.ms();
    return GSIM_OK;
}

int build_pair_csr(gsim_db* db, Shard& s, uint64_t total, uint64_t nout, int order, gsim_graph* g)
{
    const hipStream_t st = s.stream;
    const bool by_score = order == GSIM_JOIN_BY_SCORE;
    // sort the keys (list, column), then the row offsets and the column indices
    const uint32_t end_bit = 32 + bit_width(nout - 1);
    DevBuf<> keys2, vals2, d_indptr, d_indices, tmp;
    EventPair ev_csr, ev_d2h;
    GSIM_HIP(ev_csr.create());
    GSIM_HIP(ev_d2h.create());
    size_t tmp_bytes = 0, tmp2_bytes = 0;
    GSIM_HIP(gsim::nbr_sort_bytes(total, end_bit, &tmp_bytes));
    if (by_score) GSIM_HIP(gsim::join_score_sort_bytes(total, end_bit, &tmp2_bytes));
    tmp_bytes = std::max(tmp_bytes, tmp2_bytes);
    hipError_t e = keys2.grow(total * 8);
    if (e == hipSuccess) e = vals2.grow(total * 4);
    if (e == hipSuccess) e = d_indptr.grow((nout + 1) * 8);
    if (e == hipSuccess) e = d_indices.grow(total * 4);
    if (e == hipSuccess) e = tmp.grow(tmp_bytes);
    if (e != hipSuccess) return fail_alloc(e, "device memory for the CSR build");
    GSIM_HIP(hipEventRecord(ev_csr.a, st));
    GSIM_HIP(gsim::launch_nbr_csr(tmp, tmp_bytes, s.d_nbr_keys, s.d_nbr_vals, keys2.as<unsigned long long>(), vals2.as<float>(), total, end_bit,
                                  nout, db->row_base, d_indptr.as<uint64_t>(), d_indices.as<uint32_t>(), st));
    if (by_score) // (the pair buffer is free again: the second sort's output; the scores come back in vals2)
        GSIM_HIP(gsim::launch_join_by_score(tmp, tmp_bytes, keys2.as<unsigned long long>(), vals2.as<float>(), s.d_nbr_keys,
                                            s.d_nbr_vals.as<uint32_t>(), total, end_bit, nout, db->row_base,
                                            d_indptr.as<uint64_t>(), d_indices.as<uint32_t>(), vals2.as<float>(), st));
    GSIM_HIP(hipEventRecord(ev_csr.b, st));
    g->indices.resize(total);
    g->scores.resize(total);
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    GSIM_HIP(hipMemcpyAsync(g->indptr.data(), d_indptr, (nout + 1) * 8, hipMemcpyDeviceToHost, st));
    if (total) {
        GSIM_HIP(hipMemcpyAsync(g->indices.data(), d_indices, total * 4, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipMemcpyAsync(g->scores.data(), vals2, total * 4, hipMemcpyDeviceToHost, st));
    }
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st));
    g->stats.csr_ms = ev_csr.ms();
    g->stats.d2h_ms = ev_d2h.ms();
    if (g->indptr[nout] != total) return fail(GSIM_ERR_STATE, "pair CSR: row offsets do not add up");
    return GSIM_OK;
}

int build_knn_csr(gsim_db* db, Shard& s, const gsim::KnnEntry* lists, const uint32_t* len, uint64_t nout, uint32_t k, const DevBuf<>& tmp,
                  uint64_t* d_indptr, const DevBuf<>& ctl, const char* csr_what, const char* prefix, gsim_graph* g, KnnCsr* out)
{
    const hipStream_t st = s.stream;
    DevBuf<uint32_t>& d_indices = out->d_indices;
    DevBuf<float>& d_scores = out->d_scores;
    EventPair ev_csr, ev_d2h;
    GSIM_HIP(ev_csr.create());
    GSIM_HIP(ev_d2h.create());
    // indptr on the device; its last entry sizes the compacted arrays
    GSIM_HIP(hipEventRecord(ev_csr.a, st));
    GSIM_HIP(gsim::launch_knn_offsets(tmp, tmp.bytes(), len, nout + 1, d_indptr, st));
    out->ctl.resize(ctl.bytes() / 8);
    GSIM_HIP(hipMemcpyAsync(g->indptr.data(), d_indptr, (nout + 1) * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(out->ctl.data(), ctl, ctl.bytes(), hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    const uint64_t total = g->indptr[nout];
    if (total > nout * k) return fail(GSIM_ERR_STATE, std::string(prefix) + ": the device reported impossible list lengths");
    const std::string what = std::string("device memory for ") + csr_what;
    if (d_indices.grow(total * 4) != hipSuccess || d_scores.grow(total * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, what);
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
    out->total = total;
    out->csr_ms = ev_csr.ms();
    out->d2h_ms = ev_d2h.ms();
    return GSIM_OK;
}

int check_csr_offsets(const uint64_t* indptr, uint64_t nrows, uint64_t* nnz)
{
    if (nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "more than 2^32-1 rows");
    if (indptr[0] != 0) return fail(GSIM_ERR_INVALID, "indptr[0] must be 0");
    for (uint64_t r = 0; r < nrows; r++)
        if (indptr[r + 1] < indptr[r]) return fail(GSIM_ERR_INVALID, "indptr must not decrease");
    *nnz = indptr[nrows];
    return GSIM_OK;
}

int check_csr_indices(const uint32_t* indices, uint64_t nnz, uint64_t nrows)
{
    if (nnz && !indices) return fail(GSIM_ERR_INVALID, "NULL indices");
    for (uint64_t e = 0; e < nnz; e++)
        if (indices[e] >= nrows) return fail(GSIM_ERR_INVALID, "column index outside the graph");
    return GSIM_OK;
}

uint32_t number_components(Forest& f, uint64_t nrows, uint32_t* component_of, uint32_t* first_row, uint32_t* sizes)
{
    // rows ascending: a root comes before every other row of its component and takes the next number
    uint32_t nc = 0;
    for (uint64_t r = 0; r < nrows; r++) {
        const uint32_t root = f.root(static_cast<uint32_t>(r));
        if (root == r) {
            component_of[r] = nc;
            if (first_row) first_row[nc] = static_cast<uint32_t>(r);
            if (sizes) sizes[nc] = 1;
            nc++;
        } else {
            component_of[r] = component_of[root];
            if (sizes) sizes[component_of[root]]++;
        }
    }
    return nc;
}

} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_graph_shape(const gsim_graph* g, uint64_t* nrows, uint64_t* nnz)
{
    if (!g) return fail(GSIM_ERR_INVALID, "NULL graph");
    if (nrows) *nrows = g->indptr.size() - 1;
    if (nnz) *nnz = g->indices.size();
    return GSIM_OK;
}

int gsim_graph_copy(const gsim_graph* g, uint64_t* indptr, uint32_t* indices, float* scores)
{
    if (!g) return fail(GSIM_ERR_INVALID, "NULL graph");
    if (indptr) std::memcpy(indptr, g->indptr.data(), g->indptr.size() * sizeof(uint64_t));
    if (indices && !g->indices.empty()) std::memcpy(indices, g->indices.data(), g->indices.size() * sizeof(uint32_t));
    if (scores && !g->scores.empty()) std::memcpy(scores, g->scores.data(), g->scores.size() * sizeof(float));
    return GSIM_OK;
}

int gsim_graph_get_stats(const gsim_graph* g, gsim_graph_stats* out)
{
    if (!g || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    *out = g->stats;
    return GSIM_OK;
}

int gsim_graph_get_join_stats(const gsim_graph* g, gsim_join_stats* out)
{
    if (!g || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (g->kind != gsim_graph::Kind::kJoin) return fail(GSIM_ERR_INVALID, "not the result of a join");
    *out = g->join;
    return GSIM_OK;
}

int gsim_graph_get_knn_stats(const gsim_graph* g, gsim_knn_stats* out)
{
    if (!g || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (g->kind != gsim_graph::Kind::kKnn) return fail(GSIM_ERR_INVALID, "not the result of gsim_db_knn");
    *out = g->knn;
    return GSIM_OK;
}

int gsim_graph_destroy(gsim_graph* g)
{
    delete g;
    return GSIM_OK;
}

} // extern "C"
