// capi_neighbors.cpp -- gsim_db_neighbors (every pair of rows at or above a cutoff, as CSR) and gsim_butina (Taylor-Butina
// clustering of such a graph, host code).  The device side is gsim_neighbors.hip.
#include "capi_internal.h"

#include <chrono>
#include <numeric>

struct gsim_graph {
    std::vector<uint64_t> indptr;
    std::vector<uint32_t> indices;
    std::vector<float> scores;
    gsim_graph_stats stats{};
};

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

namespace
{

// device memory owned for the length of one call
struct DevBuf {
    void* p = nullptr;
    ~DevBuf()
    {
        if (p) (void) hipFree(p);
    }
    hipError_t alloc(size_t bytes)
    {
        return hipMalloc(&p, bytes ? bytes : 16);
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair()
    {
        if (a) (void) hipEventDestroy(a);
        if (b) (void) hipEventDestroy(b);
    }
    hipError_t create()
    {
        hipError_t e = hipEventCreate(&a);
        return e == hipSuccess ? hipEventCreate(&b) : e;
    }
    double ms() const
    {
        float t = 0.0f;
        return hipEventElapsedTime(&t, a, b) == hipSuccess ? static_cast<double>(t) : 0.0;
    }
};

struct NbrLaunch {
    uint32_t rt0, nrt, ct0, nct;
};

// Tile launches of a call: consecutive tile rows share a launch while their tiles fit the budget; a tile row longer than
// the budget is cut into column pieces.  Triangle: tile row r holds the tiles r .. nct - 1 (the grid of a group starts at
// its first row's diagonal; the tiles left of a later row's diagonal return at once).
std::vector<NbrLaunch> plan_launches(uint64_t nlt, uint64_t nct, bool tri, uint32_t WP)
{
    const double per_tile = static_cast<double>(gsim::kNbrTile) * gsim::kNbrTile * (2.0 * (WP + 8) + kNbrEmitCost);
    const uint64_t max_tiles = std::max<uint64_t>(1, static_cast<uint64_t>(kNbrLaunchBudget / per_tile));
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

// d_clk: 4 words per launch (gsim::NbrArgs::clk)
int run_launches(const gsim::NbrArgs& a0, const std::vector<NbrLaunch>& plan, size_t first, unsigned long long* d_snap,
                 unsigned long long* d_clk, hipStream_t st)
{
    gsim::NbrArgs a = a0;
    for (size_t l = first; l < plan.size(); l++) {
        a.clk = d_clk + 4 * l;
        GSIM_HIP(gsim::launch_nbr_tiles(a, plan[l].rt0, plan[l].nrt, plan[l].ct0, plan[l].nct, st));
        GSIM_HIP(gsim::launch_nbr_snap(a.cursor, d_snap + l, st));
    }
    return GSIM_OK;
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

int neighbors(gsim_db* db, Shard& s, float cutoff, int metric, float alpha, float beta, uint64_t rb, uint64_t re, gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint64_t nout = re - rb;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    const bool tri = rb == 0 && re == N;
    g->indptr.assign(nout + 1, 0);
    if (nout == 0 || N < 2) {
        g->stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    // popc of every row, and the rows zero-padded to WP words unless they already are WP words
    DevBuf pop, pad;
    GSIM_HIP(pop.alloc(N * 4));
    if (WP != s.W) GSIM_HIP(pad.alloc(N * WP * 4));
    GSIM_HIP(gsim::launch_nbr_prepare(s.d_rows, N, s.W, WP, pad.as<uint32_t>(), pop.as<uint32_t>(), st));

    const uint64_t nlt = (nout + gsim::kNbrTile - 1) / gsim::kNbrTile;
    const uint64_t nct = (N + gsim::kNbrTile - 1) / gsim::kNbrTile;
    const std::vector<NbrLaunch> plan = plan_launches(nlt, nct, tri, WP);
    DevBuf ctl; // [0] the cursor, [1 + l] the cursor after launch l, then 4 clock stamps per launch
    GSIM_HIP(ctl.alloc((1 + 5 * plan.size()) * 8));
    unsigned long long* d_cursor = ctl.as<unsigned long long>();
    unsigned long long* d_snap = d_cursor + 1;
    unsigned long long* d_clk = d_snap + plan.size();
    GSIM_HIP(hipMemsetAsync(d_cursor, 0, 8, st));
    if (!s.d_nbr_keys) {
        GSIM_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_nbr_keys), kNbrInitCap * 8));
        GSIM_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_nbr_vals), kNbrInitCap * 4));
        s.nbr_cap = kNbrInitCap;
    }
    gsim::NbrArgs a{};
    a.rows = WP != s.W ? pad.as<uint32_t>() : static_cast<const uint32_t*>(s.d_rows);
    a.pop = pop.as<uint32_t>();
    a.nrows = N;
    a.row_begin = rb;
    a.row_end = re;
    a.WP = WP;
    a.tri = tri ? 1 : 0;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;
    a.keys = s.d_nbr_keys;
    a.vals = s.d_nbr_vals;
    a.cursor = d_cursor;
    a.cap = s.nbr_cap;

    EventPair ev_tile, ev_rerun, ev_csr, ev_d2h;
    GSIM_HIP(ev_tile.create());
    GSIM_HIP(ev_csr.create());
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipEventRecord(ev_tile.a, st));
    int rc = run_launches(a, plan, 0, d_snap, d_clk, st);
    if (rc != GSIM_OK) return rc;
    GSIM_HIP(hipEventRecord(ev_tile.b, st));
    std::vector<unsigned long long> snap(plan.size());
    GSIM_HIP(hipMemcpyAsync(snap.data(), d_snap, plan.size() * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    const uint64_t total = snap.back();
    g->stats.launches = plan.size();
    g->stats.tile_ms = ev_tile.ms();
    if (total > s.nbr_cap) {
        // the launches from the first one that overflowed on: grow the buffer to the exact size, keep what the launches
        // before them appended, run them once more
        size_t lf = 0;
        while (snap[lf] <= s.nbr_cap) lf++;
        const unsigned long long kept = lf ? snap[lf - 1] : 0;
        unsigned long long* nk = nullptr;
        float* nv = nullptr;
        GSIM_HIP(hipMalloc(reinterpret_cast<void**>(&nk), total * 8));
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&nv), total * 4);
        if (e == hipSuccess && kept) e = hipMemcpyAsync(nk, s.d_nbr_keys, kept * 8, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && kept) e = hipMemcpyAsync(nv, s.d_nbr_vals, kept * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void) hipFree(nk);
            if (nv) (void) hipFree(nv);
            return fail_hip(e, "growing the neighbour buffer");
        }
        (void) hipFree(s.d_nbr_keys);
        (void) hipFree(s.d_nbr_vals);
        s.d_nbr_keys = nk;
        s.d_nbr_vals = nv;
        s.nbr_cap = total;
        a.keys = nk;
        a.vals = nv;
        a.cap = total;
        GSIM_HIP(ev_rerun.create());
        if (lf) GSIM_HIP(hipMemcpyAsync(d_cursor, d_snap + lf - 1, 8, hipMemcpyDeviceToDevice, st));
        else GSIM_HIP(hipMemsetAsync(d_cursor, 0, 8, st));
        GSIM_HIP(hipEventRecord(ev_rerun.a, st));
        rc = run_launches(a, plan, lf, d_snap, d_clk, st);
        if (rc != GSIM_OK) return rc;
        GSIM_HIP(hipEventRecord(ev_rerun.b, st));
        GSIM_HIP(hipMemcpyAsync(snap.data(), d_snap, plan.size() * 8, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipStreamSynchronize(st));
        if (snap.back() != total) return fail(GSIM_ERR_STATE, "neighbour launches found a different number of pairs when run again");
        g->stats.launches_rerun = plan.size() - lf;
        g->stats.tile_ms += ev_rerun.ms();
    }
    g->stats.pairs = tri ? total / 2 : total;
    {
        std::vector<unsigned long long> clk(4 * plan.size());
        GSIM_HIP(hipMemcpyAsync(clk.data(), d_clk, clk.size() * 8, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipStreamSynchronize(st));
        double cyc = 0.0, ticks = 0.0;
        for (size_t l = 0; l < plan.size(); l++) {
            cyc += static_cast<double>(clk[4 * l + 2] - clk[4 * l]);
            ticks += static_cast<double>(clk[4 * l + 3] - clk[4 * l + 1]);
        }
        g->stats.clock_mhz = ticks > 0.0 ? cyc / ticks * 100.0 : 0.0; // wall clock: 100 MHz
    }

    // CSR: sort the keys (row, column), then the row offsets and the column indices
    const uint32_t end_bit = 32 + bit_width(nout - 1);
    DevBuf keys2, vals2, d_indptr, d_indices, tmp;
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::nbr_sort_bytes(total, end_bit, &tmp_bytes));
    GSIM_HIP(keys2.alloc(total * 8));
    GSIM_HIP(vals2.alloc(total * 4));
    GSIM_HIP(d_indptr.alloc((nout + 1) * 8));
    GSIM_HIP(d_indices.alloc(total * 4));
    GSIM_HIP(tmp.alloc(tmp_bytes));
    GSIM_HIP(hipEventRecord(ev_csr.a, st));
    GSIM_HIP(gsim::launch_nbr_csr(tmp.p, tmp_bytes, s.d_nbr_keys, s.d_nbr_vals, keys2.as<unsigned long long>(), vals2.as<float>(), total, end_bit,
                                  nout, db->row_base, d_indptr.as<uint64_t>(), d_indices.as<uint32_t>(), st));
    GSIM_HIP(hipEventRecord(ev_csr.b, st));
    g->indices.resize(total);
    g->scores.resize(total);
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    GSIM_HIP(hipMemcpyAsync(g->indptr.data(), d_indptr.p, (nout + 1) * 8, hipMemcpyDeviceToHost, st));
    if (total) {
        GSIM_HIP(hipMemcpyAsync(g->indices.data(), d_indices.p, total * 4, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipMemcpyAsync(g->scores.data(), vals2.p, total * 4, hipMemcpyDeviceToHost, st));
    }
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st));
    g->stats.csr_ms = ev_csr.ms();
    g->stats.d2h_ms = ev_d2h.ms();
    if (g->indptr[nout] != total) return fail(GSIM_ERR_STATE, "neighbour CSR: row offsets do not add up");
    g->stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_neighbors(gsim_db* db, float cutoff, int metric, float alpha, float beta, uint64_t row_begin, uint64_t row_end,
                      gsim_graph** out)
{
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, "neighbour cutoff must be in (0, 1]");
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    if (metric == GSIM_METRIC_TVERSKY && !(alpha == beta))
        return fail(GSIM_ERR_INVALID, "neighbour lists need a symmetric metric (Tversky with alpha == beta)");
    if (gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "neighbour lists support rows of up to 4096 bits");
    if (row_begin > row_end || row_end > db->nrows) return fail(GSIM_ERR_INVALID, "row range outside the table");
    if (!db->finalized) return fail(GSIM_ERR_STATE, "table not finalized (no rows on a GPU)");
    if (db->fold > 1) return fail(GSIM_ERR_STATE, "neighbour lists do not support folded tables");
    if (db->shards.size() != 1) return fail(GSIM_ERR_STATE, "neighbour lists need a single-shard handle");
    std::lock_guard<std::mutex> guard(db->search_mutex);
    gsim_graph* g = new (std::nothrow) gsim_graph;
    if (!g) return fail(GSIM_ERR_NOMEM, "graph");
    int rc;
    try {
        rc = neighbors(db, db->shards[0], cutoff, metric, alpha, beta, row_begin, row_end, g);
    } catch (const std::bad_alloc&) {
        rc = fail(GSIM_ERR_NOMEM, "host memory for the neighbour lists");
    }
    if (rc != GSIM_OK) {
        delete g;
        return rc;
    }
    *out = g;
    return GSIM_OK;
}

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

int gsim_graph_destroy(gsim_graph* g)
{
    delete g;
    return GSIM_OK;
}

int gsim_butina(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, uint32_t* cluster_of, uint32_t* centroids,
                uint64_t* nclusters)
{
    if (!indptr || !cluster_of || !centroids || !nclusters) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "more than 2^32-1 rows");
    if (indptr[0] != 0) return fail(GSIM_ERR_INVALID, "indptr[0] must be 0");
    for (uint64_t r = 0; r < nrows; r++)
        if (indptr[r + 1] < indptr[r]) return fail(GSIM_ERR_INVALID, "indptr must not decrease");
    const uint64_t nnz = indptr[nrows];
    if (nnz && !indices) return fail(GSIM_ERR_INVALID, "NULL indices");
    for (uint64_t e = 0; e < nnz; e++)
        if (indices[e] >= nrows) return fail(GSIM_ERR_INVALID, "column index outside the graph");
    try {
        // candidates: (neighbour count desc, row desc)
        std::vector<uint32_t> order(nrows);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            const uint64_t cx = indptr[x + 1] - indptr[x], cy = indptr[y + 1] - indptr[y];
            return cx != cy ? cx > cy : x > y;
        });
        std::vector<char> assigned(nrows, 0);
        uint32_t nc = 0;
        for (const uint32_t r : order) {
            if (assigned[r]) continue;
            assigned[r] = 1;
            cluster_of[r] = nc;
            centroids[nc] = r;
            for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++) {
                const uint32_t j = indices[e];
                if (!assigned[j]) {
                    assigned[j] = 1;
                    cluster_of[j] = nc;
                }
            }
            nc++;
        }
        *nclusters = nc;
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "butina");
    }
    return GSIM_OK;
}

} // extern "C"
