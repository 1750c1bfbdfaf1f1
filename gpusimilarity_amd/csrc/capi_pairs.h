// capi_pairs.h -- the units more than one call runs, by section: the result object; the pair buffer, tile plan and CSR build of
// gsim_db_neighbors and the threshold joins (capi_pairs.cpp); the fold plans and the CSR build of the k-NN lists (capi_knn_join.cpp,
// capi_pairs.cpp); the CSR checks, forest and numbering of the host functions (capi_pairs.cpp); the round loop, order E and edge
// checks of the two spanning forests (capi_mst.cpp); the k-NN list pass of gsim_db_knn, the shared-neighbour calls and the core
// scores (capi_knn.cpp).  Internal.
#pragma once

#include "capi_internal.h"

#include <functional>

struct gsim_graph {
    std::vector<uint64_t> indptr;
    std::vector<uint32_t> indices;
    std::vector<float> scores;
    gsim_graph_stats stats{};
    enum class Kind : uint8_t { kNeighbors, kJoin, kKnn, kKnnJoin, kSnn }; // who made it: which of the *_get_*_stats accessors answers for it
    Kind kind = Kind::kNeighbors;
    gsim_join_stats join{}; // kJoin (gsim_db_join / gsim_db_join_queries)
    gsim_knn_stats knn{};   // kKnn (gsim_db_knn, capi_knn.cpp)
    gsim_knn_join_stats knn_join{}; // kKnnJoin (gsim_db_knn_join / gsim_db_knn_queries, capi_knn_join.cpp)
    gsim_snn_stats snn{};           // kSnn (gsim_db_snn, capi_snn.cpp) ...
    std::vector<uint32_t> shared;   // ... and its count per entry (gsim_graph_copy_shared)
};

namespace gsim_host
{

struct NbrLaunch {
    uint32_t rt0, nrt, ct0, nct;
};
// Tiles (kNbrTile x kNbrTile pairs of rows of WP words) one launch may cover: the work budget over a tile's price.
uint64_t launch_tile_budget(uint32_t WP);
// Tile launches of a call over nlt tile rows x nct tile columns (rows of WP words), each within the work budget.
std::vector<NbrLaunch> plan_launches(uint64_t nlt, uint64_t nct, bool tri, uint32_t WP);
// ... each of at most pair_budget pairs instead (at least one tile; 0: the work budget) -- gsim_db_components' knob
std::vector<NbrLaunch> plan_launches(uint64_t nlt, uint64_t nct, bool tri, uint32_t WP, uint64_t pair_budget);

// The column segments and fold launches of gsim_db_knn_join* over nl owner rows x N table rows on num_cus compute units
// (capi_knn_join.cpp has the rule; `segments`, `pairs`: GSIM_KNN_JOIN_SEGMENTS, GSIM_KNN_JOIN_LAUNCH_PAIRS).  Pure.  With
// segments == 0 the partial lists, nl x S x k x 8 bytes, stay below 2 x (2 x num_cus) x 256 x k x 8: 256 MiB at k = 128, 256 CUs.
struct KnnJoinLaunch {
    uint32_t ot0, not_; // owner tiles
    uint64_t r0, r1;    // rows of every segment, counted from the segment's first row (gsim::knn_join_seg_begin)
};
struct KnnJoinPlan {
    uint32_t segments = 1;
    std::vector<KnnJoinLaunch> launches;
};
KnnJoinPlan plan_knn_join(uint64_t nl, uint64_t N, uint32_t WP, int num_cus, int segments, long long pairs);
// The fold launches of gsim_db_knn and gsim_db_mst over nout owner rows x N candidate rows: plan_knn_join's with one segment,
// whose rows are the table's
struct KnnLaunch {
    uint32_t ot0, not_; // owner tiles
    uint64_t c0, c1;    // candidate rows
};
std::vector<KnnLaunch> plan_knn(uint64_t nout, uint64_t N, uint32_t WP, long long pairs);

// Where a launch appends: the shard's pair buffer as it is now
struct PairSink {
    unsigned long long* keys;
    float* vals;
    unsigned long long* cursor;
    uint64_t cap;
};
using PairLaunchFn = std::function<int(size_t l, const PairSink& sink)>; // enqueue launch l of the call on the shard's stream
struct PairRun {
    uint64_t total = 0;  // entries the call appended
    uint64_t rerun = 0;  // launches run a second time
    double ms = 0.0;     // HIP events around all launches, reruns included
};
// The n launches of a call, in order, each followed by a snapshot of the cursor (d_snap: n words; d_cursor is zeroed here).  If
// they appended more than the buffer holds it grows to the exact size (GSIM_ERR_NOMEM if it cannot; the buffer is then as it
// was), keeps what the launches before the first overflowing one appended, and runs the others once more; a different count
// on that second pass is GSIM_ERR_STATE.  Returns with the stream idle.
int run_pair_launches(Shard& s, size_t n, unsigned long long* d_cursor, unsigned long long* d_snap, const PairLaunchFn& launch, PairRun* out);

// The pair buffer's `total` entries (keys = list << 32 | column) -> g's CSR over nout lists, columns + db->row_base; each list
// by column (GSIM_JOIN_BY_ROW) or by (score descending, column) (GSIM_JOIN_BY_SCORE).  Fills g->stats.csr_ms / d2h_ms.
int build_pair_csr(gsim_db* db, Shard& s, uint64_t total, uint64_t nout, int order, gsim_graph* g);

// The k-NN calls' lists (nout of them, k slots each, `len` entries used; one more length, zero) -> g's CSR, columns +
// db->row_base: offsets by a scan (scratch `tmp`) into d_indptr, then, once the host has seen the total, compaction into
// device memory of the name `csr_what`.  The control block `ctl` comes back with the offsets, in the same group of copies.
// STATE "<prefix>: the device reported impossible list lengths".  Returns with the stream idle.
struct KnnCsr {
    uint64_t total = 0;                  // entries of the CSR
    double csr_ms = 0.0, d2h_ms = 0.0;   // HIP events; csr_ms spans the host's look at the total: offsets, one small read, compaction
    std::vector<unsigned long long> ctl; // the control block as the fold (and merge) launches left it
    DevBuf<uint32_t> d_indices;          // the compacted arrays: the caller's to free, after it has taken its wall time
    DevBuf<float> d_scores;
};
int build_knn_csr(gsim_db* db, Shard& s, const gsim::KnnEntry* lists, const uint32_t* len, uint64_t nout, uint32_t k, const DevBuf<>& tmp,
                  uint64_t* d_indptr, const DevBuf<>& ctl, const char* csr_what, const char* prefix, gsim_graph* g, KnnCsr* out);
// g->stats from the fields that gsim_knn_stats and gsim_knn_join_stats share, once those are final
template <class Stats> void mirror_graph_stats(const Stats& ks, uint64_t launches, double tile_ms, gsim_graph_stats* gs)
{
    gs->launches = launches;
    gs->pairs = ks.entries;
    gs->tile_ms = tile_ms;
    gs->csr_ms = ks.csr_ms;
    gs->d2h_ms = ks.d2h_ms;
    gs->clock_mhz = ks.clock_mhz;
    gs->wall_ms = ks.wall_ms;
}

// ---- the host functions on a caller's graph (gsim_butina, gsim_components, gsim_mst, gsim_mst_linkage, gsim_mst_cut) ----

// INVALID "more than 2^32-1 rows", "indptr[0] must be 0", "indptr must not decrease"; *nnz = indptr[nrows]
int check_csr_offsets(const uint64_t* indptr, uint64_t nrows, uint64_t* nnz);
// INVALID "NULL indices" when nnz > 0, "column index outside the graph"
int check_csr_indices(const uint32_t* indices, uint64_t nnz, uint64_t nrows);

// union-find over rows: `root` with path halving
struct Forest {
    std::vector<uint32_t> parent;
    explicit Forest(uint64_t n) : parent(n)
    {
        for (uint64_t r = 0; r < n; r++) parent[r] = static_cast<uint32_t>(r);
    }
    uint32_t root(uint32_t x)
    {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    }
    // the smaller index wins every hook, so a tree's root is its smallest row
    bool unite(uint32_t a, uint32_t b)
    {
        const uint32_t x = root(a), y = root(b);
        if (x == y) return false;
        parent[std::max(x, y)] = std::min(x, y);
        return true;
    }
};
// The trees of f numbered by ascending first row: component_of [nrows], and per component (where not NULL) first_row and sizes.
// Returns the number of components.
uint32_t number_components(Forest& f, uint64_t nrows, uint32_t* component_of, uint32_t* first_row, uint32_t* sizes);

// ---- what gsim_db_mst and the mutual-reachability forests share (capi_mst.cpp; capi_hdbscan.cpp calls them) ----

// What differs between the two forests on the device: `prepare` (or nothing) fills more device state once the padded table is ready,
// before the first round -- it may wait for the stream --; `fold` enqueues one fold launch (gsim::launch_mst_fold's arguments).
struct ForestFold {
    std::function<int(const PaddedRows& table, hipStream_t st)> prepare;
    std::function<hipError_t(const gsim::MstArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t nchunk, hipStream_t st)> fold;
};
// The Boruvka rounds of a forest call on the handle's one shard: the call's device memory, the round loop, the sort into order E
// (row_base added to both rows of an edge) and the copy to the host.  N < 2 returns before `prepare`.
int boruvka_forest(gsim_db* db, Shard& s, float cutoff, int metric, float alpha, float beta, uint32_t row_base, const ForestFold& ff,
                   gsim_mst_edge* edges, uint64_t* nedges, gsim_mst_stats* st);
// order E
bool before_in_e(const gsim_mst_edge& x, const gsim_mst_edge& y);
// INVALID "NULL edges", "more than 2^32-1 rows", "mst: an edge needs a < b < nrows", "mst: an edge with a NaN score"
int check_edges(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows);
// gsim_mst's checks of its graph and of the edge buffer: the CSR checks above, "NULL indices or scores", "NULL edges" with nrows > 1,
// "mst: an edge with a NaN score"
int check_scored_csr(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows, const gsim_mst_edge* edges,
                     uint64_t* nnz);
// Kruskal over the pairs a < b of `all` (sorted here into order E; repeated pairs are harmless) -> edges, in order E; their number
uint64_t kruskal_in_e(std::vector<gsim_mst_edge>& all, uint64_t nrows, gsim_mst_edge* edges);

// ---- the k-NN list pass: gsim_db_knn, the shared-neighbour pass (capi_snn.cpp), the core pass (capi_hdbscan.cpp) ----

// The lists of the owner rows [rb, re) of a table of N rows, k slots each, with their lengths, the plan and the control block:
// `front` words of counters ([0] the fold's inserts, the rest the caller's), 4 clock stamps per fold launch, `back` words more of
// the caller's.  k == 0 is a list of no slots: nothing but the control block is allocated, nothing launched.
struct KnnListPass {
    struct Names {
        const char *lists, *len, *ctl; // of the three allocations, after "device memory for "
    };
    DevBuf<gsim::KnnEntry> lists;
    DevBuf<uint32_t> len;
    DevBuf<> ctl;
    std::vector<KnnLaunch> plan;
    LaunchClocks clocks;
    EventPair ev_fold;
    size_t front = 1, ctl_words = 0;
    gsim::KnnArgs args{};                      // what alloc knows of the fold's arguments

    unsigned long long* word(size_t w) const { return ctl.as<unsigned long long>() + w; }
    size_t back_at() const { return front + LaunchClocks::kWords * plan.size(); } // where the caller's `back` words begin

    // the plan; the three allocations, by these names; lengths (`total`: one more, which build_knn_csr's scan makes the total) and block zeroed
    int alloc(const gsim_db* db, uint64_t N, uint32_t WP, uint64_t rb, uint64_t re, uint32_t k, size_t front, size_t back, bool total,
              const Names& names, hipStream_t st);
    // the plan's fold launches on the prepared table, every launch with its clock words, HIP events (ev_fold) around all of them
    int fold(const PaddedRows& table, float cutoff, int metric, float alpha, float beta, hipStream_t st);
    void add_clocks(const unsigned long long* h_ctl) { clocks.add(h_ctl + front, plan.size()); } // from a host copy of the block
};

} // namespace gsim_host
