// capi_pairs.h -- what gsim_db_neighbors (capi_neighbors.cpp) and the threshold joins (capi_join.cpp) share: the result
// object, the handle's pair buffer with its overflow / exact-regrow protocol, the tile kernel's launch plan, and the CSR
// build.  Implemented in capi_pairs.cpp.  Internal.
#pragma once

#include "capi_internal.h"

#include <functional>

struct gsim_graph {
    std::vector<uint64_t> indptr;
    std::vector<uint32_t> indices;
    std::vector<float> scores;
    gsim_graph_stats stats{};
    enum class Kind : uint8_t { kNeighbors, kJoin, kKnn, kKnnJoin }; // who made it: which of the *_get_*_stats accessors answers for it
    Kind kind = Kind::kNeighbors;
    gsim_join_stats join{}; // kJoin (gsim_db_join / gsim_db_join_queries)
    gsim_knn_stats knn{};   // kKnn (gsim_db_knn, capi_knn.cpp)
    gsim_knn_join_stats knn_join{}; // kKnnJoin (gsim_db_knn_join / gsim_db_knn_queries, capi_knn_join.cpp)
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

// The fold launches of gsim_db_knn and gsim_db_mst over nout owner rows x N candidate rows (capi_knn.cpp has the rule)
struct KnnLaunch {
    uint32_t ot0, not_; // owner tiles
    uint64_t c0, c1;    // candidate rows
};
std::vector<KnnLaunch> plan_knn(uint64_t nout, uint64_t N, uint32_t WP, long long pairs);

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

} // namespace gsim_host
