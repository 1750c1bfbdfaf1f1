// capi_knobs.cpp -- the tuning knobs' table and its one reader (capi_knobs.h)
#include "capi_knobs.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gsim_device.h" // (kFusedMaxK, kLeaderMaxRound)

namespace gsim_host
{

using K = Knobs;
constexpr unsigned kInt = KnobSpec::kInt, kBool = KnobSpec::kBool, kEmptyIsZero = KnobSpec::kEmptyIsZero;
const KnobSpec kKnobSpecs[] = {
    {"GSIM_FUSED", &K::fused, kNoLo, kNoHi, kInt},
    {"GSIM_FUSED_DEBUG", &K::fused_debug, kNoLo, kNoHi, kInt},
    {"GSIM_FUSED_FLAGS", &K::fused_flags, kNoLo, kNoHi, kInt},
    {"GSIM_LARGEK_BINRANK", &K::largek_binrank, kNoLo, kNoHi, kInt},
    {"GSIM_FUSED_SELECT_MAX_K", &K::fused_select_max_k, 2048, gsim::kFusedMaxK, kInt}, // (the large-k sort takes k > 2048)
    {"GSIM_LARGEK_ONE_BLOCK_MAX", &K::largek_one_block_max, kNoLo, kNoHi, kInt},
    {"GSIM_FUSED_BACKOFF", &K::fused_backoff, kNoLo, kNoHi, kInt},
    {"GSIM_PUBLISH_MIN_ROWS_PER_K", &K::publish_min_rows_per_k, 0, kNoHi, kInt},
    {"GSIM_EACH_LANES", &K::each_lanes, kNoLo, kNoHi, kInt},
    {"GSIM_BATCH_SEG_CAP", &K::batch_seg_cap, kNoLo, kNoHi, kInt},
    {"GSIM_BATCH_SEG_CAP_INIT", &K::batch_seg_cap_init, kNoLo, kNoHi, kInt},
    {"GSIM_BATCH_MFMA_MIN_Q", &K::batch_mfma_min_q, kNoLo, kNoHi, kInt},
    {"GSIM_BATCH_MFMA_DENSE", &K::batch_mfma_dense, kNoLo, kNoHi, kInt},
    {"GSIM_JOIN_STREAM_MAX_ROWS", &K::join_stream_max_rows, kNoLo, kNoHi, kInt},
    {"GSIM_SUBSET_GATHER_MAX_PERMILLE", &K::subset_gather_max_permille, 0, kNoHi, kInt},
    {"GSIM_GROUP_LAUNCH_PAIRS", &K::group_launch_pairs, 0, kNoHi, 0}, // (0: by the row width)
    {"GSIM_LEADER_ROUND", &K::leader_round, 1, gsim::kLeaderMaxRound, kInt},
    {"GSIM_LEADER_LAUNCH_PAIRS", &K::leader_launch_pairs, 0, kNoHi, 0}, // (0: by the row width)
    {"GSIM_KNN_LAUNCH_PAIRS", &K::knn_launch_pairs, 0, kNoHi, 0},       // (0: by the row width)
    {"GSIM_KNN_JOIN_SEGMENTS", &K::knn_join_segments, 0, kNoHi, kInt},  // (0: by the owner tiles and the CUs)
    {"GSIM_KNN_JOIN_LAUNCH_PAIRS", &K::knn_join_launch_pairs, 0, kNoHi, 0}, // (0: by the row width)
    {"GSIM_HIST_STREAM_MAX_ROWS", &K::hist_stream_max_rows, kNoLo, kNoHi, kInt},
    {"GSIM_HIST_LAUNCH_PAIRS", &K::hist_launch_pairs, 0, kNoHi, 0}, // (0: by the row width)
    {"GSIM_HIST_NAIVE_ADD", &K::hist_naive_add, kNoLo, kNoHi, kInt | kBool},
    {"GSIM_SCORES_LAUNCH_PAIRS", &K::scores_launch_pairs, 0, kNoHi, 0}, // (0: by the row width)
    {"GSIM_SCORES_STAGE_BYTES", &K::scores_stage_bytes, 1, kNoHi, 0},   // (at least one row anyway)
    {"GSIM_COMPONENTS_LAUNCH_PAIRS", &K::components_launch_pairs, 0, kNoHi, 0}, // (0: the neighbour lists' plan)
    {"GSIM_DBSCAN_LAUNCH_PAIRS", &K::dbscan_launch_pairs, 0, kNoHi, 0},         // (0: the neighbour lists' plan)
    {"GSIM_DBSCAN_SKIP", &K::dbscan_skip, kNoLo, kNoHi, kInt | kBool | kEmptyIsZero},
    {"GSIM_MST_LAUNCH_PAIRS", &K::mst_launch_pairs, 0, kNoHi, 0},       // (0: by the row width)
    {"GSIM_PROFILE_LAUNCH_ROWS", &K::profile_launch_rows, 0, kNoHi, 0}, // (0: 32 GiB of rows)
    {"GSIM_ASSIGN_LAUNCH_PAIRS", &K::assign_launch_pairs, 0, kNoHi, 0}, // (0: by the row width)
    {"GSIM_LABELS_LAUNCH_ROWS", &K::labels_launch_rows, 0, kNoHi, 0},   // (0: 32 GiB of rows)
};
const size_t kKnobSpecCount = sizeof(kKnobSpecs) / sizeof(kKnobSpecs[0]);

Knobs read_knobs()
{
    Knobs k;
    for (const KnobSpec& s : kKnobSpecs) {
        const char* v = std::getenv(s.name);
        if (!v || (!*v && (s.mode & (kInt | kEmptyIsZero)) == kInt)) continue;
        const long long x = (s.mode & kInt) ? std::atoi(v) : std::atoll(v);
        k.*s.member = (s.mode & kBool) ? (x != 0) : std::min(std::max(x, s.lo), s.hi);
    }
    k.debug_batch = std::getenv("GSIM_DEBUG_BATCH") ? 1 : 0;
    if (const char* v = std::getenv("GSIM_FOLD_RESCORE")) k.fold_rescore_host = std::strcmp(v, "host") == 0;
    return k;
}

} // namespace gsim_host
