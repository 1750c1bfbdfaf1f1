// capi_knobs.h -- every tuning knob of the library, read from the environment ONCE per handle -- by gsim_db_create -- and nowhere else
// (INTEGRATION.md lists them with their meaning; nothing under a search entry point calls getenv).  Host code only: no kernel file
// includes it, so a new knob rebuilds the capi_*.o objects alone.  Retired knobs are constants beside their code.
#pragma once

#include <climits>
#include <cstddef>

namespace gsim_host
{

struct Knobs {
    long long fused = 1;                   // GSIM_FUSED               0: every query through the four-kernel pipeline
    long long fused_debug = 0;             // GSIM_FUSED_DEBUG         in-kernel phase stamps
    long long fused_flags = 0;             // GSIM_FUSED_FLAGS
    long long fused_select_max_k = 2048;   // GSIM_FUSED_SELECT_MAX_K  largest k the single launch ranks itself (2048 ... 8192) where it can also publish for the large-k kernels
    long long largek_one_block_max = 32768; // GSIM_LARGEK_ONE_BLOCK_MAX
    long long fused_backoff = 1;           // GSIM_FUSED_BACKOFF       0: a query handed back never routes later ones around the single launch
    long long publish_min_rows_per_k = 0;  // GSIM_PUBLISH_MIN_ROWS_PER_K  tables shorter than this many rows per hit rank large k inside the launch (up
                                     // to round 5: 64 -- short tables publish most of their rows; measured in round 6 the publishing route is
                                     // still 1.5 ... 6 x faster there and hands nothing back: profiles/r06_short_tables_large_k.txt)
    long long largek_binrank = 1;          // GSIM_LARGEK_BINRANK      0: the published rows of a large-k query always go through the radix select + sort
    long long each_lanes = 2;              // GSIM_EACH_LANES          below 2: pipelined queries of small tables never alternate between two half-grid lanes
    long long batch_seg_cap = 65536;       // GSIM_BATCH_SEG_CAP
    long long batch_seg_cap_init = 4096;   // GSIM_BATCH_SEG_CAP_INIT
    long long batch_mfma_min_q = 4;        // GSIM_BATCH_MFMA_MIN_Q    0: batches never take the matrix cores
    long long batch_mfma_dense = 1;        // GSIM_BATCH_MFMA_DENSE    0: dense cutoffs go to the VALU pass
    long long debug_batch = 0;             // GSIM_DEBUG_BATCH         print the batch flags (instrumented builds: phase counters)
    long long fold_rescore_host = 0;       // GSIM_FOLD_RESCORE=host
    long long join_stream_max_rows = 2;    // GSIM_JOIN_STREAM_MAX_ROWS  joins of at most this many left rows stream the table once per left row, larger
                                     // ones take the tile kernel (0: always tiles; DESIGN.md section 11 has the crossover)
    long long subset_gather_max_permille = 250; // GSIM_SUBSET_GATHER_MAX_PERMILLE  gsim_db_search_rows gathers the selected rows when
                                     // selected x max(row bytes, 128) x 1000 <= this x N x row bytes, else streams the table under the
                                     // mask (0: always stream, 1000 or more: always gather; DESIGN.md section 12 has the crossover)
    long long group_launch_pairs = 0; // GSIM_GROUP_LAUNCH_PAIRS  a launch of gsim_db_search_group scores at most this many row x query
                                     // pairs (at least one chunk of rows); 0: by the row width (capi_group.cpp group_launch_pairs;
                                     // DESIGN.md section 13 has the rates and the arithmetic)
    long long leader_round = 256;          // GSIM_LEADER_ROUND        candidates per round of gsim_db_leader (1 ... kLeaderMaxRound); the result
                                     // does not depend on it
    long long leader_launch_pairs = 0; // GSIM_LEADER_LAUNCH_PAIRS  a launch of a gsim_db_leader pass scores at most this many row x leader
                                     // pairs (at least one chunk of rows); 0: by the row width, as group_launch_pairs
    long long knn_launch_pairs = 0;  // GSIM_KNN_LAUNCH_PAIRS    a launch of gsim_db_knn's fold kernel scores at most this many owner x candidate
                                     // pairs (at least one column tile of 256 candidates); 0: by the row width, with the tile
                                     // kernel's pricing and budget (capi_knn.cpp).  The result does not depend on it
    long long knn_join_segments = 0;       // GSIM_KNN_JOIN_SEGMENTS   column segments of a gsim_db_knn_join* call, each folded by workgroups of its
                                     // own and merged afterwards; 0: 1 when the owner tiles alone give two workgroups per CU, else as
                                     // many as make up for it; n: n, at most the table's column tiles and kKnnJoinMaxSegments
                                     // (capi_knn_join.cpp plan_knn_join).  The result does not depend on it
    long long knn_join_launch_pairs = 0; // GSIM_KNN_JOIN_LAUNCH_PAIRS  a launch of gsim_db_knn_join*'s fold kernel scores at most this many
                                     // owner x candidate pairs (at least one column tile of 256 candidates per segment); 0: by the row
                                     // width, as knn_launch_pairs.  The result does not depend on it
    long long hist_stream_max_rows = 32;   // GSIM_HIST_STREAM_MAX_ROWS  histogram calls of at most this many left rows stream the table once per left
                                     // row, larger ones take the owner-tile kernel (0: always tiles; DESIGN.md section 16 has the crossover:
                                     // between 32 and 64 left rows at 1 M and at 100 M x 1024-bit rows)
    long long hist_launch_pairs = 0; // GSIM_HIST_LAUNCH_PAIRS   a launch of either histogram kernel scores at most this many left x table
                                     // pairs (at least one 256 x 256 tile / 64 table rows); 0: by the row width, as knn_launch_pairs.
                                     // The result does not depend on it
    long long hist_naive_add = 0;          // GSIM_HIST_NAIVE_ADD      1: the streaming kernel adds with one LDS atomic per lane instead of one per
                                     // distinct bin of the wave (for timing the two forms; same counts)
    long long scores_launch_pairs = 0; // GSIM_SCORES_LAUNCH_PAIRS  a launch of gsim_db_scores*'s matrix kernel computes at most this many left x
                                     // table pairs (at least one 128 x 128 block); 0: by the padded row width (capi_scores.cpp;
                                     // DESIGN.md section 17).  The result does not depend on it
    long long scores_stage_bytes = 256ll << 20; // GSIM_SCORES_STAGE_BYTES  device staging of the host-output calls: a slab of whole left rows of
                                     // at most this many bytes (at least one row) is computed, then copied out.  The result does not
                                     // depend on it
    long long components_launch_pairs = 0; // GSIM_COMPONENTS_LAUNCH_PAIRS  a launch of gsim_db_components' tile kernel scores at most this
                                     // many pairs (at least one 256 x 256 tile); 0: the neighbour lists' launch plan (capi_pairs.cpp;
                                     // DESIGN.md section 18).  The result does not depend on it
    long long dbscan_launch_pairs = 0; // GSIM_DBSCAN_LAUNCH_PAIRS  a launch of either of gsim_db_dbscan's tile kernels scores at most this many
                                     // pairs (at least one 256 x 256 tile); 0: the neighbour lists' launch plan (capi_pairs.cpp;
                                     // DESIGN.md section 26).  The result does not depend on it
    long long dbscan_skip = 1;             // GSIM_DBSCAN_SKIP         0: the link pass scores every left row, even one that can matter to no
                                     // lane of the wave (for timing; the result does not depend on it)
    long long mst_launch_pairs = 0;  // GSIM_MST_LAUNCH_PAIRS    a launch of gsim_db_mst's fold kernel scores at most this many owner x candidate
                                     // pairs (at least one column tile of 256 candidates); 0: as knn_launch_pairs (capi_mst.cpp;
                                     // DESIGN.md section 19).  The result does not depend on it
    long long profile_launch_rows = 0; // GSIM_PROFILE_LAUNCH_ROWS  a launch of gsim_db_bit_counts / gsim_db_overlap_sums takes at most this many
                                     // rows (list entries on the gather route); 0: 32 GiB of rows (capi_profile.cpp; DESIGN.md section
                                     // 20).  The result does not depend on it
    long long assign_launch_pairs = 0; // GSIM_ASSIGN_LAUNCH_PAIRS  a launch of gsim_db_assign's kernel scores at most this many centre x row
                                     // pairs (at least one block of 128 table rows against every centre); 0: by the padded row width,
                                     // as scores_launch_pairs (capi_labels.cpp).  The result does not depend on it
    long long labels_launch_rows = 0; // GSIM_LABELS_LAUNCH_ROWS  a launch of gsim_db_label_counts' counting kernel takes at most this many
                                     // entries of the sorted row list; 0: 32 GiB of rows, as profile_launch_rows.  The result does not
                                     // depend on it
};

// One knob that is a number: its variable, its member, the bounds its value is clamped to (kNoLo / kNoHi: none) and how it reads --
// kInt: through atoi, an empty string counts as unset (else: through atoll, an empty string is 0 -- the two hand-written forms this table
// replaces); kBool: any non-zero value is 1; kEmptyIsZero: a kInt knob whose empty string is 0.  Garbage is atoi's / atoll's 0.
struct KnobSpec {
    enum : unsigned { kInt = 1, kBool = 2, kEmptyIsZero = 4 };
    const char* name;
    long long Knobs::*member;
    long long lo, hi;
    unsigned mode;
};
constexpr long long kNoLo = LLONG_MIN, kNoHi = LLONG_MAX;
extern const KnobSpec kKnobSpecs[]; // (the table read_knobs walks; tests/cpp/knobs_check.cpp reads the members through it)
extern const size_t kKnobSpecCount;

Knobs read_knobs(); // the one place that calls getenv for tuning knobs (gsim_db_create)

} // namespace gsim_host
