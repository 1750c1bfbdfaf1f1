// gsim_device.h -- launch interface between the C-ABI host code (capi_*.cpp)
// and the gfx950 kernels (gsim_*.hip).  Internal; not part of the ABI.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <cstddef>
#include <stdint.h>

namespace gsim
{

// In-scan coarse histogram: linear bins over the score range [0, 1].
constexpr int kScanBins = 1024;
// Largest finalist count the single-workgroup LDS select handles.
constexpr int kSelectCap = 8192;
constexpr int kScanBlock = 256; // 4 wavefronts
constexpr int kFusedCheckpoints = 16; // single-launch path: threshold checkpoints (trip counts 1, 4, 16, ... and 3/4 of the trips)

// Device-resident per-query state, zeroed before every scan.
// Device-resident per-query state.  Zero when a query starts: allocated zeroed,
// and the last workgroup of the select kernel re-zeroes it for the next query
// (no per-query memset on the stream).
struct QueryState {
    uint32_t ghist[kScanBins];   // candidates per coarse bin (bins >= each workgroup's final threshold)
    unsigned long long kept;     // rows with score >= cutoff (cutoff > 0 only)
    unsigned long long ncand;    // total candidates emitted by the scan
    uint32_t nfinal;             // finalists appended by the compaction
    uint32_t done;               // select-kernel workgroups that have finished (ticket)
    uint32_t gtau;               // table-wide threshold bin shared by all workgroups of the scan (monotone)
    uint32_t elected;            // single-launch path: highest in-loop checkpoint (1-based) whose threshold election has been held
                                 // ({gtau, elected} are polled with ONE 64-bit load: static_assert below)
    uint32_t redo;               // single-launch path gave up (candidate overflow, heavy ties): the gated
                                 // classic kernels behind it run the query; their select kernel clears it
    uint32_t pad0;
    // --- single-launch path (fused_kernel) ---
    unsigned long long sel_done; // top-level closing ticket: groups of selectors that have written their hits (bits 0..15), those
                                 // that saw the query fail (bits 16..31), the sum of the words of all hits written (bits 32..63)
    // --- not reset per query (the reset boundary is offsetof(redo_why)) ---
    uint32_t redo_why;           // the union of the reasons (kRedo*) of every query handed back so far
    uint32_t pad1;
    unsigned long long ncand_sum; // running totals for gsim_db_get_timing
    unsigned long long nfinal_sum;
    unsigned long long queries;
    unsigned long long redo_sum; // queries the single-launch path handed back to the four-kernel pipeline
};
static_assert(offsetof(QueryState, gtau) % 8 == 0 && offsetof(QueryState, elected) == offsetof(QueryState, gtau) + 4,
              "the single launch's poller reads {gtau, elected} with one 64-bit load");
static_assert(offsetof(QueryState, sel_done) % 8 == 0, "64-bit atomic");

// The single launch's closing word carries a checksum of the result block for synchronous callers: the sum (mod 2^32) of
// the 32-bit words of every hit written, plus epoch * kBlockCheckMul, travels in the upper half of the header's approx
// field (a shard holds < 2^31 rows, so the true upper half is zero) -- the host verifies it against the hits it reads
// before it trusts the block, and clears it (capi_query.cpp finish_query_sync).
constexpr uint32_t kBlockCheckMul = 0x9E3779B1u;

// Why the single-launch path handed a query back (bits of QueryState::redo; the gated kernels only test for non-zero).
constexpr uint32_t kRedoStore = 1;        // a wave met more rows at its threshold than its LDS store holds / a region overflowed
constexpr uint32_t kRedoElectionWait = 2; // small table: a threshold election did not arrive within wait_ticks (shared GPU)
constexpr uint32_t kRedoArrivalWait = 4;  // the grid-wide arrival did not complete within wait_ticks (shared GPU)
constexpr uint32_t kRedoFinalists = 8;    // more rows at or above the final threshold than a selector's LDS holds
constexpr uint32_t kRedoOwned = 16;       // ... or more of them owned by one selector than its list holds
constexpr uint32_t kRedoSeen = 32;        // a selector found the query already failed
constexpr uint32_t kRedoBinTies = 64;     // large k, ranked by coarse bin: one of the top bins holds more rows than kBinRankCap (ties)

struct ScanGeometry {
    uint32_t lanes_per_row; // 16-byte lanes per fingerprint (fp words / 4), 0 = generic path
    uint32_t unroll;        // 16-byte loads in flight per lane
    uint32_t chunk_rows;    // rows per wave iteration
    uint32_t nwaves;        // wavefronts in the grid
    uint32_t seg_cap;       // candidate slots per wavefront
    uint64_t nchunks;
    uint32_t ragged_loads;  // generic widths that are whole 16-byte units per row, not a power of two (896, 1536 ... bits): loads per
                            // chunk of scan_ragged_kernel (the odd part of W / 4: 3, 5 or 7), 0 = the LDS-staged generic scan
    uint32_t ragged_words;  // 1: rows are NOT whole 16-byte units (W = 3, 5, 7, 9, 11 or twice that: 96 ... 704 bits) -- the single launch's
                            // word-granular variant (scan_rows_wragged), ragged_loads = the odd part of W; the four-kernel pipeline
                            // keeps the LDS-staged generic scan for them
};

struct ScanArgs {
    const void* rows;       // device, row-major uint32[nrows][W]
    uint64_t nrows;
    uint32_t W;             // words per fingerprint
    const uint32_t* query;  // W words; device memory or device-visible pinned host memory (read once per wave)
    uint32_t* query_dev;    // device copy for the kernels after the scan (the scan writes it when != query)
    uint32_t qpop;          // popc(query)
    uint32_t k;
    float cutoff;
    int metric;
    float alpha, beta;
    unsigned long long* cand; // device, nwaves*seg_cap keys
    uint32_t* cand_cb;        // device, nwaves*seg_cap (common << 16 | popc_db), parallel to cand
    uint32_t* seg_count;      // device, nwaves
    QueryState* state;        // device
    const uint32_t* gate;     // NULL, or device word: the classic kernels return at once unless *gate != 0
                              // (they are enqueued behind the single-launch path as its fallback)
};

// ---- single-launch path: scan + publish + select in ONE kernel --------------------------------
constexpr uint32_t kFusedMaxK = 8192;       // largest k the single-launch path serves
constexpr uint32_t kFusedPublishMaxK = 262144; // ... and the largest it scans and publishes for (k > kSelectCap: the large-k kernels rank what it published)
// M of the publishing launch's in-loop reports: up to 64 as long as 64 rows per wave cover k (65 536 hits on 1024 waves), up to 256 beyond
// (mth_best keeps four keys per lane -- eight from M = 65 on -- i.e. 256 / 512 per wave: a report is the wave's M-th best of those,
// valid at any M, tight while M is well below that)
constexpr uint32_t fused_publish_max_m(uint32_t k) { return k > 65536u ? 256u : 64u; }
constexpr uint32_t kFusedPublishOnly = 2048u; // FusedArgs::xflags: scan + publish, no selection (launch_fused_handoff follows)
constexpr int kFusedWaveCap = 2048;         // candidate slots per wavefront, in LDS
constexpr int kFusedSelectors = 256;        // workgroups of the grid: every one of them ranks its share of the finalists
constexpr uint32_t kFusedRegion = 4 * kFusedWaveCap; // published entries (16 B each) of one workgroup: its fixed region of the list
constexpr uint32_t kFusedHeaderBytes = 16;  // per workgroup: {entries | sorted << 31, bucket shift | launch tag << 5 | failed << 31, its end-of-scan report (64-bit key)}
constexpr uint32_t kFusedArriveWords = 25;  // arrival (publishing launches of large-k queries only: the last workgroup tidies up): 8 group counters (b % 8), 1 top counter, [8 unused]; closing: 8 group tickets -- 128 B apart

struct FusedArgs {
    void* pub;            // device, nwg regions of kFusedRegion x 16 B {key, cb, launch tag}: what each workgroup publishes
    void* hdr;            // device, nwg headers of kFusedHeaderBytes
    uint32_t* arrive;     // device, kFusedArriveWords words 128 B apart (zero between queries)
    uint32_t* summ;       // device, nwaves score keys: the waves' in-loop checkpoint summaries (zero between queries)
    uint32_t summ_keys;   // M: at the in-loop checkpoints every wave reports its M-th best key (fused_summary_keys), 0 = no checkpoints
    uint32_t final_keys;  // Mw: at the end of the scan every workgroup reports its Mw-th best key (fused_final_keys), 0 = no final threshold
    uint32_t* tickets;    // device, kFusedCheckpoints x 9 counters 128 B apart (8 per-group + 1 top), zero between queries
    void* result;         // result block: device memory or device-visible pinned host memory
    uint32_t row_base;
    uint32_t* done_flag;  // non-NULL: a synchronous caller polls the result header (in pinned host memory): its flags word carries `epoch` << 8
    uint32_t epoch;
    uint32_t pub_tag;     // non-zero, new for every launch on this handle: the fourth word of every entry this launch publishes, its low 26
                          // bits in every header -- readers tell this query's lists from what a region held before (no arrival counter)
    uint32_t wait_ticks;     // bound of the grid-wide wait (100 MHz ticks): a few scan times, see fused_kernel
    uint32_t xflags;         // 4 = QueryState::gtau was seeded by the sample kernel (a coarse bin); experiments (GSIM_FUSED_FLAGS): 2 = no in-loop checkpoints, 1024 = release fence before the closing ticket, 4096 = the published entries get their tags a few microseconds after the header (drives the selectors' read-again path), 8192 = the final threshold always by ranking every report (the path behind a sampled election that found no sample)
    unsigned long long* dbg; // NULL, or 24 timestamps (100 MHz wall clock) per workgroup: phase profile (GSIM_FUSED_DEBUG)
};

// bytes of the three device buffers of the single-launch path for a grid of nwg workgroups
inline size_t fused_pub_bytes(uint32_t nwg) { return static_cast<size_t>(nwg) * kFusedRegion * 16; }
inline size_t fused_hdr_bytes(uint32_t nwg) { return static_cast<size_t>(nwg) * kFusedHeaderBytes; }

hipError_t launch_fused(const ScanArgs& a, const ScanGeometry& g, const FusedArgs& f, hipStream_t s);
// Behind a kFusedPublishOnly launch: the published rows of the coarse bins at or above the k-th best's become the finalists of
// the large-k kernels (their keys into `finalists`, QueryState::nfinal set; ::ghist was filled by the launch) -- unless the
// launch handed the query back (QueryState::redo != 0).
// ... or, for callers that look at the result block (a hand-back can be run again by the host): the same rows placed BY COARSE BIN,
// highest bin first (the histogram gives every bin's first position; `cursors`: kScanBins counters, zero between queries, + kScanBins words that receive the layout), so
// that launch_binrank_emit only has to order each bin's rows among themselves.  A top bin of more than kBinRankCap rows: handed
// back (kRedoBinTies), nothing is placed.
constexpr uint32_t kBinRankCap = 16384; // (a hand-back costs a second scan; a bin of 16 Ki rows ~40 us of compares)
hipError_t launch_fused_binsort(const ScanArgs& a, const FusedArgs& f, uint32_t nwg, unsigned long long* finalists, uint32_t cap, uint32_t* cursors, hipStream_t s);
hipError_t launch_fused_handoff(const ScanArgs& a, const FusedArgs& f, uint32_t nwg, unsigned long long* finalists, uint32_t cap, hipStream_t s);
bool fused_supported(const ScanGeometry& g);
uint32_t fused_summary_keys(uint32_t nwaves, uint32_t k, uint32_t max_m = 16);
uint32_t fused_final_keys(uint32_t nwg, uint32_t k);

// ScanGeometry::lanes_per_row of rows of W words: W / 4 where that is a whole power of two up to 64 (the kernels with a group of
// lanes per row), else 0
inline uint32_t pow2_lanes_per_row(uint32_t W)
{
    const uint32_t l = W / 4;
    return (W % 4 == 0 && l != 0 && (l & (l - 1)) == 0 && l <= 64) ? l : 0;
}
// Geometry of the scan grid for a table (host side, no device work).
ScanGeometry scan_geometry(uint64_t nrows, uint32_t W, int num_cus, int waves_per_cu, int unroll);
// ... of the single launch where it differs from the four-kernel pipeline's: rows of 3, 5, 7, 9, 11 or twice that many WORDS
// (false: it does not -- use scan_geometry's)
bool fused_word_geometry(uint64_t nrows, uint32_t W, int num_cus, ScanGeometry* out);

// Optional K0: starting threshold from a strided sample of chunks_per_wave chunks per scan wave.
hipError_t launch_sample(const ScanArgs& a, const ScanGeometry& g, uint32_t chunks_per_wave, hipStream_t s, bool* launched = nullptr);
hipError_t launch_scan(const ScanArgs& a, const ScanGeometry& g, hipStream_t s);

// Compaction of candidates at or above the k-th best coarse bin into `finalists`.
hipError_t launch_compact(const ScanArgs& a, const ScanGeometry& g, unsigned long long* finalists,
                          uint32_t* finalists_cb, uint32_t finalists_cap, hipStream_t s);

// Final exact select + sort of the finalists (k <= kSelectCap, any finalist count);
// writes {gsim_result_header; gsim_hit[k]}.
hipError_t launch_select(const ScanArgs& a, const unsigned long long* finalists, const uint32_t* finalists_cb,
                         uint32_t finalists_cap, uint32_t row_base, void* d_result, hipStream_t s);
// Large-k path (k > kSelectCap): device state of the radix select (zero between queries).
struct LargeKState {
    unsigned long long prefix; // leading bytes of the k-th largest finalist key found so far
    uint32_t remaining;        // its rank among the finalists that share the prefix
    uint32_t ticket;
    uint32_t count;            // keys gathered
    uint32_t all;              // fewer finalists than k: every finalist is taken
    uint32_t hist[256];
};
hipError_t launch_largek_select(const ScanArgs& a, const unsigned long long* finalists, uint32_t finalists_cap, LargeKState* lk,
                                unsigned long long* out, uint32_t out_cap, uint32_t* hint, bool one_block, hipStream_t s);

// Large-k path (k > kSelectCap): the gathered top-k keys sorted in two launches (tiles in LDS, positions by counting).
// (n_pow2 keys, unique apart from zero padding; `tmp` holds n_pow2 more; *sorted = where the result is: keys or tmp)
hipError_t launch_sort_desc(unsigned long long* keys, unsigned long long* tmp, uint32_t n_pow2, hipStream_t s, unsigned long long** sorted);
// ... the large-k path's last two launches: tiles sorted (slots past LargeKState::count read as padding -- nobody zero-fills
// the buffer), then every key's position by counting AND its hit written there, the header, and -- the last workgroup -- the
// per-query state re-zeroed (until round 4: a fill, the sort, an emission kernel and a reset kernel)
hipError_t launch_largek_sort_emit(const ScanArgs& a, unsigned long long* keys, uint32_t n_pow2, LargeKState* lk, uint32_t row_base,
                                   uint64_t approx_if_no_cutoff, uint32_t flags, void* d_result, hipStream_t s);

// Behind launch_fused_binsort: every finalist's position = its bin's first position + the number of larger keys in its bin; the
// hits of the first k, the header (flag 2 and no hits if QueryState::redo is set: the host runs the query again), the per-query
// state and the cursors re-zeroed by the last workgroup.  Two launches instead of the radix select + gather + two-launch sort.
hipError_t launch_binrank_emit(const ScanArgs& a, const unsigned long long* finalists, uint32_t cap, uint32_t* cursors, LargeKState* lk,
                               uint32_t row_base, uint64_t approx_if_no_cutoff, uint32_t flags, void* d_result, hipStream_t s);

// Folded tables: re-score the candidates of a folded search (result block `folded_block`, device memory) with the full
// fingerprints, stable sort by the new score, first min(k, .) at or above the cutoff -> out_block (fingerprintdb_cuda.cu:
// 307-331).  npad = candidates rounded up to a power of two (<= 65536): size of keys / cbs.  *nan_flag is set when a
// score is NaN (the caller then takes the host path).
hipError_t launch_fold_rescore(const void* folded_block, const uint32_t* full_rows, const uint32_t* full_query, uint32_t W, uint32_t qpop,
                               unsigned long long* keys, uint32_t* cbs, uint32_t npad, uint32_t* nan_flag, uint32_t k, float cutoff,
                               uint32_t row_base, void* out_block, hipStream_t s);

// Merge of result blocks (multi-GPU gather) for nq queries: the lists of query q are the blocks
// q, q + nq, ... (nblocks of them); merged block q goes to d_results + q * block_bytes.
hipError_t launch_merge_batch(const void* d_blocks, uint32_t nblocks, uint32_t nq, size_t block_bytes, uint32_t k,
                              void* d_results, hipStream_t s);

// ---- multi-query batches (gsim_batch.hip) ------------------------------------------
constexpr int kBQ = 32;     // queries per pass over the table
constexpr int kBBins = 512; // linear coarse bins of the batch filter

struct BatchQueryState { // one per query of a batch, device memory, zeroed before the batch
    uint32_t ghist[kBBins];
    uint32_t gtau;
    uint32_t nfinal;
    uint32_t bstar;
    uint32_t pad;             // matrix-core pass: candidates emitted so far (threshold update trigger)
    unsigned long long kept;
};

// Rarely used arguments (emission / compaction paths) live in device memory so that the
// scan's inner loop has scalar registers left for double-buffered query loads.
struct BatchRare {
    BatchQueryState* qstate; // device, Q
    unsigned long long* cand; // per-wave segments, seg_cap entries each
    uint32_t* cand_cb;
    uint32_t* cand_q;
    uint32_t* seg_count;      // nwaves
    unsigned long long* fin_key; // Q x kSelectCap
    uint32_t* fin_cb;
    uint32_t* flags;          // bit 0: a candidate segment overflowed
    uint32_t* ticket;
    uint32_t seg_cap;
    uint32_t pad;
};

struct BatchArgs {
    const void* rows;
    uint64_t nrows;
    const uint32_t* queries; // device, Q x W words
    const uint32_t* qpop;    // device, Q
    const BatchRare* rare;   // device copy of the rare arguments
    const uint16_t* rowpop;  // matrix-core pass: popc(row) per row (launch_row_popcounts), padded to whole 16-byte chunks
    uint32_t W;
    uint32_t q0, nq;         // this pass: queries q0 .. q0+nq-1 (nq <= kBQ, matrix-core pass: kMfmaQueries)
    uint32_t k;
    float cutoff;
    int metric;
    float alpha, beta;
    uint32_t opts;           // host side only -- bit 1: dense-cutoff variant allowed (GSIM_BATCH_MFMA_DENSE); the other bits are not in use
};

bool batch_supported(uint32_t W);
hipError_t launch_batch_pass(const BatchArgs& a, const BatchRare& rare_host, const ScanGeometry& g,
                             uint32_t sample_chunks, uint32_t row_base, void* results, size_t block_bytes,
                             hipStream_t s);

// Matrix-core variant of the scan (gsim_batch_mfma.hip): up to kMfmaQueries queries per table pass.
constexpr int kMfmaQueries = 256;
bool batch_mfma_supported(uint32_t W);
// the side array of row popcounts the matrix-core pass reads: nrows 16-bit counts (allocate row_popcount_bytes(nrows))
hipError_t launch_row_popcounts(const void* rows, uint64_t nrows, uint32_t W, uint16_t* d_out, hipStream_t s);
inline size_t row_popcount_bytes(uint64_t nrows) { return static_cast<size_t>((nrows + 7) / 8 + 1) * 16; }
uint32_t batch_mfma_waves(int num_cus);
hipError_t launch_batch_mfma_scan(const BatchArgs& a, int num_cus, hipStream_t s);
bool batch_mfma_dense_applies(int metric, float alpha, float beta, float cutoff, bool enabled);
bool launch_batch_mfma_sample(const BatchArgs& a, int num_cus, hipStream_t s, hipError_t* err);
bool batch_mfma_sample_applies(uint32_t W, uint64_t nrows, uint32_t nq, uint32_t k, int num_cus);
hipError_t launch_batch_mfma_pass(const BatchArgs& a, const ScanGeometry& g, int num_cus, uint32_t sample_chunks,
                                  uint32_t row_base, void* results, size_t block_bytes, hipStream_t s,
                                  hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// debug hooks for the pre-filter of the matrix-core pass (gsim_prefilter.h): device and host twins
hipError_t launch_prefilter_table(int tversky, float alpha, float beta, uint32_t max_qa, int has_cutoff, float cutoff,
                                  float* d_out, hipStream_t s);
void prefilter_table_host(int tversky, float alpha, float beta, uint32_t max_qa, int has_cutoff, float cutoff, float* out);

// ---- all-pairs neighbour lists (gsim_neighbors.hip, gsim_db_neighbors) --------------------------------------------------
constexpr int kNbrTile = 256;      // left rows x right rows of one workgroup's tile
constexpr int kNbrBlock = 256;     // 4 waves, 64 right rows each
constexpr uint32_t kNbrMaxWords = 128; // 4096-bit rows
struct NbrArgs {
    const uint32_t* rows;        // nrows x WP words, 16-byte aligned (the table itself when W == WP, else a zero-padded copy)
    const uint32_t* pop;         // popc of every row
    uint64_t nrows;
    uint64_t row_begin, row_end; // left rows
    uint32_t WP;                 // words per row as the kernel reads them (4, 8, ... 128)
    int tri;                     // 1: full-table call, upper triangle, every pair appended under both rows
    int metric;
    float alpha, beta, cutoff;
    unsigned long long* keys;    // ((left row - row_begin) << 32) | right row
    float* vals;                 // score
    unsigned long long* cursor;  // entries appended so far (keeps counting past cap)
    uint64_t cap;                // entries keys / vals hold
    unsigned long long* clk;     // this launch's {s_memtime, wall clock} at the start and end of one tile (nullptr: none)
};
// The join instantiations of the same kernel (gsim_db_join*): the left operand is not the table -- nl x WP words (16-byte
// aligned) and their popc; row_begin = 0 and row_end = nl index THESE rows, tri is ignored, and no pair is excluded
struct JoinTileArgs : NbrArgs {
    const uint32_t* lrows;
    const uint32_t* lpop;
};
uint32_t nbr_padded_words(uint32_t W); // 0: wider than kNbrMaxWords
hipError_t launch_nbr_prepare(const void* rows, uint64_t nrows, uint32_t W, uint32_t WP, uint32_t* pad, uint32_t* pop, hipStream_t s);
// tiles (rt0 .. rt0+nrt-1) x (ct0 .. ct0+nct-1), tile row rt = left rows row_begin + rt * kNbrTile ..
hipError_t launch_nbr_tiles(const NbrArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s);
hipError_t launch_join_tiles(const JoinTileArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s);
hipError_t launch_nbr_snap(const unsigned long long* cursor, unsigned long long* snap, hipStream_t s);
hipError_t nbr_sort_bytes(uint64_t n, uint32_t end_bit, size_t* bytes);
hipError_t launch_nbr_csr(void* tmp, size_t tmp_bytes, const unsigned long long* keys, const float* vals, unsigned long long* keys_sorted,
                          float* vals_sorted, uint64_t n, uint32_t end_bit, uint64_t nrows_out, uint32_t row_base, uint64_t* indptr,
                          uint32_t* indices, hipStream_t s);

// ---- primitives (gsim_prims.hip) ------------------------------------------------------------------------------------------
// out[0 .. n) = the exclusive prefix sums of in[0 .. n), 32-bit words (tmp: scan_u32_bytes(n) bytes)
hipError_t scan_u32_bytes(uint64_t n, size_t* bytes);
hipError_t launch_scan_u32(void* tmp, size_t tmp_bytes, const uint32_t* in, uint32_t* out, uint64_t n, hipStream_t s);

// ---- single-linkage clustering: connected components of the threshold graph (gsim_components.hip, gsim_db_components) -----
constexpr uint32_t kCompMaxLevels = 8; // GSIM_COMPONENTS_MAX_LEVELS
constexpr uint32_t kCompKept = 0, kCompUnions = 1, kCompCasFailed = 2, kCompCounters = 3; // CompArgs::counters
struct CompArgs {
    const uint32_t* rows;        // nrows x WP words, 16-byte aligned (the table itself when W == WP, else a zero-padded copy)
    const uint32_t* pop;         // popc of every row
    uint64_t nrows;
    uint32_t WP;                 // words per row as the kernel reads them (4, 8, ... 128)
    uint32_t nlevels;            // 1 ... kCompMaxLevels
    int metric;
    float alpha, beta;
    float cutoffs[kCompMaxLevels]; // ascending; [0 .. nlevels)
    uint32_t* parent;            // nlevels forests of nrows words (the protocol: gsim_components.hip)
    unsigned long long* counters; // kCompCounters words, added to
    unsigned long long* clk;     // as NbrArgs::clk
};
hipError_t launch_comp_init(uint32_t* parent, uint64_t nrows, uint32_t nlevels, hipStream_t s);
// tiles (rt0 .. rt0+nrt-1) x (ct0 .. ct0+nct-1) of the upper triangle, as launch_nbr_tiles with tri = 1
hipError_t launch_comp_tiles(const CompArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s);
hipError_t launch_comp_flatten(uint32_t* parent, uint64_t nrows, uint32_t nlevels, hipStream_t s);
// one flattened forest -> component_of[nrows], *ncomponents, first_row / sizes (or nullptr; sizes zeroed before) -- flag, num: nrows
// words of scratch each, tmp: scan_u32_bytes(nrows)
hipError_t launch_comp_label(void* tmp, size_t tmp_bytes, const uint32_t* parent, uint64_t nrows, uint32_t row_base, uint32_t* flag,
                             uint32_t* num, uint32_t* component_of, uint32_t* first_row, uint32_t* sizes, uint32_t* ncomponents,
                             hipStream_t s);

// ---- DBSCAN density clustering (gsim_dbscan.hip, gsim_db_dbscan) -----------------------------------------------------------
constexpr uint32_t kDbscanKept = 0, kDbscanUnions = 1, kDbscanCasFailed = 2, kDbscanCores = 3, kDbscanBorders = 4, kDbscanNoise = 5,
                   kDbscanDegreeSum = 6, kDbscanCounters = 7; // DbscanArgs::counters
struct DbscanArgs {
    const uint32_t* rows;        // nrows x WP words, 16-byte aligned (the table itself when W == WP, else a zero-padded copy)
    const uint32_t* pop;         // popc of every row
    uint64_t nrows;
    uint32_t WP;                 // words per row as the kernels read them (4, 8, ... 128)
    int metric;
    float alpha, beta;
    float cutoff;
    uint32_t min_pts;            // >= 1; row x is a core iff degree[x] + 1 >= min_pts
    uint32_t skip;               // link pass: 1 = a wave passes over a non-core left row when it holds no core (GSIM_DBSCAN_SKIP)
    uint32_t* degree;            // nrows words, zeroed before the degree pass, which adds to them; the link pass reads them
    uint32_t* parent;            // one forest of nrows words over ALL rows (the protocol: gsim_components.hip); only cores are united
    unsigned long long* best;    // nrows words, zeroed before the link pass: key(score, ~core row) of a non-core row's anchor, 0: none
    unsigned long long* counters; // kDbscanCounters words, added to
    unsigned long long* clk;     // as NbrArgs::clk
};
// tiles (rt0 .. rt0+nrt-1) x (ct0 .. ct0+nct-1) of the upper triangle, as launch_comp_tiles: the degree pass, and the link pass (each
// launch of which launch_comp_flatten follows)
hipError_t launch_dbscan_count(const DbscanArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s);
hipError_t launch_dbscan_link(const DbscanArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s);
// the flattened forest, the degrees and best[] -> label_of[nrows], *nclusters, the census in a.counters, anchor / first_row / sizes (or
// nullptr; sizes zeroed before) -- flag, num: nrows words of scratch each, tmp: scan_u32_bytes(nrows)
hipError_t launch_dbscan_label(void* tmp, size_t tmp_bytes, const DbscanArgs& a, uint32_t row_base, uint32_t* flag, uint32_t* num,
                               uint32_t* label_of, uint32_t* anchor, uint32_t* first_row, uint32_t* sizes, uint32_t* nclusters, hipStream_t s);

// ---- exact k-nearest-neighbour lists of the table's own rows (gsim_knn.hip, gsim_db_knn) ----------------------------------
constexpr int kKnnTile = 256;   // owner rows of one workgroup
constexpr int kKnnBlock = 256;  // 4 waves, 64 owners each, all walking the same candidates
constexpr uint32_t kKnnColTile = 256; // launches are cut at multiples of this many candidate rows
struct KnnEntry {
    float score;
    uint32_t row; // table row, without the row base
};
struct KnnArgs {
    const uint32_t* rows;        // nrows x WP words, 16-byte aligned (the table itself when W == WP, else a zero-padded copy)
    const uint32_t* pop;         // popc of every row
    uint64_t nrows;
    uint64_t row_begin, row_end; // the owners: list o belongs to table row row_begin + o
    uint32_t WP;                 // words per row as the kernel reads them (4, 8, ... 128)
    uint32_t k;                  // 1 ... GSIM_KNN_MAX_K
    int metric;
    float alpha, beta, cutoff;
    KnnEntry* lists;             // (row_end - row_begin) x k entries, each list in (score descending, row ascending) order
    uint32_t* len;               // entries held per list (zero before the first launch)
    unsigned long long* inserts; // list insertions made so far
    unsigned long long* clk;     // this launch's {s_memtime, wall clock} at the start and end of its first workgroup (nullptr: none)
};
// Owner tiles ot0 .. ot0 + not_ - 1 (tile t = owners t * kKnnTile ..) fold the candidate rows [c0, c1) into their lists.  The
// pieces of the same owners must be launched in ascending column order on one stream.
hipError_t launch_knn_fold(const KnnArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, hipStream_t s);
// indptr[0 .. n) = exclusive prefix sums of len[0 .. n) (n = lists + 1 with len[lists] = 0: indptr[lists] is the total)
hipError_t knn_scan_bytes(uint64_t n, size_t* bytes);
hipError_t launch_knn_offsets(void* tmp, size_t tmp_bytes, const uint32_t* len, uint64_t n, uint64_t* indptr, hipStream_t s);
// every held entry to its place: indices (+ row_base) and scores
hipError_t launch_knn_compact(const KnnEntry* lists, const uint32_t* len, const uint64_t* indptr, uint64_t nown, uint32_t k, uint32_t row_base,
                              uint32_t* indices, float* scores, hipStream_t s);

// ---- exact k-nearest-neighbour joins: the k nearest TABLE rows of another table's rows (gsim_knn_join.hip, gsim_db_knn_join*) ----
// knn_fold_kernel's scheme with the owners read from a second array and the table's columns cut into nseg segments, each folded
// by workgroups of its own into a partial list per (owner, segment); a merge kernel then ranks the partial lists' entries.
constexpr uint32_t kKnnJoinMaxSegments = 65535; // (a launch's second grid dimension)
// Segment s of nseg over N table rows: whole column tiles [first_tile(s), first_tile(s + 1)), clipped to N.  Segment 0 is never
// shorter than another.
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint64_t knn_join_seg_begin(uint64_t s, uint64_t nseg, uint64_t N)
{
    const uint64_t nct = (N + kKnnColTile - 1) / kKnnColTile;
    const uint64_t r = (s * nct + nseg - 1) / nseg * kKnnColTile;
    return r < N ? r : N;
}
struct KnnJoinArgs {
    const uint32_t* rows;        // the table: nrows x WP words, 16-byte aligned (itself when W == WP, else a zero-padded copy)
    const uint32_t* pop;         // popc of every table row
    uint64_t nrows;
    const uint32_t* lrows;       // the owners: nl x WP words, 16-byte aligned
    uint64_t nl;
    uint64_t self0;              // GSIM_KNN_EXCLUDE_SELF: owner o is table row self0 + o and that pair is left out; ~0: no pair is
    uint32_t WP;                 // words per row as the kernel reads them (4, 8, ... 128)
    uint32_t k;                  // 1 ... GSIM_KNN_MAX_K
    uint32_t nseg;               // 1 ... kKnnJoinMaxSegments, at most the table's column tiles
    int metric;
    float alpha, beta, cutoff;
    KnnEntry* lists;             // nl x nseg x k entries: list (o, s) at (o * nseg + s) * k, in (score descending, row ascending) order
    uint32_t* len;               // entries held per list (zero before the first launch)
    unsigned long long* inserts; // list insertions made so far
    unsigned long long* clk;     // as KnnArgs.clk
};
// Owner tiles ot0 .. ot0 + not_ - 1 fold, for every segment, the segment's rows [r0, r1) (counted from the segment's first row)
// into the partial lists.  The pieces of the same owners must be launched in ascending order of r0 on one stream.
hipError_t launch_knn_join_fold(const KnnJoinArgs& a, uint32_t ot0, uint32_t not_, uint64_t r0, uint64_t r1, hipStream_t s);
// The nseg partial lists of every owner -> its first k of all of them in out (nl x k) and their number in out_len (nl); *held
// grows by the number of entries the partial lists hold
hipError_t launch_knn_join_merge(const KnnEntry* lists, const uint32_t* len, uint64_t nl, uint32_t nseg, uint32_t k, KnnEntry* out,
                                 uint32_t* out_len, unsigned long long* held, hipStream_t s);

// ---- exact single-linkage dendrograms: the maximum-similarity spanning forest (gsim_mst.hip, gsim_db_mst) -------------------
// Boruvka rounds.  The fold kernel is knn_fold_kernel's scheme (kKnnTile owners to a workgroup, kKnnBlock threads) with the list
// replaced by one 64-bit word per row; the owners of a round come through an index list.
constexpr unsigned long long kMstNone = 0ull; // best[i]: (score bits << 32) | ~partner -- larger is earlier in order E; 0: none held
constexpr uint32_t kMstCtlEdges = 0, kMstCtlOwners = 1, kMstCtlRoots = 2, kMstCtlWords = 3; // MstState::ctl
struct MstArgs {
    const uint32_t* rows;        // nrows x WP words, 16-byte aligned (the table itself when W == WP, else a zero-padded copy)
    const uint32_t* pop;         // popc of every row
    const uint32_t* comp;        // component id of every row (a row of the component)
    const uint32_t* own;         // the round's owners: nown table rows, ascending
    uint64_t nrows;
    uint32_t nown;
    uint32_t WP;                 // words per row as the kernel reads them (4, 8, ... 128)
    int metric;
    float alpha, beta, cutoff;
    unsigned long long* best;    // nrows words, kMstNone for every owner before the round's first launch
    unsigned long long* clk;     // as KnnArgs.clk
};
// Owner tiles ot0 .. ot0 + not_ - 1 of the list (tile t = owners t * kKnnTile ..) fold the candidate rows [c0, c1), cut into
// nchunk pieces that run side by side, into best[].  Launch order and the cut play no part in the result.
hipError_t launch_mst_fold(const MstArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t nchunk, hipStream_t s);
struct MstState {
    uint64_t nrows;
    uint32_t* comp;              // nrows
    uint32_t* parent;            // nrows, indexed by component id
    uint32_t* own;               // nrows: the next round's owner list
    uint32_t* flag;              // nrows
    uint32_t* cscore;            // nrows, per component id: the best held score's bits
    unsigned long long* best;    // nrows
    unsigned long long* ckey;    // nrows, per component id: (a << 32) | b of its E-first edge
    unsigned long long* ekey;    // cap: (~score bits << 32) | a of every edge taken so far
    uint32_t* eb;                // cap: its b
    uint64_t cap;                // nrows - 1
    unsigned long long* ctl;     // kMstCtlWords: edges taken so far, owners of the next round, roots (mst_count_roots)
};
hipError_t launch_mst_init(const MstState& m, hipStream_t s); // comp = parent = own = identity, best = none, ctl = 0
hipError_t mst_select_bytes(uint64_t nrows, size_t* bytes);
// One round's bookkeeping after its fold launches: every component's E-first held edge, the edges appended (each once), the
// components merged and flattened, and the next round's owner list (ctl[kMstCtlOwners] rows of own[], their best[] reset).
hipError_t launch_mst_round(const MstState& m, void* tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_mst_count_roots(const MstState& m, hipStream_t s);
hipError_t mst_sort_bytes(uint64_t n, size_t* bytes);
// the n edges taken, in order E, as gsim_mst_edge (12 bytes: a + row_base, b + row_base, score); ekey2 / eb2: n words of scratch
hipError_t launch_mst_sort(const MstState& m, uint64_t n, void* tmp, size_t tmp_bytes, unsigned long long* ekey2, uint32_t* eb2,
                           uint32_t row_base, void* edges, hipStream_t s);

// ---- mutual-reachability forests (gsim_mreach.hip, gsim_db_core_scores / gsim_db_mreach_mst / gsim_db_hdbscan) ---------------
// gsim_db_mst's rounds with m(i, j) = min(score(i, j), core[i], core[j]) in place of the score: only the fold kernel differs.
struct MreachArgs {
    MstArgs mst;
    const float* core;           // nrows core scores: 0.0f, or a value >= cutoff
};
// as launch_mst_fold
hipError_t launch_mreach_fold(const MreachArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t nchunk, hipStream_t s);
// core[i] = list i's last entry's score where the list is full (len[i] == k), else 0.0f; with k == 0 (min_pts 1: no lists) 1.0f.
// *dense grows by the number of rows with core[i] >= cutoff.
hipError_t launch_mreach_core(const KnnEntry* lists, const uint32_t* len, uint64_t nrows, uint32_t k, float cutoff, float* core,
                              unsigned long long* dense, hipStream_t s);

// ---- shared-nearest-neighbour counts and Jarvis-Patrick links (gsim_snn.hip, gsim_db_snn / gsim_db_jarvis_patrick) -----------------
constexpr uint32_t kSnnEntries = 0, kSnnMutual = 1, kSnnUnions = 2, kSnnCasFailed = 3, kSnnLinks = 4; // SnnArgs::counters; kSnnLinks + level
constexpr uint32_t kSnnCounters = kSnnLinks + kCompMaxLevels;
struct SnnArgs {
    const KnnEntry* lists;       // nrows x k slots as the fold left them (KnnArgs::lists, all rows as owners)
    const uint32_t* len;         // entries held per list
    const uint32_t* nbr;         // nrows x k: every list's rows ascending, padded with 0xFFFFFFFF (launch_snn_sort)
    uint64_t nrows;
    uint32_t k;                  // 1 ... GSIM_KNN_MAX_K
    uint32_t flags;              // GSIM_SNN_CLOSED | GSIM_SNN_EITHER
    uint32_t nlevels;            // 1 ... kCompMaxLevels (with parent)
    uint32_t kmins[kCompMaxLevels]; // ascending; [0 .. nlevels)
    uint32_t* parent;            // nlevels forests of nrows words (gsim_components.hip's protocol), or nullptr: no links
    uint32_t* shared;            // nrows x k: the count | GSIM_SNN_MUTUAL_BIT of every held entry, or nullptr
    unsigned long long* counters; // kSnnCounters words, added to
};
hipError_t launch_snn_sort(const KnnEntry* lists, const uint32_t* len, uint64_t nrows, uint32_t k, uint32_t* nbr, hipStream_t s);
// every entry of every list: its count, and its links into the forests (launch_comp_flatten follows)
hipError_t launch_snn_link(const SnnArgs& a, int num_cus, hipStream_t s);
// the counts of the held entries to their CSR places, as launch_knn_compact moves indices and scores
hipError_t launch_snn_compact(const uint32_t* shared, const uint32_t* len, const uint64_t* indptr, uint64_t nrows, uint32_t k, uint32_t* out,
                              hipStream_t s);

// ---- per-bit column counts and weighted popcounts (gsim_profile.hip, gsim_db_bit_counts / gsim_db_overlap_sums) -------------
constexpr int kProfileBlock = 256;
constexpr uint32_t kProfileMaxIters = 4088; // rows one thread can add into its 12 vertical counter planes: a multiple of 8 below 2^12
constexpr uint32_t kProfileSliceIters = 1024; // ... and the most a slice gives it
struct ProfileCountArgs {
    const uint32_t* rows;        // the whole table, nrows x W words (16-byte aligned rows when W % 4 == 0)
    uint32_t W;
    const uint32_t* bits;        // a row set's bitmap: the launch streams its rows and counts those the bitmap selects; or nullptr
    const uint32_t* list;        // a row set's ascending list: the launch gathers entries of it; or nullptr (never both)
    unsigned long long* counts;  // W x 32 counters + one more: the rows counted
    uint32_t* partial;           // scratch of a launch: profile_count_blocks(num_cus) x (W x 32 + 1) words
};
uint32_t profile_count_blocks(int num_cus); // the most workgroups a launch has
// One launch (the counting kernel and the reduce kernel behind it): adds the rows [i0, i1) -- with `list`, the rows
// list[i0 .. i1) -- into counts.  Any cut of a range into launches gives the same counters (integer adds).  Launches that share
// counts and partial go on one stream.
hipError_t launch_profile_count(const ProfileCountArgs& a, uint64_t i0, uint64_t i1, int num_cus, hipStream_t s);
// range[0], range[1] = the first entries of the ascending list[0 .. n) that are >= r0, >= r1
hipError_t launch_profile_list_range(const uint32_t* list, uint32_t n, uint64_t r0, uint64_t r1, uint32_t* range, hipStream_t s);
struct ProfileOverlapArgs {
    const uint32_t* rows;        // as ProfileCountArgs
    uint32_t W;
    const uint32_t* planes;      // 32 x W words: plane b = the fingerprint of the columns whose weight has bit b set (zero from nplanes on)
    uint32_t nplanes;            // planes the largest weight needs (1 ... 32)
    unsigned long long* sums;    // sums[row - out0]
    uint32_t* popc;              // popc[row - out0], or nullptr
    uint64_t out0;
};
bool profile_overlap_matrix(uint32_t W); // does the matrix-core kernel take rows of W words (whole 256-bit groups)?
// One launch over the rows [r0, r1): on the matrix cores (`matrix`, only where profile_overlap_matrix(W)) or the VALU kernel (any W <= 128)
hipError_t launch_profile_overlap(const ProfileOverlapArgs& a, uint64_t r0, uint64_t r1, bool matrix, int num_cus, hipStream_t s);

// ---- similarity histograms (gsim_hist.hip, gsim_db_histogram / gsim_db_histogram_queries) ----------------------------------
constexpr int kHistTile = 256;           // owner (left) rows of one workgroup of the owner-tile kernel
constexpr int kHistBlock = 256;          // 4 waves, 64 owners each, all walking the same candidates
constexpr uint32_t kHistColTile = 256;   // column chunks and launch cuts are multiples of this many table rows
constexpr uint32_t kHistMaxChunk = 65280; // table rows one workgroup counts before it flushes: < 2^16, two counters share an LDS word
constexpr uint32_t kHistCoarse = 256;    // cells of the coarse bin table: cell t holds bin(t / 256), the bin search starts there
struct HistBins {
    const float* edges;          // nedges floats, strictly ascending, edges[0] > 0
    const uint8_t* coarse;       // kHistCoarse bytes: coarse[t] = number of edges <= t / kHistCoarse
    uint32_t nedges;             // 1 ... GSIM_HIST_MAX_EDGES
    float cut_lo;                // valu_cutoff_lo(edges[0]) when edges[0] <= 1, else 0: a pair with c < cut_lo x den is in bin 0
};
// words per owner of the tile kernel's LDS counters (16 bits each, two to a word; odd, so that the 64 lanes' rows start on
// different banks) and the dynamic LDS of a workgroup
uint32_t hist_tile_stride(uint32_t nedges);
size_t hist_tile_lds_bytes(uint32_t nedges);
struct HistTileArgs {
    const uint32_t* rows;        // the table: nrows x WP words, 16-byte aligned (zero-padded copy unless W == WP)
    const uint32_t* pop;         // popc of every table row
    const uint32_t* lrows;       // the left rows: nl x WP words, 16-byte aligned
    uint64_t nrows, nl;
    uint32_t WP;
    int metric;
    float alpha, beta;
    uint64_t self0;              // GSIM_HIST_EXCLUDE_SELF: left row o is table row self0 + o, that pair is skipped; ~0: nothing is
    HistBins bins;
    unsigned long long* hist;    // nl x (nedges + 1) counters
    unsigned long long* clk;     // as KnnArgs.clk
};
// Owner tiles ot0 .. ot0 + not_ - 1 against the table rows [c0, c1), `chunk` (a multiple of kHistColTile, <= kHistMaxChunk) to a
// workgroup: grid = owner tiles x column chunks, every workgroup adds its counts into hist with atomics.
hipError_t launch_hist_tiles(const HistTileArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t chunk, hipStream_t s);
struct HistStreamArgs {
    const void* rows;            // the whole table, nrows x W words
    uint32_t W;
    int metric;
    float alpha, beta;
    const uint32_t* left;        // the left rows, W words each
    uint64_t self0;              // as HistTileArgs.self0
    HistBins bins;
    unsigned long long* hist;
    int naive;                   // hist_naive_add
};
// One launch of left row l's pass: table rows [r0, r0 + nrows), g = maxmin_geometry(nrows, ...), r0 a multiple of 64.
hipError_t launch_hist_pass(const HistStreamArgs& h, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t l, hipStream_t s);
// total[b] = sum over the nl rows of hist[i][b] (total is zeroed by the launch)
hipError_t launch_hist_total(const unsigned long long* hist, uint64_t nl, uint32_t nbins, unsigned long long* total, hipStream_t s);

// ---- dense similarity matrices (gsim_scores.hip, gsim_db_scores / gsim_db_scores_queries / gsim_db_scores_device) ----------
constexpr int kScoresTile = 128;  // left rows x table rows of one workgroup's block of the output
constexpr int kScoresBlock = 256; // 4 waves, a 64 x 64 quarter of the block each
struct ScoresArgs {
    const uint32_t* lrows;       // the call's left rows: nl x WP words, 16-byte aligned (zero-padded copy unless W == WP)
    const uint32_t* rrows;       // the call's table rows: nr x WP words, likewise
    const uint32_t* lpop;        // popc of every left row
    const uint32_t* rpop;        // popc of every table row
    uint64_t nl, nr;
    uint32_t WP;                 // words per row as the kernel reads them: a multiple of 8 (256 bits), at most kNbrMaxWords
    int metric;
    float alpha, beta;
    float* out;                  // out[i * ld + j] = score(left row i, table row j), device memory; only j < nr is written
    uint64_t ld;
    unsigned long long* clk;     // as KnnArgs.clk
};
uint32_t scores_padded_words(uint32_t W); // 0: wider than kNbrMaxWords
// The block of left rows [l0, l1) x table rows [r0, r1) of the call's rectangle: l0 and r0 multiples of kScoresTile, l1 and r1
// too unless they are nl / nr; at most 65 535 x kScoresTile left rows to a launch.
hipError_t launch_scores(const ScoresArgs& a, uint64_t l0, uint64_t l1, uint64_t r0, uint64_t r1, hipStream_t s);

// ---- nearest-centre assignment (gsim_assign.hip, gsim_db_assign / gsim_db_kmeans) ------------------------------------------
struct AssignArgs {
    const uint32_t* centres;     // m x WP words, 16-byte aligned (zero-padded copy unless W == WP)
    const uint32_t* rows;        // the slab's table rows: nr x WP words, likewise
    const uint32_t* cpop;        // popc of every centre
    const uint32_t* rpop;        // popc of every row of the slab
    uint32_t m;                  // 1 ... GSIM_ASSIGN_MAX_CENTRES
    uint64_t nr;
    uint32_t WP;                 // as ScoresArgs.WP
    int metric;
    float alpha, beta;           // the centre is the left side: alpha weighs its bits
    uint32_t* label;             // label[j], j < nr: the centre of the greatest f32 score, the lowest index among equals
    float* score;                // that score (never nullptr)
    unsigned long long* clk;     // as KnnArgs.clk
};
// The rows [r0, r1) of the slab, every centre: r0 a multiple of kScoresTile, r1 too unless it is nr.  One workgroup per block of
// kScoresTile rows; it loops over the centres itself.
hipError_t launch_assign(const AssignArgs& a, uint64_t r0, uint64_t r1, hipStream_t s);

// ---- column counts of every label (gsim_labels.hip, gsim_db_label_counts / gsim_db_kmeans) ---------------------------------
constexpr int kLabelsBlock = 256;
constexpr uint32_t kLabelsSlice = 4096; // entries of the sorted list one workgroup walks before it takes the next slice
// keys[i] = min(labels[i], nlabels) (GSIM_LABEL_NONE sorts behind every label), vals[i] = row0 + i
hipError_t launch_labels_keys(const uint32_t* labels, uint64_t n, uint32_t nlabels, uint32_t row0, uint32_t* keys, uint32_t* vals, hipStream_t s);
hipError_t labels_sort_bytes(uint64_t n, uint32_t nlabels, size_t* bytes);
// (keys, vals) -> (keys_sorted, vals_sorted), stable: the rows of a label ascend
hipError_t launch_labels_sort(void* tmp, size_t tmp_bytes, const uint32_t* keys, uint32_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted,
                              uint64_t n, uint32_t nlabels, hipStream_t s);
// first[l], l <= nlabels: the first entry of the sorted keys that is >= l (first[nlabels]: the rows counted)
hipError_t launch_labels_bounds(const uint32_t* keys_sorted, uint64_t n, uint32_t nlabels, uint32_t* first, hipStream_t s);
struct LabelCountArgs {
    const uint32_t* rows;        // the whole table, nrows x W words
    uint32_t W;
    const uint32_t* keys;        // the sorted labels
    const uint32_t* list;        // ... and their rows
    uint32_t* counts;            // nlabels x (W x 32) counters
    uint32_t nlabels;
};
// Adds the rows list[i0 .. i1) into their labels' counters.  Any cut of the list into launches gives the same counters.
hipError_t launch_labels_count(const LabelCountArgs& a, uint64_t i0, uint64_t i1, int num_cus, hipStream_t s);
// *changed (zeroed by the caller) += the number of i < n with a[i] != b[i]
hipError_t launch_labels_changed(const uint32_t* a, const uint32_t* b, uint64_t n, unsigned long long* changed, hipStream_t s);

// ---- quantised score sums by label (gsim_label_sums.hip, gsim_db_label_sums) -------------------------------------------------
constexpr int kLsumTile = 256;          // owner rows of one workgroup
constexpr int kLsumBlock = 256;         // 4 waves, 64 owners each
constexpr uint32_t kLsumColTile = 256;  // launches are cut at multiples of this many candidates
// What an owner carries from launch to launch (32 bytes)
struct LsumState {
    unsigned long long run_q;    // the sum over the part seen so far of the segment that the last launch ended in (0: it ended at a segment's end)
    unsigned long long own_q;    // Q[i, labels[i]]
    unsigned long long best_q;   // Q[i, best_label]
    uint32_t best_label;         // GSIM_LABEL_NONE: no other segment folded yet
    uint32_t pad;
};
struct LsumArgs {
    const uint32_t* rows;        // the labelled rows in sorted order: n x WP words, 16-byte aligned, zero-padded
    const uint32_t* pop;         // popc of every one
    const uint32_t* keys;        // the label of every sorted position (ascending)
    const uint32_t* first;       // nlabels + 1 segment starts: label l is [first[l], first[l + 1])
    uint64_t n;                  // labelled rows: owners and candidates are the sorted positions [0, n)
    uint32_t WP;                 // words per row as the kernel reads them (4, 8, ... 128)
    int metric;
    float alpha, beta;           // the owner is the query side: alpha weighs its bits
    LsumState* state;            // n entries; before the first launch {0, 0, 0, GSIM_LABEL_NONE}
    unsigned long long* clk;     // as KnnArgs.clk
};
// out (n x WP words) = the table rows list[0 .. n) of W words each, zero-padded
hipError_t launch_lsum_gather(const uint32_t* rows, uint32_t W, uint32_t WP, const uint32_t* list, uint64_t n, uint32_t* out, hipStream_t s);
hipError_t launch_lsum_init(LsumState* state, uint64_t n, hipStream_t s);
// Owner tiles ot0 .. ot0 + not_ - 1 (tile t = sorted positions t * kLsumTile ..) fold the candidates [c0, c1) into their state; with
// own_only a wave walks only the part of [c0, c1) that holds its owners' own segments.  The pieces of the same owners must be launched
// in ascending, gapless column order on one stream.
hipError_t launch_lsum_fold(const LsumArgs& a, bool own_only, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, hipStream_t s);
// The state of sorted position p -> the outputs of row list[p] - row0 (other_label / other_q: or nullptr)
hipError_t launch_lsum_scatter(const LsumState* state, const uint32_t* list, uint64_t n, uint32_t row0, unsigned long long* own_q, uint32_t* other_label,
                               unsigned long long* other_q, hipStream_t s);

// ---- MaxMin diversity picking (gsim_maxmin.hip, gsim_db_maxmin) ----------------------------------------------------------
// ctl words of a call (zeroed by the host before the first pass; the ticket on its own 128-byte line)
constexpr uint32_t kMaxMinDone = 0;    // 1: picking has ended (early stop or no unpicked row left); later passes return at once
constexpr uint32_t kMaxMinPicked = 1;  // picks made so far
constexpr uint32_t kMaxMinTicket = 32; // workgroups of the current pass that have finished (the last one selects and re-zeroes it)
constexpr uint32_t kMaxMinUpdated = 64; // (u64) rows whose maxsim strictly increased, summed over passes
constexpr uint32_t kMaxMinCtlWords = 96;
struct MaxMinArgs {
    const void* rows;            // the whole table, nrows x W words
    uint64_t nrows;
    uint32_t W;
    int metric;
    float alpha, beta;
    float max_score;
    float* maxsim;               // nrows: largest score against the picks so far (-1 before pick 0), +inf for a picked row
    uint32_t* nearest;           // nrows or nullptr: position in picks of the pick that attains maxsim
    uint32_t* picks;             // npicks rows (without the row base); the seeds are there before the first pass
    float* pick_scores;          // npicks
    uint32_t* ctl;               // kMaxMinCtlWords words
    unsigned long long* partials; // nwg_total: every workgroup's smallest (maxsim bits << 32 | row) of the pass
    uint32_t npicks, nseeds;
    uint32_t nwg_total;          // workgroups of one pass over all its launches (the ticket's target)
};
// The grid of one launch of a pass over `nrows` rows of width W (the streaming loop's own geometry; nwaves % 4 == 0).
ScanGeometry maxmin_geometry(uint64_t nrows, uint32_t W, int num_cus);
// Pass p (the pick whose row is the query) over rows [r0, r0 + nrows) -- g = maxmin_geometry(nrows, ...), r0 a multiple of 64 --
// whose workgroups are numbered wg0, wg0 + 1, ... within the pass.
hipError_t launch_maxmin_pass(const MaxMinArgs& m, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t wg0, uint32_t p,
                              hipStream_t s);
// ... the same kernels with default-policy table loads (gsim_maxmin_cached.hip): for tables that fit the Infinity Cache
hipError_t launch_maxmin_pass_cached(const MaxMinArgs& m, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t wg0, uint32_t p,
                                     hipStream_t s);

// ---- threshold joins, streaming route (gsim_join.hip, gsim_db_join / gsim_db_join_queries) -------------------------------------
struct JoinArgs {
    const void* rows;            // the whole table, nrows x W words
    uint32_t W;
    int metric;
    float alpha, beta, cutoff;
    const uint32_t* left;        // the call's left rows, W words each (16-byte aligned when W % 4 == 0)
    unsigned long long* keys;    // (left row << 32) | table row: the pair buffer gsim_db_neighbors' tile kernel fills
    float* vals;                 // score
    unsigned long long* cursor;  // entries appended so far (keeps counting past cap)
    uint64_t cap;
};
// One launch of left row l's pass: table rows [r0, r0 + nrows), g = maxmin_geometry(nrows, ...), r0 a multiple of 64.
hipError_t launch_join_pass(const JoinArgs& j, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t l, hipStream_t s);
// GSIM_JOIN_BY_SCORE: the pairs sorted by (left, column) -- keys / scores as launch_nbr_csr's sort leaves them -- are sorted
// once more, stably, by (left, score descending); then indptr, indices (+ row_base) and scores_out.  keys / scores are
// overwritten; keys_tmp / cols_tmp hold n entries each.
hipError_t join_score_sort_bytes(uint64_t n, uint32_t end_bit, size_t* bytes);
hipError_t launch_join_by_score(void* tmp, size_t tmp_bytes, unsigned long long* keys, float* scores, unsigned long long* keys_tmp,
                                uint32_t* cols_tmp, uint64_t n, uint32_t end_bit, uint64_t nrows_out, uint32_t row_base, uint64_t* indptr,
                                uint32_t* indices, float* scores_out, hipStream_t s);

// ---- row sets (gsim_subset.hip, gsim_rowset_* / gsim_db_search_rows) ------------------------------------------------------------
// A set's bitmap: rowset_words(nrows) words + kRowsetPadWords zero words (the streaming route reads three consecutive words)
constexpr uint64_t kRowsetPadWords = 2;
inline uint64_t rowset_words(uint64_t nrows) { return (nrows + 31) / 32; }
// rows d_rows[0 .. n) (with the row base, all inside the table) marked in the zeroed bitmap
hipError_t launch_rowset_mark(const uint32_t* d_rows, uint64_t n, uint32_t row_base, uint64_t nrows, uint32_t* bits, hipStream_t s);
// the bitmap finished in place (src: the caller's words instead of the marks; invert: an exclusion set; zero past the last row and in
// the padding -- nalloc = words + padding) and popc[0 .. words] = its words' popcounts (popc[words] = 0)
hipError_t launch_rowset_finish(uint32_t* bits, const uint32_t* src, uint64_t nrows, uint64_t nalloc, int invert, uint32_t* popc, hipStream_t s);
// list[offs[t] ..] = the rows of word t, ascending; offs[0 .. words] = the exclusive prefix sums of popc[0 .. words]
// (launch_scan_u32: offs[words] is the set's size)
hipError_t launch_rowset_list(const uint32_t* bits, const uint32_t* offs, uint64_t nwords, uint32_t* list, hipStream_t s);
// The two scans of gsim_db_search_rows; both leave what launch_scan leaves (candidate segments of g.seg_cap slots per wave,
// seg_count, QueryState) for launch_compact and the tail behind it.
ScanGeometry subset_scan_geometry(uint64_t nrows, uint32_t W, int num_cus);  // streaming: the whole table under the mask
ScanGeometry subset_gather_geometry(uint64_t nsel, uint32_t W, int num_cus); // gather: the list
hipError_t launch_subset_scan(const ScanArgs& a, const ScanGeometry& g, const uint32_t* bits, hipStream_t s);
hipError_t launch_subset_gather(const ScanArgs& a, const ScanGeometry& g, const uint32_t* list, uint32_t nsel, hipStream_t s);

// ---- popcount indexes (gsim_popindex.hip, gsim_popindex_* / gsim_db_search_bounded) ---------------------------------------------
// bins of the popcount histogram a workgroup keeps in LDS (rows up to 4096 bits; wider rows add to the global bins directly)
constexpr uint32_t kPopcLdsBins = 4097;
// popc[r] = popc(row r) for the nrows rows of W words, hist[b] += rows with popcount b (hist: W x 32 + 1 bins, zeroed by the caller)
hipError_t launch_popindex_popc(const void* rows, uint64_t nrows, uint32_t W, uint16_t* popc, uint32_t* hist, int num_cus, hipStream_t s);
// order[0 .. n) = the rows 0 .. n - 1 sorted stably by popc (its low end_bit bits hold every value): (popcount, row) ascending
hipError_t popindex_sort_bytes(uint64_t n, uint32_t end_bit, size_t* bytes);
hipError_t launch_popindex_sort(void* tmp, size_t tmp_bytes, const uint16_t* popc, uint16_t* popc_sorted, uint32_t* order, uint64_t n,
                                uint32_t end_bit, hipStream_t s);
// (the buckets' first positions: launch_scan_u32 over hist[0 .. bins] with hist[bins] = 0 -- first[bins] is the row count)
// ub[b], b <= fp_bits: the largest score_of(metric, alpha, beta, qpop, b, c) over c in [max(0, qpop + b - fp_bits), min(qpop, b)], NaN as 0
hipError_t launch_popindex_bounds(uint32_t fp_bits, uint32_t qpop, int metric, float alpha, float beta, float* ub, hipStream_t s);
// The window scan: slots [lo, lo + n) of the popcount-ordered copy `a.rows` (n >= 1), slot i offered as row order[i]; leaves what
// launch_scan leaves (candidate segments of g.seg_cap slots per wave, seg_count, QueryState) for launch_compact and the tail behind it.
ScanGeometry popindex_scan_geometry(uint64_t n, uint32_t W, int num_cus);
hipError_t launch_popindex_scan(const ScanArgs& a, const ScanGeometry& g, const uint32_t* order, uint64_t lo, uint32_t n, hipStream_t s);

// ---- row-hash indexes (gsim_rowhash.hip, gsim_rowhash_*) -------------------------------------------------------------------------
// The table: 2 x nslots words, slot s = {row, count} at words 2 s and 2 s + 1; nslots = rowhash_slots(nrows) (gsim_rowhash_hash.h).
// A workgroup is kRowhashBlock threads; a wave's chunk is kRowhashUnroll x 64 / (W / 4) rows where W / 4 is a power of two up to 64,
// 64 rows for other rows of fewer than 32 words, else one row; the finishing pass takes 64 rows per wave.
constexpr int kRowhashBlock = 256;
constexpr int kRowhashUnroll = 4;
// every slot {GSIM_ROW_NONE, 0}
hipError_t launch_rowhash_init(uint32_t* slots, uint64_t nslots, int num_cus, hipStream_t s);
// the table's rows [r0, r1) of W words enter the slots; slot_of[row] = the slot whose group the row joined; *flag |= 1 if a probe
// went round the whole table (flag: zeroed by the caller)
hipError_t launch_rowhash_insert(const void* rows, uint64_t r0, uint64_t r1, uint32_t W, uint32_t* slots, uint64_t nslots, uint32_t* flag,
                                 unsigned long long* slot_of, int num_cus, hipStream_t s);
// rec[row]: the row's slot -> first | size << 32 of its group (no row base); bits: rowset_words(n) words, bit `row` set where the row
// is its group's first; counters[4] (zeroed by the caller): groups, groups of two rows or more, the largest size, the sizes summed;
// *flag |= 2 on a slot that cannot be
hipError_t launch_rowhash_finish(unsigned long long* rec, uint64_t n, uint32_t* slots, uint64_t nslots, uint32_t* flag, uint32_t* bits,
                                 uint64_t nbitwords, unsigned long long* counters, int num_cus, hipStream_t s);
// found[q] = row | size << 32 of the group of the table's rows identical to left row q of nl (GSIM_ROW_NONE and 0: none); read-only
hipError_t launch_rowhash_find(const void* left, uint64_t nl, const void* rows, uint32_t W, const uint32_t* slots, uint64_t nslots, uint32_t* flag,
                               unsigned long long* found, int num_cus, hipStream_t s);

// ---- group queries (gsim_group.hip, gsim_db_search_group) --------------------------------------------------------------------------
struct GroupArgs {
    const uint32_t* queries; // device, nq x W words
    const uint32_t* qpop;    // device, nq popcounts
    uint32_t nq;
    int mode;                // GSIM_GROUP_MAX / _MIN / _MEAN
    uint64_t c0, c1;         // this launch: chunks [c0, c1) of g.chunk_rows rows
    uint32_t first;          // 1: the pass's first launch (the waves' segments start empty)
};
// The grid of every launch of a pass (chunk c belongs to wave c % nwaves in all of them); seg_cap holds every row of a wave's share.
ScanGeometry group_geometry(uint64_t nrows, uint32_t W, int num_cus);
// One launch of the pass: leaves what launch_scan leaves (candidate segments, seg_count, QueryState) once the last one has run.
hipError_t launch_group_scan(const ScanArgs& a, const ScanGeometry& g, const GroupArgs& ga, hipStream_t s);
// Behind the tail: `which` of hits [h0, h1) of a block whose header carries flag 1 (device-side test; ga.c0 / c1 / first unused).
hipError_t launch_group_which(const ScanArgs& a, const GroupArgs& ga, uint32_t row_base, void* block, uint32_t h0, uint32_t h1, hipStream_t s);

// ---- label-grouped search (gsim_label_search.hip, gsim_db_search_labels) -----------------------------------------------------------
constexpr uint32_t kLabelScanWavesPerCu = 16; // every launch of the scan keeps this many waves on a compute unit, whatever its route
constexpr uint32_t kLabelLdsBudget = 144u * 1024u; // route LDS: the largest per-workgroup table (of the CU's 160 KiB)
struct LabelSearchArgs {
    const void* rows;        // device, nrows x W words
    uint64_t nrows;
    uint32_t W;
    const uint32_t* labels;  // device, nrows labels (< nlabels, or GSIM_LABEL_NONE)
    uint32_t nlabels;
    const uint32_t* queries; // device, the pass's nq x W words
    const uint32_t* qpop;    // device, their popcounts
    uint32_t nq;
    float cutoff;
    int metric;
    float alpha, beta;
    unsigned long long* best; // device, nq x nlabels candidate keys (make_key; 0: no row yet), carried from launch to launch
    uint32_t* kept;           // device, nq x nlabels kept rows -- or NULL: not counted (cutoff <= 0, or nobody asked)
    uint64_t c0, c1;          // this launch: chunks [c0, c1) of label_chunk_rows(W) rows
    uint32_t nwaves;          // waves of the grid: chunk c belongs to wave c % nwaves
    uint32_t block;           // threads of a workgroup: 256, 512 or 1024
    uint32_t lds_bytes;       // route LDS: the workgroup's table, nq x nlabels x (8, + 4 when counting) bytes; 0: route global
};
uint32_t label_chunk_rows(uint32_t W);
// the threads of a workgroup whose LDS table has `lds_bytes` (0: route global), so that kLabelScanWavesPerCu waves fit a compute unit
uint32_t label_block_threads(uint32_t lds_bytes);
hipError_t launch_label_scan(const LabelSearchArgs& a, hipStream_t s);
// Behind the last scan launch, per query of the pass: label_best[q, l] (the hit of best[q, l]: common and popc_db again from the row,
// `row` with the row base; {0xFFFFFFFF, 0, 0, 0} where best is 0), totals[2 q] += labels with a row, totals[2 q + 1] += kept[q, l]
// (not with kept == NULL)
hipError_t launch_label_finish(const LabelSearchArgs& a, uint32_t row_base, void* label_best, unsigned long long* totals, hipStream_t s);
// best[0 .. nlabels) of one query, descending, into sorted (rocprim's radix sort; tmp from label_rank_bytes)
hipError_t label_rank_bytes(uint32_t nlabels, size_t* bytes);
hipError_t launch_label_rank(void* tmp, size_t tmp_bytes, const unsigned long long* best, unsigned long long* sorted, uint32_t nlabels, hipStream_t s);
// hits[i], hit_labels[i] for i < kk: the label of sorted[i]'s row and that label's label_best; a zero key ends the list
hipError_t launch_label_emit(const unsigned long long* sorted, const uint32_t* labels, const void* label_best, uint32_t kk, void* hits,
                             uint32_t* hit_labels, hipStream_t s);

// ---- leader (sphere-exclusion) clustering (gsim_leader.hip, gsim_db_leader) --------------------------------------------------------
constexpr uint32_t kLeaderMaxRound = 4096; // largest GSIM_LEADER_ROUND (the resolve's leader mask: one 64-bit word per lane of a wave)
// ctl words of a call (device memory; the host reads them once per round)
constexpr uint32_t kLdrActive = 0;   // entries of the active list after the round's compaction (written by the compaction)
constexpr uint32_t kLdrLeaders = 1;  // leaders made so far
constexpr uint32_t kLdrRoundNl = 2;  // this round's leaders: the rows in the round buffer
constexpr uint32_t kLdrRoundPos = 3; // ... and the position in `leaders` of the first of them
constexpr uint32_t kLdrPairs = 4;    // (u64) leader x row scores evaluated
constexpr uint32_t kLdrAssigned = 6; // (u64) rows with a leader (leaders included)
constexpr uint32_t kLdrCtlWords = 8;
struct LeaderArgs {
    const void* rows;       // the whole table, nrows x W words
    uint32_t W;
    int metric;
    float alpha, beta, cutoff;
    uint32_t* leaders;      // max_leaders rows (without the row base); the seeds are there before the first round
    uint32_t* leader_of;    // nrows: position in `leaders`, GSIM_LEADER_NONE while unassigned
    float* row_score;       // nrows or nullptr
    uint32_t* round_fp;     // the round buffer: round x W words, the round's leaders densely, in order ...
    uint32_t* round_pop;    // ... and their popcounts
    unsigned long long* cover; // round x ceil(round / 64) words: bit i of row j = candidate i (< j) covers candidate j
    uint32_t* ctl;          // kLdrCtlWords words
    uint32_t max_leaders;
};
// bytes of the order-preserving compaction's scratch for lists of up to n entries
hipError_t leader_select_bytes(uint64_t n, size_t* bytes);
// leaders[0 .. nseeds) (the seeds) get leader_of / row_score; list_out = every other row, ascending; ctl[kLdrActive] = their number
// (leader_of: none everywhere, row_score: 0 everywhere before the call)
hipError_t launch_leader_first_list(const LeaderArgs& a, void* tmp, size_t tmp_bytes, uint64_t nrows, uint32_t nseeds, uint32_t* list_out,
                                    hipStream_t s);
// A seed round: leaders[pos0 .. pos0 + nc) (seeds) become the round's leaders as they are.
hipError_t launch_leader_seed_round(const LeaderArgs& a, uint32_t pos0, uint32_t nc, hipStream_t s);
// A round's resolve over the candidates list[0 .. nc): the cover bits of the nc x nc candidate pairs (one launch), then one
// workgroup that walks them in order, appends the new leaders, fills the round buffer and writes the candidates' outputs.
hipError_t launch_leader_resolve(const LeaderArgs& a, const uint32_t* list, uint32_t nc, hipStream_t s);
// One launch of a round's pass: list entries [e0, e1) against the round's leaders.  nt: non-temporal row loads.
uint32_t leader_chunk_rows(uint32_t W);
hipError_t launch_leader_pass(const LeaderArgs& a, const uint32_t* list, uint64_t e0, uint64_t e1, int num_cus, bool nt, hipStream_t s);
// list_out = the entries of list_in[0 .. n) that still have no leader, in order; ctl[kLdrActive] = their number
hipError_t launch_leader_compact(const LeaderArgs& a, void* tmp, size_t tmp_bytes, const uint32_t* list_in, uint64_t n, uint32_t* list_out,
                                 hipStream_t s);

// ---- complete- and average-linkage dendrograms (gsim_linkage.hip, gsim_db_linkage) -----------------------------------------
constexpr int kLinkBlock = 1024;      // the one workgroup of the chain kernel
constexpr uint32_t kLinkTile = 32;    // the mirror kernel's square tile: a slab starts at a multiple of it
constexpr uint32_t kLinkCtlWords = 16;
constexpr uint32_t kLinkCtlLen = 0;      // ctl words: elements on the chain
constexpr uint32_t kLinkCtlMerged = 1;   // ... merges executed
constexpr uint32_t kLinkCtlScans = 2;    // ... nearest-neighbour scans
constexpr uint32_t kLinkCtlChainMax = 3; // ... the longest the chain has been
constexpr uint32_t kLinkCtlDone = 4;     // ... 1 once n - 1 merges are executed, 2: a scan found no live slot (never)
constexpr uint32_t kLinkCtlClk = 8;      // ... the last launch's four clock words (as KnnArgs.clk)
struct LinkRaw {                 // a merge as the chain executed it
    uint32_t a, b;               // the slots (= smallest rows within the range), a < b
    uint32_t size_a, size_b;
    unsigned long long v;        // complete linkage: the bits of the minimum; average linkage: Q
};
struct LinkArgs {
    void* mat;                   // n rows of ld entries: float (complete linkage) or unsigned long long (average linkage), symmetric
    uint64_t ld;                 // a multiple of 4, >= n: every row starts on 16 bytes
    uint32_t n;
    int average;
    uint32_t* size;              // ld entries: the rows of the cluster in slot z, 0 for a dead slot and for the padding
    uint32_t* chain;             // n entries
    LinkRaw* raw;                // n - 1 entries
    unsigned long long* ctl;     // kLinkCtlWords
};
// size = 1 for z < n, 0 for the padding; ctl zeroed
hipError_t launch_link_init(const LinkArgs& a, hipStream_t s);
// in: `rows` rows of ld_in floats, the scores of the range's rows [first, first + rows) against its rows [col0, n), col0 <= first;
// `first` a multiple of kLinkTile.  For i < j both mat[i][j] and mat[j][i] become s(i, j) (complete linkage, in place: in == mat, col0 == first == 0, rows == n) or
// q(s(i, j)) (average linkage); the lower triangle of `in` is not read.
hipError_t launch_link_mirror(const LinkArgs& a, const float* in, uint64_t ld_in, uint64_t col0, uint64_t first, uint64_t rows, hipStream_t s);
// at most `steps` > 0 chain steps (a scan, then a push or a merge)
hipError_t launch_link_chain(const LinkArgs& a, uint32_t steps, hipStream_t s);

hipError_t launch_generate(void* rows, uint64_t seed, int kind, uint64_t first_row, uint64_t nrows,
                           uint32_t W, hipStream_t s);

// gsim_litmus.hip: the hardware behaviours the single launch rests on, as litmus kernels (gsim_debug_litmus)
hipError_t launch_litmus_pair(void* entries, void* headers, unsigned long long* stats, uint32_t nblocks, uint32_t iters, int with_header,
                              unsigned long long budget_ticks, hipStream_t s);
hipError_t launch_litmus_host(void* slots, const uint32_t* ack, unsigned long long* stats, uint32_t nblocks, uint32_t iters, unsigned long long budget_ticks,
                              hipStream_t s);
hipError_t launch_score_table(int metric, float alpha, float beta, uint32_t a, uint32_t max_b,
                              uint32_t max_c, float* d_out, hipStream_t s);

} // namespace gsim
