/* gpusim_hip.h -- C ABI of the MI355X-native fingerprint scan engine.
 *
 * This is the drop-in boundary for the ONE hot path of schrodinger/gpusimilarity:
 * "score every packed fingerprint of a table against a query (popcount
 * Tanimoto / Tversky), apply a cutoff, return the exact top-k".  In the
 * reference that path lives behind the C++ class gpusim::FingerprintDB
 * (fingerprintdb_cuda.h:53-140), whose stated purpose is to keep CUDA types
 * away from its callers (fingerprintdb_cuda.h:47, fingerprintdb_cuda.cpp:2-3).
 * The reference has no FFI of its own; the entry points below are what a
 * binding for that class would bind, one for each thing the class does with the
 * device.  Host C++ (gpusimilarity_amd/csrc/host/fingerprintdb.h, the Qt-free
 * twin of the reference class) reaches HIP only through these functions.
 *
 * Rules of the ABI: plain C, opaque handle, plain pointers and sizes, no HIP /
 * STL / torch types, never throws, every call returns a status (0 = ok, < 0 =
 * error, text via gsim_last_error()).  One search at a time per handle (the
 * reference serialises searches behind a function-static mutex,
 * fingerprintdb_cuda.cu:236, and its server is single threaded).
 *
 * Fingerprint layout: row-major uint32_t[nrows][fp_bits/32]; word i of a row is
 * bytes 4i..4i+3 of the RDKit BitVectToBinaryText string read little-endian --
 * the same pass-through reinterpretation as fingerprintdb_cuda.cu:117-126.
 */
#ifndef GPUSIM_HIP_H
#define GPUSIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSIM_OK 0
#define GSIM_ERR_INVALID (-1)   /* bad argument                                  */
#define GSIM_ERR_NO_DEVICE (-2) /* no usable GPU / device index out of range     */
#define GSIM_ERR_HIP (-3)       /* a HIP runtime call failed                     */
#define GSIM_ERR_NOMEM (-4)     /* host or device allocation failed              */
#define GSIM_ERR_STATE (-5)     /* call not valid in the handle's current state  */

#define GSIM_METRIC_TANIMOTO 0 /* c / (a + b - c)          fingerprintdb_cuda.cu:89-103 */
#define GSIM_METRIC_TVERSKY 1  /* c / (al*(a-c)+be*(b-c)+c) build extension (BASELINE config 5) */

#define GSIM_SYNTH_SPARSE 0 /* bit density 1/16 (Morgan-like) */
#define GSIM_SYNTH_DENSE 1  /* bit density 1/2                */
#define GSIM_SYNTH_MORGAN 2 /* Morgan-shaped rows: popcount 20..53 of 1024, a dozen very frequent bits, series of
                               analogs, table-wide scaffolds, ~3 % exact duplicates (csrc/gsim_synth.h) -- coarse,
                               tie-heavy scores like the reference's ChEMBL / Zinc / Enamine tables */

typedef struct gsim_db gsim_db;

/* One result row.  `row` is the index in the table (plus the handle's row base,
 * see gsim_db_set_row_base) -- the ABI speaks row indices; SMILES / ID strings
 * live above it (reference: m_smiles/m_ids lookups, fingerprintdb_cuda.cu:297-304).
 * `score` is the float the reference would return; `common` = popc(q & row),
 * `popc_db` = popc(row) are the integers it was computed from. */
typedef struct {
    uint32_t row;
    float score;
    uint16_t common;
    uint16_t popc_db;
} gsim_hit;

/* Header of a device-resident result block written by gsim_db_search_device and
 * gsim_merge_device: {gsim_result_header; gsim_hit hits[k];}. */
typedef struct {
    uint32_t count;  /* number of valid hits (<= k)                         */
    uint32_t flags;  /* bit 0: block produced by the general (large) path; bit 1: the single launch handed the query back
                        (internal: never set in a block a call returns); bits 8..31: zero in every returned block
                        (the library's own pinned blocks carry the query's epoch there while it polls them) */
    uint64_t approx; /* "approximate matching results", see gsim_db_search  */
} gsim_result_header;

/* Per-handle timing of the last searches, measured with HIP events on the
 * stream the kernels were launched on (gsim_db_enable_timing). */
typedef struct {
    uint64_t queries;        /* searches accumulated since enable/reset           */
    double scan_ms_sum;      /* sum of scan-kernel (dominant kernel) durations    */
    double select_ms_sum;    /* sum of compaction + final select kernel durations */
    uint64_t candidates_sum; /* rows that survived the in-scan threshold filter   */
    uint64_t finalists_sum;  /* rows handed to the final select                   */
    uint64_t handed_back;    /* queries the single-launch path handed back to the four-kernel pipeline */
    uint64_t batches;        /* multi-query passes timed (gsim_db_search with nq >= 4)                  */
    double batch_kernel_ms_sum; /* sum of their dominant kernel's durations (the matrix-core contraction,
                                   or all table passes of the VALU route)                               */
    uint64_t handed_back_why;   /* union of the reasons, since the handle was created: 1 a wave's candidate store or a
                                   workgroup's list overflowed (heavy ties, ascending scores), 2 / 4 a wait ran out
                                   (GPU shared with another process), 8 more rows at the final threshold than a
                                   selector holds, 16 more of them owned by one selector than its list holds, 64 (the publishing route: k above GSIM_FUSED_SELECT_MAX_K = 2048 and up
                                   to 100 000, bin-ranked up to 65 536 -- up to 8192 on 128 / 256-bit rows) more rows in one of the top
                                   score bins than the bin-ranked emission takes (ties)                                 */
    uint64_t batches_dense_cutoff; /* multi-query passes, since the handle was created, whose cutoff kept so many rows that the
                                      matrix-core pass counted them from its accumulators (gsim_prefilter.h cutoff_band)      */
    uint64_t collectives;          /* searches (single queries or <= 256-query batches) merged through gsim_db_set_comm's route */
    double gather_ms_sum;          /* ... their all-gather: last shard kernel enqueued on the first shard's stream -> blocks gathered */
    double merge_ms_sum;           /* ... their merge_kernel                                                                  */
    uint64_t blocks_rechecked;     /* since the handle was created: result blocks of the single launch whose checksum did not match
                                      the hits when the header arrived in host memory (the hits were still on their way) ...   */
    uint64_t blocks_torn;          /* ... and those that never matched: the query was re-run on the four-kernel pipeline      */
    uint64_t batches_regrown;      /* since the handle was created: multi-query passes run again because a wave's candidate segment
                                      overflowed (the segments start at 4 Ki slots and grow to what was asked for, up to 64 Ki)   */
    uint64_t large_k_single_scan;  /* since the handle was created: shard queries with k above 2048 whose scan was the single launch's
                                      (it publishes, other kernels rank: DESIGN.md section 3); the rest of them were ranked inside it (k up to 8192)
                                      or took the four-kernel pipeline's scan */
    /* Why synchronous queries (gsim_db_search, _each, _timed) ran a second time on the four-kernel pipeline, counted on the host
     * since the handle was created -- `handed_back` above is the DEVICE's count of single launches that ended with a hand-back and
     * equals rerun_own + rerun_publish when nothing else went wrong: */
    uint64_t rerun_own;     /* the query's own single launch handed it back (reasons: handed_back_why)                          */
    uint64_t rerun_publish; /* large k: its publishing launch, or the bin-ranked emission behind it, handed it back             */
    uint64_t rerun_behind;  /* it ran behind a launch that ended without closing its query (GPU shared: a wait ran out and the
                               kernel was gone before its header): every query in flight on that state is run again            */
    uint64_t rerun_torn;    /* = blocks_torn                                                                                    */
    uint64_t lane_queries;  /* since the handle was created: shard queries of gsim_db_search_each that ran on one of the shard's two
                               half-grid lanes (small tables: consecutive queries overlap)                  */
    uint64_t backoff_skips; /* queries routed AROUND the single launch (or its publishing mode / the bin-ranked emission) because
                               earlier ones were handed back: they scan once, on the four-kernel pipeline, and are not hand-backs */
} gsim_timing;

/* ---- device enumeration / placement ------------------------------------- */
/* get_gpu_count()            fingerprintdb_cuda.cu:40-52  */
int gsim_device_count(int* count);
/* get_gpu_free_memory(i)     fingerprintdb_cuda.cu:33-38  */
int gsim_device_free_bytes(int device, size_t* free_bytes);
/* get_available_gpu_memory() fingerprintdb_cuda.cu:401-413: sum of free bytes */
int gsim_available_device_bytes(size_t* total_free_bytes);
/* get_next_gpu(required)     fingerprintdb_cuda.cu:54-68: round-robin over the
 * devices, skipping those without `required_bytes` free.  (The reference tests
 * device i but returns the round-robin device -- a latent bug, :57-62; here the
 * device that is returned is the one that was checked.)  GSIM_ERR_NO_DEVICE with
 * no GPU, GSIM_ERR_NOMEM when none has room (reference: throws, :65-66). */
int gsim_next_device(size_t required_bytes, int* device);

/* ---- table lifecycle ------------------------------------------------------ */
/* FingerprintDB::FingerprintDB   fingerprintdb_cuda.cu:133-166.  fp_bits must be
 * a positive multiple of 32 (":140 ASSUMES INT-DIVISIBLE SIZE"), <= 32768. */
int gsim_db_create(uint32_t fp_bits, gsim_db** out);
/* FingerprintDBStorage ctor      fingerprintdb_cuda.cu:111-126: appends one slice
 * of host rows (copied; the caller keeps its buffer).  Slices are concatenated in
 * call order; global row = slice offset + local (getOffsetIndex, :128-131). */
int gsim_db_add_rows(gsim_db* db, const uint32_t* rows, uint64_t nrows);
/* FingerprintDB::copyToGPU(1)    fingerprintdb_cuda.cu:168-183: uploads the rows
 * and allocates the search scratch.  ndevices == 1: the whole table goes to
 * `device` (device < 0: gsim_next_device picks).  ndevices > 1: rows are split
 * into ndevices contiguous shards on devices device .. device+ndevices-1
 * (ndevices == 0: all devices).  The host copy is kept (reference keeps m_data,
 * fingerprintdb_cuda.h:46) for gsim_db_row and gsim_db_search_cpu. */
int gsim_db_finalize(gsim_db* db, int device, int ndevices);
/* FingerprintDB::copyToGPU(fold_factor > 1)  fingerprintdb_cuda.cu:168-195 + fold_data
 * fingerprintdb_cuda.cpp:56-69: call before gsim_db_finalize.  The table is then kept
 * on the GPU OR-folded to fp_bits / F bits (F = the smallest factor >= fold_factor that
 * divides the word count, :170-173), one shard per add_rows slice (one reference
 * "storage" each).  gsim_db_search on a folded table is the reference's approximate
 * search: the k*F*(int)log2(2F) best folded scores per storage (:284-287) are
 * re-scored with the full fingerprints from the host copy (:307-331).  Tanimoto only.
 * Not needed on MI355X for capacity (288 GB hold 2.25 G unfolded 1024-bit rows). */
int gsim_db_set_fold_factor(gsim_db* db, uint32_t fold_factor);
uint32_t gsim_db_fold_factor(const gsim_db* db);
/* Folded tables: may gsim_db_finalize also place the storages' FULL fingerprints in HBM, so that the candidates are
 * re-scored on the GPU instead of on the host?  1 (default): yes, when all of them fit next to the folded rows and the
 * search scratch with 2 GB to spare, on every device -- all storages or none; 0: never (callers that fold because the
 * tables do NOT fit and still have tables to place, e.g. a server loading several databases).  Before gsim_db_finalize. */
int gsim_db_set_fold_full_on_device(gsim_db* db, int allow);
/* FoldFingerprintFunctorCPU (calculation_functors.cpp:22-41) for one fingerprint of
 * `words` 32-bit words: out receives words / fold_factor words (host function). */
int gsim_fold_fingerprint(const uint32_t* fingerprint, uint32_t words, uint32_t fold_factor,
                          uint32_t* out);
/* Synthetic table generated directly in HBM (no host copy): row r, word j =
 * the counter-based generator of SURVEY.md 8d (oracle/gsim_oracle.c
 * gso_synth_word is the CPU twin), rows first_row .. first_row+nrows-1.
 * Replaces add_rows+finalize for benchmark tables that exceed host memory. */
int gsim_db_generate(gsim_db* db, uint64_t seed, int kind, uint64_t first_row,
                     uint64_t nrows, int device);
/* The same table split over `ndevices` GPUs (device .. device + ndevices - 1) exactly as
 * gsim_db_finalize(db, device, ndevices) splits uploaded rows -- contiguous, equal shares -- each
 * shard generated on its own device: the one-process multi-GPU handle of fingerprintdb_cuda.cu:176-182
 * for tables that exceed host memory (bench.py --in-process, gpusimserver synthetic:... --gpus N). */
int gsim_db_generate_sharded(gsim_db* db, uint64_t seed, int kind, uint64_t first_row,
                             uint64_t nrows, int device, int ndevices);
/* Row `row` of that synthetic table, computed on the host by the generator's own code (benchmark
 * queries are rows of the table; no device, no handle needed). */
int gsim_synth_row(uint64_t seed, int kind, uint64_t row, uint32_t fp_bits, uint32_t* out_words);
/* Borrow rows that already live in device memory (e.g. a torch tensor); the
 * caller keeps ownership and must keep them alive.  16-byte aligned. */
int gsim_db_attach_device_rows(gsim_db* db, const void* d_rows, uint64_t nrows,
                               int device);
int gsim_db_destroy(gsim_db* db);

/* FingerprintDB::count()                  fingerprintdb_cuda.h:74  */
uint64_t gsim_db_count(const gsim_db* db);
/* FingerprintDB::getFingerprintBitcount() fingerprintdb_cuda.h:123-126 */
uint32_t gsim_db_fp_bits(const gsim_db* db);
/* FingerprintDB::getFingerprintDataSize() fingerprintdb_cuda.h:122 */
size_t gsim_db_data_bytes(const gsim_db* db);
/* FingerprintDB::getFingerprint(index)    fingerprintdb_cuda.cu:212-226 */
int gsim_db_row(const gsim_db* db, uint64_t row, uint32_t* out_words);
/* number of device shards the table was placed on (1 unless ndevices > 1) */
int gsim_db_shard_count(const gsim_db* db);
/* the device shard `shard` lives on (-1: no such shard) -- the order gsim_comm_create wants */
int gsim_db_shard_device(const gsim_db* db, int shard);

/* ---- search --------------------------------------------------------------- */
/* FingerprintDB::search          fingerprintdb_cuda.cu:341-381 (+ search_storage
 * :228-339).  For each of the nq queries (nq * fp_bits/32 words, host memory):
 *   score(row) = metric(query, row); score = score >= cutoff ? score : 0  (:101;
 *   NaN -> 0); rows kept = all rows when cutoff <= 0, else rows with score != 0
 *   (:263-273); approx[q] = #kept (:272-277, :367-369); hits = the first
 *   min(k, #kept) kept rows in the order (score desc, row asc) -- the set the
 *   reference's sort_by_key returns, in canonical order (within a tie group the
 *   reference's own order depends on heap addresses, :366).
 * hits: caller-allocated nq*k entries, query q's hits at hits[q*k ..];
 * counts[q] = number of valid hits; approx may be NULL.  alpha/beta are used by
 * GSIM_METRIC_TVERSKY only.  Four or more queries in one call share table passes
 * (up to 256 per pass; on the matrix cores for 256..2048-bit rows) -- purely an
 * execution detail: every query gets exactly the result a call with nq = 1 would
 * return. */
int gsim_db_search(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k,
                   float cutoff, int metric, float alpha, float beta, gsim_hit* hits,
                   uint32_t* counts, uint64_t* approx);
/* The same call with the queries answered strictly one after the other through the single-query path
 * (FingerprintDB::search called nq times, as the reference's server does, gpusim.cpp:306-374): no table
 * pass is shared.  On a single-shard handle up to eight queries are enqueued ahead of the one being waited for
 * (each with its own pinned result block): they still run one at a time on the GPU, but the next one starts when
 * the previous kernel retires, not after a host round trip. */
int gsim_db_search_each(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k,
                        float cutoff, int metric, float alpha, float beta, gsim_hit* hits,
                        uint32_t* counts, uint64_t* approx);
/* gsim_db_search for nq queries strictly ONE AT A TIME -- nothing enqueued ahead, unlike gsim_db_search_each -- with the
 * wall time of each, measured inside the library around the single-query path: seconds[q] = query q in host memory ->
 * its hits in host memory (the reference's server logs the same interval per request, gpusim.cpp:420-429).  What a
 * caller of gsim_db_search with nq = 1 waits for, without the caller's own binding overhead. */
int gsim_db_search_timed(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, int metric,
                         float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx, double* seconds);
/* FingerprintDB::search_cpu      fingerprintdb_cuda.cpp:20-54: the reference's
 * explicit host path (TanimotoFunctorCPU on all host threads + the partial
 * bubble sort of :92-103).  Same outputs as gsim_db_search, but reference
 * semantics: cutoff is ignored, NaN scores are kept, approx is not written,
 * and k > count is an error (the reference reads out of bounds).  Needs the host
 * copy.  Never used by gsim_db_search -- there is no CPU fallback. */
int gsim_db_search_cpu(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k,
                       float cutoff, gsim_hit* hits, uint32_t* counts);

/* ---- device-resident results (one process per GPU + RCCL gather) ---------- */
/* All kernels of this handle are enqueued on `hip_stream` (a hipStream_t passed
 * as void*; NULL = the handle's own stream). */
int gsim_db_set_stream(gsim_db* db, void* hip_stream);
/* Added to every returned row index: the shard's first global row. */
int gsim_db_set_row_base(gsim_db* db, uint32_t row_base);
/* bytes of one result block for top-k: sizeof(header) + k*sizeof(gsim_hit),
 * rounded up to 16. */
size_t gsim_result_block_bytes(uint32_t k);
/* One query, single-shard handle: leaves {header; hits[k]} in device memory at
 * d_result (gsim_result_block_bytes(k) bytes), enqueued on the handle's stream,
 * no host synchronisation for any k (k > 8192: a radix select on the device finds
 * the k-th best key, nothing is sized by a count the host would have to read) --
 * except that the FIRST call with a k above the largest one seen so far allocates
 * its buffers (hipMalloc synchronises the device once).
 * query is host memory (fp_bits/32 words). */
int gsim_db_search_device(gsim_db* db, const uint32_t* query, uint32_t k, float cutoff,
                          int metric, float alpha, float beta, void* d_result);
/* Merge nblocks result blocks (contiguous in device memory, block_bytes apart,
 * e.g. the output of an RCCL all-gather) into one block holding the first k of
 * their union in canonical order; approx = sum.  FingerprintDB::search's host
 * merge, fingerprintdb_cuda.cu:363-380.  Enqueued on hip_stream of `device`. */
int gsim_merge_device(int device, void* hip_stream, const void* d_blocks,
                      uint32_t nblocks, size_t block_bytes, uint32_t k, void* d_result);

/* nq queries (host memory, nq x fp_bits/32 words), single-shard handle: result
 * block q = {header; hits[k]} at d_results + q * gsim_result_block_bytes(k) in
 * device memory, enqueued on the handle's stream.  Batches share table passes
 * (the multi-query / matrix-core pass) exactly as in gsim_db_search; the call
 * waits for the handle's stream once per 256 queries (queries that need the
 * single-query pipeline -- heavy ties, candidate overflow -- are re-enqueued
 * before it returns).  Reference: the per-storage half of FingerprintDB::search,
 * fingerprintdb_cuda.cu:228-339, for a batch (build-defined). */
int gsim_db_search_batch_device(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k,
                                float cutoff, int metric, float alpha, float beta,
                                void* d_results);
/* gsim_merge_device for nq queries at once: d_blocks holds nranks arrays of nq
 * result blocks (rank-major, the layout an all-gather of each rank's
 * gsim_db_search_batch_device output produces); merged block q goes to
 * d_results + q * block_bytes. */
int gsim_merge_device_batch(int device, void* hip_stream, const void* d_blocks,
                            uint32_t nranks, uint32_t nq, size_t block_bytes, uint32_t k,
                            void* d_results);

/* Host twin of gsim_merge_device for result blocks that are in host memory (the
 * in-process multi-device path, and the gloo/CPU tests of the gather+merge
 * logic): std::sort + truncate exactly as fingerprintdb_cuda.cu:363-380. */
int gsim_merge_host(const void* blocks, uint32_t nblocks, size_t block_bytes, uint32_t k,
                    void* result);

/* ---- in-process collective: per-GPU top-k merged via an RCCL all-gather ---- */
/* FingerprintDB::search runs one host thread per storage and merges their results on the host
 * (fingerprintdb_cuda.cu:356-380); gsim_db_search on a multi-device handle does the same by default.  With a
 * communicator attached, every shard's kernels leave their result block in their own device's HBM, ONE grouped
 * ncclAllGather over the shards' streams (RCCL over xGMI; 16 + 12 k bytes per device) brings the blocks to every
 * device and a merge kernel on the first shard's device writes the merged block into pinned host memory -- no
 * PyTorch, no second process.  Results are identical to the host merge's, bit for bit. */
typedef struct gsim_comm gsim_comm;
/* ncclCommInitAll over `devices` (distinct device indices, in the order of the handle's shards:
 * gsim_db_finalize(db, device, n) places shard i on device + i). */
int gsim_comm_create(const int* devices, int ndevices, gsim_comm** out);
int gsim_comm_destroy(gsim_comm* comm); /* detach it from every handle first (gsim_db_set_comm(db, NULL)) */
/* The RCCL this process is bound to: NCCL_VERSION_CODE of the header the library was built with, ncclGetVersion() of the
 * library the loader resolved, and that library's file (a process that imported PyTorch first runs on PyTorch's own
 * librccl.so, not /opt/rocm/lib's).  gsim_comm_create refuses a different MAJOR version; a different minor one is this
 * call's to report (the entry points used are unchanged across 2.x).  Any pointer may be NULL. */
int gsim_rccl_info(int* header_version, int* runtime_version, char* path, size_t path_bytes);
int gsim_comm_size(const gsim_comm* comm);
/* Route gsim_db_search / gsim_db_search_each of this handle through the communicator (NULL: back to the host
 * merge).  The communicator's devices must be the shards' devices, in order.  Not for folded tables. */
int gsim_db_set_comm(gsim_db* db, gsim_comm* comm);
/* Which shard's device merges the gathered blocks and answers the host (default 0; after the all-gather every
 * device holds all blocks, so any of them can). */
int gsim_db_set_comm_root(gsim_db* db, int shard);

/* ---- all-pairs neighbour lists (similarity self-join) and Taylor-Butina clustering ---------------------------------------------- */
/* gsim_db_neighbors: every pair of rows whose similarity is at or above `cutoff` (no counterpart in the reference, which only
 * answers top-k queries).  Single-shard, unfolded handles only (GSIM_ERR_STATE otherwise: multi-shard handles, folded tables, a
 * table not yet on a GPU); tables from gsim_db_generate and gsim_db_attach_device_rows work, no host copy is needed.  For the rows
 * [row_begin, row_end) of a handle with N rows:
 *   - row i's list holds every row j != i with score(query = row i, row j) >= cutoff, where the score is bit for bit the `score`
 *     gsim_db_search returns for that pair.  Tanimoto 0/0 is NaN, so an all-zero row is nobody's neighbour; identical rows
 *     (score 1.0) are neighbours;
 *   - cutoff must be in (0, 1] (cutoff <= 0 would be N^2 output): GSIM_ERR_INVALID otherwise;
 *   - metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with alpha == beta (symmetric; 0.5 / 0.5 is Dice).  Asymmetric
 *     Tversky is GSIM_ERR_INVALID;  rows of up to 4096 bits (wider: GSIM_ERR_INVALID);
 *   - the result is CSR: indptr[row_end - row_begin + 1] (uint64), indices (uint32: the row plus the handle's row base, as in
 *     gsim_hit.row), scores (float).  Each row's list is sorted by column, ascending; the output is byte-identical from run to run;
 *   - a full-table call (0, N) computes each unordered pair once (the upper triangle) and lists it under both rows: exact for both
 *     metrics, because swapping the rows swaps a + b (Tanimoto) or the two Tversky terms (alpha == beta) and f32 addition commutes.
 *     Any other range computes the rectangle [row_begin, row_end) x [0, N); pieces of a table give the full call's lists.
 * Runs on the handle's stream under the handle's one-call-at-a-time rule, and leaves the search state as it was.  The handle keeps
 * its pair buffer (12 bytes per listed pair) for the next call. */
typedef struct gsim_graph gsim_graph;
typedef struct {
    uint64_t launches;       /* tile-kernel launches of the call (each covers a bounded piece of the pair space)             */
    uint64_t launches_rerun; /* ... run once more because the pair buffer overflowed (it grows to the exact size first)     */
    uint64_t pairs;          /* pairs found: unordered pairs for a full-table call, listed entries for a range              */
    double tile_ms;          /* HIP events on the handle's stream: all tile-kernel launches, reruns included                */
    double csr_ms;           /* sort by (row, column) + row offsets, on the device                                          */
    double d2h_ms;           /* CSR into host memory                                                                        */
    double wall_ms;          /* the whole call, host clock                                                                  */
    double clock_mhz;        /* shader clock the tile kernel ran at: s_memtime cycles over the 100 MHz wall clock, summed over
                                one full tile of every launch                                                                */
} gsim_graph_stats;
int gsim_db_neighbors(gsim_db* db, float cutoff, int metric, float alpha, float beta, uint64_t row_begin, uint64_t row_end,
                      gsim_graph** out);
int gsim_graph_shape(const gsim_graph* g, uint64_t* nrows, uint64_t* nnz);
/* indptr: nrows + 1 entries; indices, scores: nnz entries (either may be NULL) */
int gsim_graph_copy(const gsim_graph* g, uint64_t* indptr, uint32_t* indices, float* scores);
int gsim_graph_get_stats(const gsim_graph* g, gsim_graph_stats* out);
int gsim_graph_destroy(gsim_graph* g);
/* Taylor-Butina clustering of a symmetric CSR graph (host code, no device; e.g. gsim_db_neighbors' output with row base 0).
 * Rule (RDKit's Butina.ClusterData order: it sorts (count, index) tuples in reverse):
 *   - candidates are taken in order of (neighbour count descending, row index descending);
 *   - a candidate that is already assigned is skipped;
 *   - otherwise it becomes a centroid, and it and all its still-unassigned neighbours form the next cluster;
 *   - cluster ids follow creation order.
 * cluster_of[nrows] receives each row's cluster id, centroids[0 .. *nclusters) the centroid of each cluster (capacity nrows).
 * GSIM_ERR_INVALID for a malformed graph (indptr not starting at 0 or decreasing, a column >= nrows). */
int gsim_butina(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, uint32_t* cluster_of, uint32_t* centroids,
                uint64_t* nclusters);

/* ---- threshold joins: every table row at or above a cutoff, per left row --------------------------------------------------------- */
/* gsim_db_join_queries / gsim_db_join: for each of nl LEFT rows -- the nq fingerprints at `queries` (host memory, nq x fp_bits / 32
 * words), or the rows [lrow_begin, lrow_end) of another handle `left` that is resident on the same device -- the list of EVERY row
 * of the table `db` at or above `cutoff` (chemfp's threshold search; with many left rows a library-against-library join; with
 * Tversky 1 / 0 at cutoff 1.0 the fingerprint screen "rows whose bits include all of the left row's").  No counterpart in the
 * reference.  The result is a gsim_graph: gsim_graph_shape / _copy / _destroy work on it, gsim_graph_get_stats reports the call's
 * totals (launches of either route, the time of all of them in tile_ms), gsim_graph_get_join_stats the details.
 *   - list i (i = position in `queries`, or left row - lrow_begin) holds every table row j with
 *     score(query = left row i, row j) >= cutoff, where the score is bit for bit the `score` gsim_db_search returns for that query
 *     and that row (a = popc(left row), b = popc(table row)).  NaN (0 / 0) is never >= cutoff: an all-zero left row has an empty
 *     list.  No pair is excluded: joining a handle with itself (left == db is allowed) lists every non-zero row under itself, 1.0;
 *   - indices = table row + the TABLE handle's row base (as gsim_hit.row; the left handle's base plays no part); indptr has nl + 1
 *     entries;
 *   - cutoff must be in (0, 1];
 *   - metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite alpha >= 0, beta >= 0 -- asymmetric included;
 *   - order GSIM_JOIN_BY_ROW: each list by table row, ascending.  GSIM_JOIN_BY_SCORE: (score descending, row ascending), exactly the
 *     order of gsim_db_search's hits.  Either way the output is byte-identical from run to run and does not depend on the route:
 *     calls of at most GSIM_JOIN_STREAM_MAX_ROWS left rows (read once per handle, the table's) stream the table once
 *     per left row, larger ones run gsim_db_neighbors' tile kernel on the rectangle left x table;
 *   - GSIM_ERR_INVALID, checked before any device state: NULL db / out / left (NULL queries with nq > 0), unknown metric or order,
 *     cutoff outside (0, 1] or NaN, Tversky alpha / beta negative or not finite, nl >= 2^32, a table of 2^32 rows or more,
 *     lrow_begin > lrow_end or lrow_end past the left handle's count, handles of different fp_bits, rows wider than 4096 bits.
 *     GSIM_ERR_STATE: either handle multi-shard, folded or not on a GPU; handles on different devices.  nl == 0: an empty graph
 *     (indptr = {0}), GSIM_OK;
 *   - tables from gsim_db_generate and gsim_db_attach_device_rows work on either side; no host copy is needed;
 *   - runs on the table handle's stream under the one-call-at-a-time rule (of both handles), leaves the search state of both as it
 *     was, and keeps the pair buffer with the table handle (shared with gsim_db_neighbors; 12 bytes per listed pair; sorting takes
 *     about as much again for the length of the call).  If device memory for the call's exact size cannot be had:
 *     GSIM_ERR_NOMEM, nothing truncated, nothing leaked. */
#define GSIM_JOIN_BY_ROW   0   /* each list by table row, ascending                                   */
#define GSIM_JOIN_BY_SCORE 1   /* each list in gsim_db_search's order: score descending, row ascending */
typedef struct {
    uint64_t rows_streamed;   /* left rows taken by the streaming route (one pass over the table each)                        */
    uint64_t rows_tiled;      /* left rows taken by the tile route                                                            */
    uint64_t stream_launches; /* launches of the streaming kernel (a pass over a long table is cut into launches of <= ~7 ms) */
    uint64_t tile_launches;   /* launches of the tile kernel                                                                  */
    uint64_t launches_rerun;  /* ... of either, run once more because the pair buffer overflowed (it grows to the exact size)  */
    uint64_t pairs;           /* entries listed                                                                               */
    double stream_ms;         /* HIP events on the table handle's stream: all streaming launches, reruns included             */
    double tile_ms;           /* ... all tile launches                                                                        */
    double csr_ms;            /* the sort(s) + row offsets, on the device                                                     */
    double d2h_ms;            /* CSR into host memory                                                                         */
    double wall_ms;           /* the whole call, host clock                                                                   */
    double clock_mhz;         /* tile route: shader clock the kernel ran at (as gsim_graph_stats.clock_mhz); 0 when streaming */
} gsim_join_stats;
int gsim_db_join_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, float cutoff, int metric, float alpha, float beta,
                         int order, gsim_graph** out);
int gsim_db_join(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, float cutoff, int metric, float alpha,
                 float beta, int order, gsim_graph** out);
int gsim_graph_get_join_stats(const gsim_graph* g, gsim_join_stats* out); /* GSIM_ERR_INVALID for a gsim_db_neighbors result */

/* ---- MaxMin diversity picking --------------------------------------------------------------------------------------------------- */
/* gsim_db_maxmin: `npicks` mutually dissimilar rows of a single-shard, unfolded handle with N rows, by the MaxMin rule (RDKit's
 * MaxMinPicker; no counterpart in the reference).  One pass over the table per pick, on the device.
 *   - score(p, i) is bit for bit the `score` gsim_db_search returns for query = row p against row i; a NaN score (0/0: both rows
 *     all-zero) counts as 0.0.  Metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with alpha == beta, finite and >= 0 (then
 *     every score is in [0, 1] or NaN);
 *   - picks 0 .. nseeds-1 are the seeds (rows including the row base), in the order given; with nseeds == 0 pick 0 is row 0;
 *   - every later pick is the unpicked row i with the smallest maxsim[i] = max over the earlier picks p of score(p, i), ties to
 *     the lowest row.  (Smallest maximum similarity is RDKit's largest minimum distance: 1 - s is exact in double for every
 *     score of this engine, 0 or c / den with integer operands <= 65 535.)  The result does not depend on reduction order;
 *   - max_score in [0, 1]: picking ends before the first non-seed candidate whose maxsim > max_score (1.0: never early);
 *     *npicked = the number of picks made.  Duplicates of picks are picked too, in their turn (maxsim 1.0);
 *   - picks[j] = the row plus the handle's row base (as gsim_hit.row); pick_scores[j] (or NULL) = the maxsim of pick j when it was
 *     picked, its largest score against picks 0 .. j-1 (0.0 for pick 0; seeds too);
 *   - row_score[N] and nearest[N] (either may be NULL): every row's final maxsim, and the position in picks of the pick that
 *     attains it (ties to the earliest pick: only a strictly greater score moves it).  A picked row reports 1.0 and its own
 *     position.  Together: an assignment of every row to its nearest diverse centroid.
 * GSIM_ERR_INVALID, checked before any device state: npicks > N, nseeds > npicks, a seed outside [row_base, row_base + N) or
 * repeated, max_score outside [0, 1] or NaN, an asymmetric Tversky metric or alpha = beta < 0 / not finite, NULL picks / npicked
 * (or NULL seeds with nseeds > 0), N >= 2^32.  GSIM_ERR_STATE: multi-shard handles, folded tables, a table not on a GPU.
 * npicks == 0 does nothing.  Runs on the handle's stream under the one-call-at-a-time rule and leaves the search state as it was;
 * device memory for the call (4 B per row, 8 B with `nearest`) is allocated and freed by the call. */
typedef struct {
    uint64_t picks;        /* picks made (seeds included)                                                                     */
    uint64_t launches;     /* kernel launches of the call (a pass over a long table is cut into launches of <= ~5 ms)         */
    uint64_t rows_updated; /* sum over passes of the rows whose maxsim strictly increased (their state was stored)           */
    double kernel_ms;      /* HIP events around all pass launches                                                             */
    double d2h_ms;         /* outputs to the host                                                                             */
    double wall_ms;        /* the whole call, host clock                                                                      */
} gsim_maxmin_stats;
int gsim_db_maxmin(gsim_db* db, uint32_t npicks, const uint32_t* seeds, uint32_t nseeds, int metric, float alpha, float beta,
                   float max_score, uint32_t* picks, float* pick_scores, uint32_t* npicked, float* row_score, uint32_t* nearest,
                   gsim_maxmin_stats* stats);

/* ---- row sets: exact top-k search restricted to a subset of the table ------------------------------------------------------------- */
/* A gsim_rowset is a set of rows of ONE single-shard, unfolded handle ("the compounds in stock", "the rows that passed the property
 * filter", "this Butina cluster", "everything except what we already bought"); gsim_db_search_rows searches inside it.  No
 * counterpart in the reference.
 * THE RESULT RULE: for every query the result is exactly what gsim_db_search would return on a table holding only the selected rows,
 * in ascending row order, with every hit's `row` mapped back to the original row (+ the row base):
 *   - scores, `common` and `popc_db` are bit for bit gsim_db_search's; the order is (score descending, row ascending); the boundary
 *     tie group keeps its lowest selected rows; counts[q] = min(k, kept);
 *   - approx[q] (approx may be NULL) = the number of selected rows when cutoff <= 0, else the number of selected rows with
 *     score >= cutoff (NaN is never counted);
 *   - an empty set is legal: zero hits, approx 0.  A set of all rows gives gsim_db_search's result byte for byte.
 * Rows: gsim_rowset_from_rows takes row indices INCLUDING the handle's row base, i.e. gsim_hit.row values -- hit lists, MaxMin picks,
 * Butina members and join columns go straight in -- in any order; duplicates collapse (set semantics).  gsim_rowset_from_bitmap: bit
 * r % 32 of word r / 32 selects row r WITHOUT the row base; the caller supplies (count + 31) / 32 words; bits past the last row are
 * ignored.  GSIM_ROWSET_EXCLUDE: the set is every row of the table except the ones given.  gsim_rowset_rows writes the set's
 * gsim_rowset_count rows, ascending, row base included.
 * Lifetime: a row set belongs to the handle it was made for, lives in that handle's device memory (one bit per table row + 4 bytes
 * per selected row), is immutable and serves any number of searches; destroy it before its handle.
 * Execution: gsim_db_search_rows runs on the handle's stream under the one-call-at-a-time rule, answers the nq queries one after
 * another (k is the stride of `hits`, as gsim_db_search's), and leaves the search state as it found it: a gsim_db_search before and
 * after returns identical bytes, the back-off counters and the lanes are untouched.  Per call it either GATHERS the selected rows
 * (sparse sets: reads only them) or STREAMS the table under the set's bitmap (dense sets): gather when
 * selected x max(row bytes, 128) x 1000 <= GSIM_SUBSET_GATHER_MAX_PERMILLE x N x row bytes (read once per handle; 0: always stream,
 * 1000 or more: always gather).  The result does not depend on the route.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / out / rs / queries / hits / counts / bits (NULL rows with n > 0),
 * unknown flag bits, a row outside [row_base, row_base + N), n >= 2^32, a table of 2^32 rows or more, a row set made for another
 * handle, an unknown metric (gsim_db_search's checks; like it, k == 0 is legal and returns no hits).  *out is cleared on failure.
 * GSIM_ERR_STATE: a table not on a GPU, a multi-shard handle, a folded table.  GSIM_ERR_NOMEM as elsewhere. */
typedef struct gsim_rowset gsim_rowset;
#define GSIM_ROWSET_EXCLUDE 1u  /* the set is every row of the table EXCEPT the ones given */
typedef struct {
    uint64_t selected;       /* rows in the set                                                                               */
    uint64_t queries_gather; /* queries answered by the gather route                                                          */
    uint64_t queries_stream; /* queries answered by the streaming route                                                       */
    uint64_t launches;       /* kernel launches: per query the scan, the compaction and the select (k > 8192: three for it)   */
    double kernel_ms;        /* HIP events around every query's launches, summed                                              */
    double wall_ms;          /* the whole call, host clock                                                                    */
} gsim_rowset_stats;
int gsim_rowset_from_rows(gsim_db* db, const uint32_t* rows, uint64_t n, uint32_t flags, gsim_rowset** out);
int gsim_rowset_from_bitmap(gsim_db* db, const uint32_t* bits, uint32_t flags, gsim_rowset** out);
int gsim_rowset_count(const gsim_rowset* rs, uint64_t* n);
int gsim_rowset_rows(const gsim_rowset* rs, uint32_t* rows);   /* ascending, count entries, row base included */
int gsim_rowset_destroy(gsim_rowset* rs);
int gsim_db_search_rows(gsim_db* db, const gsim_rowset* rs, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, int metric,
                        float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx, gsim_rowset_stats* stats /* or NULL */);

/* ---- group queries: exact top-k by MAX, MIN or MEAN similarity to a set of queries ---------------------------------------------- */
/* gsim_db_search_group ranks the table by its similarity to a SET of nq queries ("the known actives") in one pass over the table:
 * by the nearest of them (MAX: group fusion, 1-NN scoring), by the farthest (MIN: "similar to all of them") or by their mean (MEAN).
 * Single-shard, unfolded handles.  No counterpart in the reference.
 * THE RESULT RULE:
 *   - pair score: s_i(r) is the `score` gsim_db_search returns for query i and row r at cutoff 0, bit for bit; NaN (0 / 0) counts as 0.0;
 *   - GSIM_GROUP_MAX:  g(r) = max_i s_i(r), `which` = the lowest i that attains it;
 *     GSIM_GROUP_MIN:  g(r) = min_i s_i(r), `which` = the lowest i that attains it;
 *     GSIM_GROUP_MEAN: g(r) = fdiv_rn(acc_M, (float) M) with acc_0 = 0.0f, acc_{i+1} = fadd_rn(acc_i, s_i(r)) -- one IEEE f32 rounding per
 *     step, in query order 0 ... M-1, no contraction (the order is part of the rule: another order gives other bits); `which` = 0;
 *   - cutoff and approx: the group score is then treated exactly as a single query's score: g = g >= cutoff ? g : 0; with cutoff <= 0
 *     every row is kept, otherwise the rows with g != 0; *approx (may be NULL) = the number kept.  The cutoff applies to the group
 *     score, never to a pair score;
 *   - hits: the first min(k, kept) kept rows in (score descending, row ascending) order -- the boundary tie group keeps its lowest
 *     rows; *count = their number; `row` includes the handle's row base, popc_db = popc(row);
 *   - k == 0 is legal and returns no hits; nq == 1 gives gsim_db_search's rows, scores and popc_db, with which = 0;
 *   - the output is byte-identical from run to run.
 * Alpha and beta: every pair score must lie in [0, 1] (or be NaN) -- the streaming filter's range, and what makes acc_M <= M, so
 * g <= 1, by the monotonicity of rounding.  Tanimoto always does.  Tversky is accepted with finite alpha >= 0, beta >= 0 and
 * alpha + beta >= 1 (compared in double).  The bound itself rests on alpha >= 0 and beta >= 0 alone: common <= popc of either side, so
 * both products are >= 0 in f32, a sum of non-negative terms rounds to something >= each term, hence den >= (float) common and
 * fdiv_rn(common, den) <= 1 (a product that overflows to +inf gives score 0; den == 0 only with common == 0: NaN, counted as 0).
 * Merging: `row` carries the row base and the order is the canonical one, so the blocks of several single-shard handles over slices
 * of one table ({gsim_result_header; hits}, gsim_group_hit has gsim_hit's layout) merge with gsim_merge_host.
 * Execution: on the handle's stream under the one-call-at-a-time rule; the pass is cut into launches of at most
 * GSIM_GROUP_LAUNCH_PAIRS row x query pairs (read once per handle; unset: by the row width).  The call leaves the search state as it found
 * it: a gsim_db_search before and after returns identical bytes; the back-off counters, the lanes and the pipeline slots are
 * untouched.  Tables made by gsim_db_generate or gsim_db_attach_device_rows work as any other: no host copy is needed.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / queries / hits / count, nq == 0 or nq > GSIM_GROUP_MAX_QUERIES, an
 * unknown mode or metric, the alpha / beta condition, rows wider than 4096 bits, a table of 2^32 rows or more.
 * GSIM_ERR_STATE: a table not on a GPU, a multi-shard handle, a folded table.  GSIM_ERR_NOMEM as elsewhere. */
#define GSIM_GROUP_MAX  0
#define GSIM_GROUP_MIN  1
#define GSIM_GROUP_MEAN 2
#define GSIM_GROUP_MAX_QUERIES 1024u
typedef struct { uint32_t row; float score; uint16_t which; uint16_t popc_db; } gsim_group_hit;  /* 12 bytes, gsim_hit's layout */
typedef struct {
    uint64_t queries;   /* M                                                                                                  */
    uint64_t launches;  /* kernel launches: the scan's + the tail's (compaction, select; k > 8192: three for it) + `which`'s  */
    uint64_t pairs;     /* rows x M scored                                                                                    */
    double   scan_ms;   /* HIP events around the scan launches                                                                */
    double   kernel_ms; /* scan + tail                                                                                        */
    double   wall_ms;   /* the whole call, host clock                                                                         */
} gsim_group_stats;
int gsim_db_search_group(gsim_db* db, const uint32_t* queries, uint32_t nq, int mode, uint32_t k, float cutoff,
                         int metric, float alpha, float beta,
                         gsim_group_hit* hits, uint32_t* count, uint64_t* approx /* or NULL */,
                         gsim_group_stats* stats /* or NULL */);

/* ---- leader (sphere-exclusion) clustering ----------------------------------------------------------------------------------------- */
/* gsim_db_leader clusters a single-shard, unfolded handle with N rows by the leader rule (sphere exclusion; RDKit's LeaderPicker; no
 * counterpart in the reference): it takes a radius, needs no neighbour graph, and uses O(N) memory.
 * THE RULE:
 *   - pair score: score(p, i) is bit for bit the `score` gsim_db_search returns for query = row p against row i; NaN (0 / 0) is never
 *     >= cutoff.  Metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with alpha == beta, finite and >= 0 (gsim_db_maxmin's: these
 *     are symmetric bit for bit).  cutoff is in (0, 1];
 *   - seeds: leaders 0 .. nseeds-1 are the seeds (rows including the row base), in the order given -- leaders even where one covers
 *     another (RDKit's firstPicks), each its own cluster's leader;
 *   - the walk: every non-seed row i is then taken in ascending order.  Row i is COVERED if some leader p made so far has
 *     score(p, i) >= cutoff, and then belongs to the earliest such leader, by position in `leaders`; a row that is not covered
 *     becomes the next leader.  A leader belongs to itself by definition, not by score: every all-zero row is the leader of a
 *     singleton; a duplicate of a leader is covered by it, 1.0;
 *   - the cap: max_leaders >= 1, >= nseeds and <= N (N: no cap).  The walk stops right after leader number max_leaders has been made
 *     and has covered its rows; rows that nothing covers by then stay unassigned;
 *   - leaders[0 .. *nleaders): rows plus the row base (capacity: max_leaders); leader_of[N] (or NULL): the position in `leaders` of
 *     the row's leader, GSIM_LEADER_NONE when unassigned; row_score[N] (or NULL): score(leader, row) for a covered row, 1.0 for a
 *     leader, 0.0 for an unassigned row;
 *   - the output is byte-identical from run to run, and does not depend on GSIM_LEADER_ROUND (candidates per round) or
 *     GSIM_LEADER_LAUNCH_PAIRS (how a pass is cut into launches); both are read once per handle.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / leaders / nleaders (NULL seeds with nseeds > 0), cutoff outside (0, 1]
 * or NaN, an unknown metric, asymmetric weights or weights that are negative or not finite, a seed outside [row_base, row_base + N) or
 * repeated, max_leaders outside [max(1, nseeds), N], N >= 2^32, rows wider than 4096 bits.  N == 0 does nothing and returns GSIM_OK.
 * GSIM_ERR_STATE: a table not on a GPU, a multi-shard handle, a folded table.  GSIM_ERR_NOMEM as elsewhere.
 * Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found (back-offs, lanes and
 * slots untouched); device memory for the call (12 B per row, 16 B with row_score, and the compaction's scratch) is allocated and
 * freed by the call.  The host reads one small control block per round. */
#define GSIM_LEADER_NONE 0xFFFFFFFFu
typedef struct {
    uint64_t leaders;   /* leaders made (seeds included)                                                                       */
    uint64_t rounds;    /* rounds: seed rounds + candidate rounds                                                              */
    uint64_t launches;  /* kernel launches of the call's own kernels; a compaction counts as one                               */
    uint64_t pairs;     /* (leader, row) scores the rule needed: per listed row up to its first covering leader, plus the      */
                        /* candidate pairs i < j of every round's resolve                                                      */
    uint64_t assigned;  /* rows with a leader, the leaders among them                                                          */
    double kernel_ms;   /* HIP events around every round's launches, summed                                                    */
    double d2h_ms;      /* outputs to the host                                                                                 */
    double wall_ms;     /* the whole call, host clock; wall_ms - kernel_ms - d2h_ms: the per-round control reads and set-up    */
    double resolve_ms;  /* of kernel_ms: the rounds' resolves (and seed rounds' copies)                                        */
    double compact_ms;  /* of kernel_ms: the rounds' compactions                                                               */
} gsim_leader_stats;
int gsim_db_leader(gsim_db* db, float cutoff, const uint32_t* seeds, uint32_t nseeds, uint32_t max_leaders, int metric, float alpha,
                   float beta, uint32_t* leaders, uint32_t* nleaders, uint32_t* leader_of /* or NULL */, float* row_score /* or NULL */,
                   gsim_leader_stats* stats /* or NULL */);

/* ---- exact k-nearest-neighbour graphs: each row's k most similar other rows ------------------------------------------------------ */
/* gsim_db_knn: for every row i of [row_begin, row_end) of a single-shard, unfolded handle with N rows, its k most similar OTHER rows
 * (no counterpart in the reference).  Unlike a threshold graph (gsim_db_neighbors) the output is bounded by N x k whatever the data
 * looks like.  The result is a gsim_graph: gsim_graph_shape / _copy / _destroy work on it, gsim_graph_get_stats reports the call's
 * totals (fold launches, their time in tile_ms, entries in pairs), gsim_graph_get_knn_stats the details; gsim_graph_get_join_stats
 * returns GSIM_ERR_INVALID for it.
 * THE RESULT RULE:
 *   - list i - row_begin is exactly the hits of gsim_db_search(query = row i, k + 1, cutoff, metric, alpha, beta) with the hit whose
 *     row is i removed, cut to the first k.  Written out: it holds rows j != i with score(query = row i, row j) >= cutoff, where the
 *     score is bit for bit what gsim_db_search returns for that pair (a = popc(row i), b = popc(row j)); its order is (score
 *     descending, row ascending); the boundary tie group keeps its lowest rows; it is shorter than k when fewer rows qualify;
 *   - NaN (0 / 0) is never >= cutoff: an all-zero row has an empty list and is in nobody's list.  Duplicates of row i are listed at
 *     1.0, row i itself never is;
 *   - cutoff must be in (0, 1], as for neighbours and joins.  The smallest positive float means "every row with a non-zero score": a
 *     row that shares no bit with row i is never a neighbour;
 *   - metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite alpha >= 0, beta >= 0 -- asymmetric included, as in
 *     gsim_db_join: the owner row i is the query and every (i, j) is computed from i's side, so no symmetry is needed;
 *   - rows of up to 4096 bits; 1 <= k <= GSIM_KNN_MAX_K;
 *   - indices = row + the handle's row base (as gsim_hit.row); indptr has row_end - row_begin + 1 entries;
 *   - the output is byte-identical from run to run and does not depend on how the work is cut into launches
 *     (GSIM_KNN_LAUNCH_PAIRS, read once per handle).  Pieces of a table (ranges), concatenated, give the full call's
 *     lists -- and ranges are how a large table is done in pieces: the call allocates about (row_end - row_begin) x k x 8 bytes for
 *     the lists plus a few words per owner row, at most as much again for the compacted CSR while it is copied out, and -- as
 *     gsim_db_neighbors -- 4 bytes per TABLE row (popcounts) and a zero-padded copy of the table where its rows are not 128, 256,
 *     512, 1024, 2048 or 4096 bits wide.  All of it is freed by the call.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / out, k == 0 or k > GSIM_KNN_MAX_K, cutoff outside (0, 1] or NaN,
 * unknown metric, Tversky alpha / beta negative or not finite, row_begin > row_end or row_end past the count, rows wider than 4096
 * bits, a table of 2^32 rows or more.  *out is cleared on failure.  GSIM_ERR_STATE: a table not on a GPU, a multi-shard handle, a
 * folded table.  GSIM_ERR_NOMEM: the call's device memory cannot be had; nothing is truncated, nothing leaked.  row_begin == row_end
 * gives an empty graph (indptr = {0}) and GSIM_OK; N == 1 gives one empty list.
 * Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found (a gsim_db_search
 * before and after returns identical bytes; back-off counters, lanes and slots untouched).  Tables from gsim_db_generate and
 * gsim_db_attach_device_rows work; no host copy is needed.  The work is (row_end - row_begin) x N pair scores, cut into launches of a
 * bounded length; owner rows are spread over the device 256 to a workgroup and every workgroup walks all N candidate rows itself, so a
 * range of a few hundred rows against a very long table uses a small part of the device (its columns are not split over workgroups;
 * for such a range gsim_db_knn_join with left == db and GSIM_KNN_EXCLUDE_SELF, which splits them and returns the same bytes, or
 * gsim_db_search with the rows as queries at k + 1, is the faster route -- DESIGN.md sections 15 and 23 have the crossover). */
#define GSIM_KNN_MAX_K 128u
typedef struct {
    uint64_t rows;      /* owner rows of the call (row_end - row_begin)                                  */
    uint64_t launches;  /* launches of the fold kernel                                                   */
    uint64_t pairs;     /* owner x candidate pairs scored                                                */
    uint64_t inserts;   /* list insertions made (the kernel's slow path)                                 */
    uint64_t entries;   /* entries listed (nnz)                                                          */
    double kernel_ms;   /* HIP events on the handle's stream around all fold launches                    */
    double csr_ms;      /* offsets + compaction on the device                                            */
    double d2h_ms;      /* CSR into host memory                                                          */
    double wall_ms;     /* the whole call, host clock                                                    */
    double clock_mhz;   /* shader clock the fold kernel ran at (as gsim_graph_stats.clock_mhz)           */
} gsim_knn_stats;
int gsim_db_knn(gsim_db* db, uint32_t k, float cutoff, int metric, float alpha, float beta,
                uint64_t row_begin, uint64_t row_end, gsim_graph** out);
int gsim_graph_get_knn_stats(const gsim_graph* g, gsim_knn_stats* out); /* GSIM_ERR_INVALID for any other graph */

/* ---- exact k-nearest-neighbour joins: each left row's k most similar rows of the table -------------------------------------------- */
/* gsim_db_knn_join / gsim_db_knn_queries: for each of nl LEFT rows -- the rows [lrow_begin, lrow_end) of a handle `left` resident on
 * the same device (left == db is allowed), or the nq fingerprints at `queries` (host memory, nq x fp_bits / 32 words) -- its k most
 * similar rows of the table `db` (chemfp's knearest_tanimoto_search_arena; the nearest purchasable analogues of every virtual compound,
 * the nearest training-set neighbours of every test compound).  No counterpart in the reference.  The output is bounded by nl x k
 * whatever the data looks like.  The result is a gsim_graph of its own kind: gsim_graph_shape / _copy / _destroy work on it,
 * gsim_graph_get_stats reports the call's totals (fold + merge launches, their time in tile_ms, entries in pairs),
 * gsim_graph_get_knn_join_stats the details; gsim_graph_get_join_stats and gsim_graph_get_knn_stats return GSIM_ERR_INVALID for it.
 * THE RESULT RULE:
 *   - list i is indexed by left row - lrow_begin, or by position in `queries`, and is exactly the hits of gsim_db_search(query = left
 *     row i, k, cutoff, metric, alpha, beta) on `db`: the same rows, the same score bits (a = popc(left row), b = popc(table row)),
 *     the same order (score descending, row ascending); the boundary tie group keeps its lowest rows; it is shorter than k when fewer
 *     rows qualify;
 *   - NaN (0 / 0) is never >= cutoff: an all-zero left row has an empty list, an all-zero table row is in nobody's list;
 *   - no pair is excluded by default.  left == db is allowed: every non-zero row's list then starts at 1.0 with itself or a
 *     lower-numbered duplicate.  With GSIM_KNN_EXCLUDE_SELF (only with left == db) the pair (left row i, table row i) is left out, by
 *     row identity: the result is gsim_db_knn's rule and equals its output on the same range byte for byte;
 *   - cutoff must be in (0, 1]; the smallest positive float means "every row with a non-zero score";
 *   - metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite alpha >= 0, beta >= 0 -- asymmetric included: every pair
 *     is computed from the left row's side;
 *   - rows of up to 4096 bits; 1 <= k <= GSIM_KNN_MAX_K;
 *   - indices = table row + the TABLE handle's row base; the left handle's base plays no part; indptr has nl + 1 entries;
 *   - the output is byte-identical from run to run and does not depend on how the work is cut into launches or into column segments
 *     (GSIM_KNN_JOIN_LAUNCH_PAIRS, GSIM_KNN_JOIN_SEGMENTS, read once per handle, the table's).  Ranges of left rows,
 *     concatenated, give the full call's lists -- ranges are how a large left side is done in pieces.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / left / out (NULL queries with nq > 0), k == 0 or k > GSIM_KNN_MAX_K,
 * cutoff outside (0, 1] or NaN, unknown metric, Tversky alpha / beta negative or not finite, unknown flag bits, GSIM_KNN_EXCLUDE_SELF
 * with left != db, lrow_begin > lrow_end or lrow_end past the left handle's count, handles of different fp_bits, rows wider than 4096
 * bits, nl >= 2^32, a table of 2^32 rows or more.  *out is cleared on every failure.  GSIM_ERR_STATE: either handle multi-shard, folded
 * or not on a GPU; handles on different devices.  GSIM_ERR_NOMEM: the call's device memory cannot be had; nothing is truncated, nothing
 * leaked.  nl == 0 gives an empty graph (indptr = {0}) and GSIM_OK.
 * Execution: on the table handle's stream under the one-call-at-a-time rule (of both handles); the search state of both is left as it
 * was found (a gsim_db_search before and after returns identical bytes).  Tables from gsim_db_generate and gsim_db_attach_device_rows
 * work on either side; no host copy is needed.  The work is nl x N pair scores.  Left rows are spread over the device 256 to a
 * workgroup, and where those workgroups alone are fewer than two per compute unit the table's rows are cut into S contiguous segments
 * (S = ceil(2 x CUs / owner tiles), at most the table's tiles of 256 rows) that separate workgroups fold into a partial list per
 * (left row, segment); one more kernel merges an owner's S partial lists into its first k, exactly.  The call allocates nl x S x k x 8
 * bytes for the partial lists -- under that rule less than 2 x (2 x CUs) x 256 x k x 8 bytes, 256 MiB at k = 128 on 256 CUs -- plus,
 * for S > 1, nl x k x 8 for the merged lists, a few words per left row, at most nl x k x 8 again for the compacted CSR while it is
 * copied out, and, as gsim_db_knn, 4 bytes per TABLE row (popcounts) and zero-padded copies of both sides where the rows are not 128,
 * 256, 512, 1024, 2048 or 4096 bits wide.  All of it is freed by the call.
 * Against gsim_db_search with the left rows as queries, 256 per call (the same lists), measured on 1 M x 1024-bit rows (DESIGN.md
 * section 23): at the smallest cutoff the join is 6 to 10 times faster at k = 8, 3 to 8 times at k = 32, and at k = 128 from 0.9 times
 * as fast (512 left rows: every segment fills a list of its own) to 4 to 5 times faster (4096); at a cutoff that few rows reach (0.5
 * there) gsim_db_search, which filters on the cutoff before it scores, is 2.4 to 2.9 times FASTER than the join, whose time is then
 * the bare fold of nl x N pairs. */
#define GSIM_KNN_EXCLUDE_SELF 1u   /* only with left == db: the pair (left row i, table row i) is not listed */
typedef struct {
    uint64_t left_rows;       /* left rows of the call (nl)                                                     */
    uint64_t table_rows;      /* table rows (N)                                                                 */
    uint64_t segments;        /* column segments the table was cut into (S)                                     */
    uint64_t fold_launches;   /* launches of the fold kernel                                                    */
    uint64_t merge_launches;  /* launches of the merge kernel (0 when S == 1)                                   */
    uint64_t pairs;           /* left x table pairs scored (nl x N)                                             */
    uint64_t inserts;         /* list insertions made (the fold kernel's slow path)                             */
    uint64_t partial_entries; /* entries held by the partial lists, before the merge                            */
    uint64_t entries;         /* entries listed (nnz), after the merge                                          */
    double kernel_ms;         /* HIP events on the table handle's stream around all fold launches               */
    double merge_ms;          /* ... around the merge                                                           */
    double csr_ms;            /* offsets + compaction on the device                                             */
    double d2h_ms;            /* CSR into host memory                                                           */
    double wall_ms;           /* the whole call, host clock                                                     */
    double clock_mhz;         /* shader clock the fold kernel ran at (as gsim_graph_stats.clock_mhz)            */
} gsim_knn_join_stats;
int gsim_db_knn_join(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint32_t k, float cutoff,
                     int metric, float alpha, float beta, uint32_t flags, gsim_graph** out);
int gsim_db_knn_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, uint32_t k, float cutoff,
                        int metric, float alpha, float beta, gsim_graph** out);
int gsim_graph_get_knn_join_stats(const gsim_graph* g, gsim_knn_join_stats* out); /* GSIM_ERR_INVALID for any other graph */

/* ---- similarity histograms and hit counts: how many table rows score in each bin, per left row ------------------------------------ */
/* gsim_db_histogram_queries / gsim_db_histogram: for each of nl LEFT rows -- the nq fingerprints at `queries` (host memory, nq x
 * fp_bits / 32 words), or the rows [lrow_begin, lrow_end) of a handle `left` resident on the same device (left == db is allowed) --
 * the histogram of its scores against ALL N rows of the table `db`, over the bins that `edges` cut (chemfp's count_tanimoto_hits at
 * several thresholds in one pass; the sizes of a gsim_db_join / gsim_db_neighbors result before it is made; the similarity
 * distribution of one library against another).  No counterpart in the reference.  The output is nl x (nedges + 1) counters whatever
 * the data looks like.
 * THE RESULT RULE:
 *   - pair score: s(i, j) is bit for bit the `score` gsim_db_search returns for query = left row i against table row j
 *     (a = popc(left row), b = popc(table row)), as in gsim_db_join;
 *   - metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite alpha >= 0, beta >= 0 -- asymmetric included: every pair
 *     is computed from the left row's side, so no symmetry is needed;
 *   - edges[0 .. nedges) are finite, strictly ascending, edges[0] > 0; 1 <= nedges <= GSIM_HIST_MAX_EDGES.  Edges above 1 are legal
 *     (no score reaches them: their bins stay empty);
 *   - bin(s) = the number of edges e with s >= e, compared in f32: bin 0 is "below edges[0]", bin nedges "at or above the last edge".
 *     NaN (0 / 0) and 0.0 both land in bin 0, consistent with "NaN is never >= cutoff" everywhere else;
 *   - hist[i * (nedges + 1) + b] = the number of table rows j, of all N, with bin(s(i, j)) == b.  Row i of hist sums to N (to N - 1
 *     with GSIM_HIST_EXCLUDE_SELF), and hist[i][b + 1] + ... + hist[i][nedges] is exactly `approx` of gsim_db_search(query = left
 *     row i, cutoff = edges[b]) and exactly the length of list i of gsim_db_join* at that cutoff;
 *   - total[b] = the sum over the left rows of hist[i][b], in uint64.  At least one of hist and total must be non-NULL; only what is
 *     asked for is copied to the host;
 *   - no pair is excluded by default: left == db counts the self pair (1.0 for a non-zero row: the last bin whose edge is <= 1; NaN
 *     for an all-zero row: bin 0).  GSIM_HIST_EXCLUDE_SELF (only with left == db) leaves out the pair (left row i, table row i), by
 *     row identity.  The row base of either handle plays no part: nothing returned names a row;
 *   - the output is integer: byte-identical from run to run, independent of the route (GSIM_HIST_STREAM_MAX_ROWS) and of how the
 *     work is cut into launches (GSIM_HIST_LAUNCH_PAIRS; both read once per handle, the table's).  Ranges of left rows
 *     concatenate to the full call's hist, and their totals add up to its total -- ranges are how a left side too large for the
 *     call's nl x (nedges + 1) x 8 bytes of device counters is done.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / left (NULL queries with nq > 0), unknown metric, Tversky alpha / beta
 * negative or not finite, NULL edges, nedges == 0 or > GSIM_HIST_MAX_EDGES, an edge that is not finite, not above its predecessor or
 * <= 0, both outputs NULL, unknown flag bits, GSIM_HIST_EXCLUDE_SELF with left != db, nl >= 2^32, a table of 2^32 rows or more,
 * lrow_begin > lrow_end or lrow_end past the left handle's count, handles of different fp_bits, rows wider than 4096 bits.
 * GSIM_ERR_STATE: either handle multi-shard, folded or not on a GPU; handles on different devices.  GSIM_ERR_NOMEM: the call's device
 * memory cannot be had; nothing leaked.  nl == 0: GSIM_OK, total zeroed, hist untouched.
 * Execution: on the table handle's stream under the one-call-at-a-time rule (of both handles); the search state of both is left as
 * it was found (a gsim_db_search before and after returns identical bytes).  Calls of at most GSIM_HIST_STREAM_MAX_ROWS left rows
 * stream the table once per left row; larger ones run an owner-tile kernel (256 left rows to a workgroup, the table's rows split over
 * workgroups as well) that needs, as gsim_db_knn, 4 bytes per TABLE row (popcounts) and zero-padded copies of both sides where the rows
 * are not 128, 256, 512, 1024, 2048 or 4096 bits wide.  All of it, and the nl x (nedges + 1) x 8 bytes of counters, is freed by the
 * call.  Tables from gsim_db_generate and gsim_db_attach_device_rows work on either side; no host copy is needed. */
#define GSIM_HIST_MAX_EDGES 128u
#define GSIM_HIST_EXCLUDE_SELF 1u   /* only with left == db: the pair (left row i, table row i) is not counted */
typedef struct {
    uint64_t left_rows;       /* left rows of the call                                                                          */
    uint64_t rows_streamed;   /* ... taken by the streaming route (one pass over the table each)                                */
    uint64_t rows_tiled;      /* ... taken by the owner-tile route                                                              */
    uint64_t stream_launches; /* launches of the streaming kernel (a pass over a long table is cut into bounded launches)       */
    uint64_t tile_launches;   /* launches of the owner-tile kernel                                                              */
    uint64_t pairs;           /* pairs counted = sum of every returned histogram                                                */
    double stream_ms;         /* HIP events on the table handle's stream: all streaming launches                                */
    double tile_ms;           /* ... all owner-tile launches                                                                    */
    double reduce_ms;         /* the totals, on the device                                                                      */
    double d2h_ms;            /* counters into host memory                                                                      */
    double wall_ms;           /* the whole call, host clock                                                                     */
    double clock_mhz;         /* tile route: shader clock the kernel ran at (as gsim_graph_stats.clock_mhz); 0 when streaming   */
} gsim_hist_stats;
int gsim_db_histogram_queries(gsim_db* db, const uint32_t* queries, uint64_t nq,
                              const float* edges, uint32_t nedges, int metric, float alpha, float beta,
                              uint64_t* hist /* nq x (nedges+1), or NULL */, uint64_t* total /* nedges+1, or NULL */,
                              gsim_hist_stats* stats /* or NULL */);
int gsim_db_histogram(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end,
                      const float* edges, uint32_t nedges, int metric, float alpha, float beta, uint32_t flags,
                      uint64_t* hist, uint64_t* total, gsim_hist_stats* stats);

/* ---- dense similarity matrices: every score of a block of left rows against a range of table rows -------------------------------- */
/* gsim_db_scores / gsim_db_scores_queries / gsim_db_scores_device: the matrix S[i, j] = score(left row i, table row rrow_begin + j)
 * for nl LEFT rows -- the rows [lrow_begin, lrow_end) of a handle `left` resident on the same device (left == db is allowed), or the
 * nq fingerprints at `queries` (host memory, nq x fp_bits / 32 words) -- against the nr = rrow_end - rrow_begin rows
 * [rrow_begin, rrow_end) of the table `db` (RDKit's BulkTanimotoSimilarity, chemfp's arena-by-arena calls; the input of kernel models,
 * MDS / t-SNE / UMAP, scipy linkage, library-against-library heat maps).  No counterpart in the reference.  The intersection counts
 * are a 0/1 matrix product and run on the matrix cores; nothing is filtered, sorted or indexed: the position says which pair it is.
 * THE RESULT RULE:
 *   - out[i * ld + j] is the score of left row i against table row rrow_begin + j, with a = popc(left row), b = popc(table row): bit
 *     for bit what gsim_db_search(query = left row i, k = N, cutoff = 0) returns as that row's `score`, i.e. the reference's one f32
 *     divide followed by "NaN is never >= cutoff".  Hence a 0 / 0 pair is 0.0f, never NaN; nothing is negative; nothing exceeds 1.0;
 *   - metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite alpha >= 0, beta >= 0 -- asymmetric included: every pair
 *     is computed from the left row's side (alpha weighs the left row's own bits), as in the joins and histograms;
 *   - only the nl x nr entries are written: the columns nr ... ld - 1 of every row are left as they were found, in host and in
 *     device memory;
 *   - no pair is excluded: with left == db the diagonal is 1.0 (0.0 for an all-zero row).  The row base of either handle plays no
 *     part: nothing returned names a row;
 *   - blocks concatenate: any cut of the left range and of the table range into pieces gives exactly the slices of the whole matrix
 *     -- that is how a matrix larger than memory is made;
 *   - the output is byte-identical from run to run and does not depend on how the call is cut into launches
 *     (GSIM_SCORES_LAUNCH_PAIRS) or staging slabs (GSIM_SCORES_STAGE_BYTES; both read once per handle, the table's).
 * GSIM_ERR_INVALID, checked before any device state: NULL db / left (NULL queries with nq > 0), NULL out / d_out when nl * nr > 0,
 * unknown metric, Tversky alpha / beta negative or not finite, ld < nr, a range with begin past end or end past its handle's count,
 * nl or nr >= 2^32, handles of different fp_bits, rows wider than 4096 bits.  GSIM_ERR_STATE: either handle multi-shard, folded or
 * not on a GPU; handles on different devices.  GSIM_ERR_NOMEM: the call's device memory cannot be had; nothing leaked.  nl == 0 or
 * nr == 0: GSIM_OK, out untouched.
 * Execution: on the table handle's stream under the one-call-at-a-time rule (of both handles); every call returns with that stream
 * idle and every temporary freed -- gsim_db_scores_device may be followed at once by work on any stream that reads d_out; the
 * search state of both handles is left as it was found.  Device memory of a call: 4 bytes per left and per table row of the call
 * (popcounts), zero-padded copies of both sides where the rows are not a multiple of 256 bits wide, and, for the two host-output
 * calls, one staging slab of whole left rows of at most GSIM_SCORES_STAGE_BYTES (default 256 MiB; at least one row), computed and
 * copied out slab by slab.  gsim_db_scores_device writes straight into d_out, memory of the table's device.  Tables from
 * gsim_db_generate and gsim_db_attach_device_rows work on either side; no host copy is needed. */
typedef struct {
    uint64_t left_rows, right_rows;  /* nl, nr of the call                                                   */
    uint64_t launches;               /* launches of the matrix kernel                                        */
    uint64_t slabs;                  /* host output: device staging slabs copied out (0 for the device call) */
    uint64_t pairs;                  /* nl * nr                                                              */
    double prepare_ms;               /* popcounts and zero-padded copies                                     */
    double kernel_ms;                /* HIP events on the table handle's stream: all matrix launches         */
    double d2h_ms;                   /* host output only                                                     */
    double wall_ms;
    double clock_mhz;                /* as gsim_graph_stats.clock_mhz                                        */
} gsim_scores_stats;

int gsim_db_scores(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end,
                   uint64_t rrow_begin, uint64_t rrow_end, int metric, float alpha, float beta,
                   float* out /* host, nl rows of ld floats */, uint64_t ld, gsim_scores_stats* stats /* or NULL */);
int gsim_db_scores_queries(gsim_db* db, const uint32_t* queries, uint64_t nq,
                           uint64_t rrow_begin, uint64_t rrow_end, int metric, float alpha, float beta,
                           float* out, uint64_t ld, gsim_scores_stats* stats);
int gsim_db_scores_device(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end,
                          uint64_t rrow_begin, uint64_t rrow_end, int metric, float alpha, float beta,
                          void* d_out /* memory of the table's device */, uint64_t ld, gsim_scores_stats* stats);

/* ---- single-linkage clustering: the connected components of the threshold graph -------------------------------------------------- */
/* gsim_db_components clusters a single-shard, unfolded handle with N rows by single linkage: the connected components of the graph
 * "score >= cutoff", at up to GSIM_COMPONENTS_MAX_LEVELS cutoffs in ONE pass over the pairs (a single-linkage dendrogram cut at those
 * levels; leakage-free train / test splits, analog series, de-duplication at 1.0; no counterpart in the reference).  None of the graph
 * is stored: every kept pair feeds a union-find forest in device memory, and the answer is N labels per level.
 * THE RULE:
 *   - pair score: score(i, j) is bit for bit the `score` gsim_db_search returns for query = row i against row j; NaN (0 / 0) is never
 *     >= a cutoff: an all-zero row is a singleton at every level, non-zero duplicates join at 1.0.  Metrics: GSIM_METRIC_TANIMOTO, and
 *     GSIM_METRIC_TVERSKY with alpha == beta, finite and >= 0 (gsim_db_neighbors' metrics: symmetric bit for bit, for the reason given
 *     there);
 *   - cutoffs: cutoffs[0] < cutoffs[1] < ..., each in (0, 1], 1 <= nlevels <= GSIM_COMPONENTS_MAX_LEVELS; level 0 is the loosest;
 *   - the partition at level l: the connected components of the graph on the N rows whose edges are the pairs i != j with
 *     score(i, j) >= cutoffs[l];
 *   - numbering: the components of a level are numbered 0, 1, ... in ascending order of their smallest row;
 *   - outputs: component_of[l * N + i] is the number of row i's component at level l; ncomponents[l] their count; first_row[l * N + c]
 *     (or NULL) component c's smallest row plus the handle's row base; sizes[l * N + c] (or NULL) its member count.  The entries at and
 *     after ncomponents[l] of a first_row / sizes stripe are left untouched.
 * Consequences: level l + 1 refines level l; a single-level call and the matching stripe of a multi-level call are byte-identical; the
 * output is byte-identical from run to run and does not depend on how the pass is cut into launches (GSIM_COMPONENTS_LAUNCH_PAIRS,
 * read once per handle); the partition at level l equals gsim_components applied to gsim_db_neighbors(cutoffs[l])'s
 * CSR.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / cutoffs / component_of / ncomponents, nlevels outside [1, 8], a cutoff
 * outside (0, 1] or NaN, cutoffs not strictly ascending, an unknown metric, asymmetric weights or weights that are negative or not
 * finite, rows wider than 4096 bits, N >= 2^32.  N == 0: GSIM_OK, every ncomponents[l] = 0.  GSIM_ERR_STATE: a table not on a GPU, a
 * multi-shard handle, a folded table.  GSIM_ERR_NOMEM as elsewhere, nothing leaked.
 * Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found.  Device memory of the
 * call, allocated and freed by it: 4 B x N x nlevels for the forests, as much for each of component_of / first_row / sizes asked for,
 * 4 B x N for popcounts, the zero-padded copy of the rows where their width is not 128, 256, ... 4096 bits (as the neighbour lists),
 * and 8 B x N of label scratch plus the scan's. */
#define GSIM_COMPONENTS_MAX_LEVELS 8u
typedef struct {
    uint64_t rows;       /* N                                                                                                  */
    uint64_t levels;     /* nlevels                                                                                            */
    uint64_t launches;   /* launches of the tile kernel (each followed by one of the flatten kernel)                           */
    uint64_t pairs;      /* pairs scored: N (N - 1) / 2                                                                        */
    uint64_t kept;       /* pairs with score >= cutoffs[0]                                                                     */
    uint64_t unions;     /* successful hooks = sum over levels of (N - ncomponents[l])                                         */
    uint64_t cas_failed; /* diagnostic, NOT reproducible: compare-and-swaps that lost a race                                   */
    double kernel_ms;    /* HIP events on the handle's stream: all tile and flatten launches                                   */
    double label_ms;     /* numbering, component_of, first_row and sizes, on the device                                        */
    double d2h_ms;       /* outputs to the host                                                                                */
    double wall_ms;      /* the whole call, host clock                                                                         */
    double clock_mhz;    /* as gsim_graph_stats.clock_mhz                                                                      */
} gsim_components_stats;
int gsim_db_components(gsim_db* db, const float* cutoffs, uint32_t nlevels, int metric, float alpha, float beta,
                       uint32_t* component_of /* nlevels x N */, uint32_t* ncomponents /* nlevels */,
                       uint32_t* first_row /* nlevels x N, or NULL */, uint32_t* sizes /* nlevels x N, or NULL */,
                       gsim_components_stats* stats /* or NULL */);
/* The same rule on a symmetric CSR graph (host code, no device; gsim_butina's companion): the connected components of the graph,
 * numbered in ascending order of their smallest row.  component_of[nrows]; first_row / sizes (or NULL): capacity nrows, the first
 * *ncomponents entries written, rows without any row base.  Self edges and repeated edges are harmless.  GSIM_ERR_INVALID for a
 * malformed graph (gsim_butina's checks); nrows == 0 is legal. */
int gsim_components(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows,
                    uint32_t* component_of, uint32_t* first_row /* or NULL */, uint32_t* sizes /* or NULL */, uint64_t* ncomponents);

/* ---- exact single-linkage dendrograms: the maximum-similarity spanning forest ---------------------------------------------------- */
/* gsim_db_mst returns the single-linkage dendrogram of a single-shard, unfolded handle with N rows as its maximum-similarity spanning
 * forest: at most N - 1 edges, from which every cut (gsim_mst_cut), the merge tree (gsim_mst_linkage), HDBSCAN-style stability (gsim_mst_hdbscan) and
 * "cut where the gap is largest" follow without another pass over the pairs (no counterpart in the reference).  Built by Boruvka
 * rounds on the device; none of the graph is stored: memory is O(N).
 * THE RULE:
 *   - table and metrics: N < 2^32 rows of at most 4096 bits; gsim_db_components' metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY
 *     with alpha == beta, finite and >= 0 (symmetric bit for bit).  cutoff in (0, 1]; the smallest positive float means "every pair
 *     that shares a bit";
 *   - score: score(i, j) is bit for bit the `score` gsim_db_search returns; NaN (0 / 0) is never >= cutoff: an all-zero row is isolated;
 *   - edges: the pairs a < b with score(a, b) >= cutoff, in the strict total ORDER E: (score descending, a ascending, b ascending);
 *   - result: the spanning forest Kruskal builds when it takes the edges in order E and keeps an edge iff its ends are not yet
 *     connected.  E is total, so this forest is unique; it is also exactly what Boruvka finds when every component takes its E-first
 *     outgoing edge;
 *   - output: *nedges = N - (the number of components at `cutoff`); edges[0 .. *nedges) with a < b, the handle's row base added to
 *     both, sorted in order E.  The output is byte-identical from run to run and does not depend on how the work is cut into launches
 *     (GSIM_MST_LAUNCH_PAIRS, read once per handle).
 * Consequence: for any t >= cutoff, the edges with score >= t connect exactly the components of gsim_db_components at t (gsim_mst_cut
 * gives its labels byte for byte), and gsim_db_mst equals gsim_mst applied to gsim_db_neighbors(cutoff)'s CSR.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / nedges, NULL edges with N > 1, a cutoff outside (0, 1] or NaN, an unknown
 * metric, asymmetric weights or weights that are negative or not finite, rows wider than 4096 bits, N >= 2^32.  N == 0: GSIM_OK,
 * *nedges = 0.  GSIM_ERR_STATE: a table not on a GPU, a multi-shard handle, a folded table (N == 1 on a resident table: GSIM_OK, no
 * edges); more than ceil(log2 N) + 1 rounds or an edge count that differs from N minus the final component count (neither can happen).
 * GSIM_ERR_NOMEM as elsewhere, nothing leaked.
 * Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found.  The host waits for
 * one small read per round.  Device memory of the call, allocated and freed by it: 60 B x N (component ids and links, the owner list and its flags, 8 B
 * per row of held edge, the per-component picks, which the sort reuses, and the edges twice: as keys and as the 12-byte output), 4 B x N for popcounts, the zero-padded copy
 * of the rows where their width is not 128, 256, ... 4096 bits, and the select's and the sort's scratch. */
#define GSIM_MST_MAX_ROUNDS 33u /* ceil(log2 N) + 1 for N < 2^32 */
typedef struct {
    uint32_t a, b; /* a < b, row base added */
    float score;
} gsim_mst_edge;
typedef struct {
    uint64_t rows;       /* N                                                                                                     */
    uint64_t rounds;     /* Boruvka rounds that added edges                                                                       */
    uint64_t scans;      /* rounds whose owners were scanned: `rounds`, plus one when a last scan had to find that nothing is left */
    uint64_t launches;   /* launches of the fold kernel                                                                           */
    uint64_t pairs;      /* owner x candidate pairs handed to the fold kernel: N x the sum of scan_owners, the last scan included */
    uint64_t owner_rows; /* the sum over the `rounds` of their owner list's length (round 1: N); without the list: rounds x N     */
    uint64_t edges;      /* *nedges                                                                                               */
    double kernel_ms;    /* HIP events on the handle's stream: all fold launches                                                  */
    double round_ms;     /* ... the rounds' bookkeeping                                                                           */
    double sort_ms;      /* ... the component count and the edges' sort                                                           */
    double d2h_ms;       /* edges to the host                                                                                     */
    double wall_ms;      /* the whole call, host clock                                                                            */
    double clock_mhz;    /* as gsim_graph_stats.clock_mhz                                                                         */
    uint64_t scan_owners[GSIM_MST_MAX_ROUNDS];  /* per scan: owner rows                                                           */
    double scan_kernel_ms[GSIM_MST_MAX_ROUNDS]; /* per scan: its fold launches                                                    */
} gsim_mst_stats;
int gsim_db_mst(gsim_db* db, float cutoff, int metric, float alpha, float beta,
                gsim_mst_edge* edges /* capacity N - 1 */, uint64_t* nedges, gsim_mst_stats* stats /* or NULL */);
/* The same rule on a symmetric scored CSR graph (host code, no device; gsim_components' companion), e.g. gsim_db_neighbors' output: plain
 * Kruskal in order E over the pairs the CSR lists (under either row or both; self edges and repeated pairs are harmless).  edges:
 * capacity nrows - 1, rows without any row base.  GSIM_ERR_INVALID for a malformed graph (gsim_components' checks) or a NaN score;
 * nrows == 0 is legal. */
int gsim_mst(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows,
             gsim_mst_edge* edges, uint64_t* nedges);
/* The dendrogram of a forest in order E (rows without any row base): merges[m] joins the clusters holding edges[m].a and edges[m].b at
 * edges[m].score.  Cluster ids: a row is its own index, merge m creates id nrows + m (scipy's linkage numbering); `left` is the cluster
 * holding the smaller smallest row, `size` the new cluster's row count.  GSIM_ERR_INVALID: NULL arguments, nedges >= nrows (nedges > 0),
 * an edge with a >= b or b >= nrows or a NaN score, a score above its predecessor's, an edge whose ends are already connected. */
typedef struct {
    uint32_t left, right;
    float score;
    uint32_t size;
} gsim_mst_merge;
int gsim_mst_linkage(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows, gsim_mst_merge* merges /* nedges */);
/* The labels at any t: the connected components of the edges with score >= t, numbered in ascending order of their smallest row --
 * gsim_components' output contract (component_of[nrows]; first_row / sizes or NULL: capacity nrows, *ncomponents entries written).  The
 * edges may come in any order.  GSIM_ERR_INVALID: NULL arguments, an edge with b >= nrows or a >= b, a NaN t. */
int gsim_mst_cut(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows, float t,
                 uint32_t* component_of, uint32_t* first_row /* or NULL */, uint32_t* sizes /* or NULL */, uint64_t* ncomponents);

/* ---- DBSCAN density clustering ---------------------------------------------------------------------------------------------------- */
/* gsim_db_dbscan clusters a single-shard, unfolded handle with N rows by density (DBSCAN: Ester, Kriegel, Sander, Xu, KDD 1996; no
 * counterpart in the reference): the one clustering here that names noise, and the standard remedy where single linkage chains through
 * sparse bridges.  None of the graph "score >= cutoff" is stored: two passes over the pairs, the first counts every row's neighbours,
 * the second unites the dense rows in a union-find forest in device memory and attaches the others.  Memory is O(N).
 * THE RULE:
 *   - score: score(i, j) is bit for bit the `score` gsim_db_search returns; NaN (0 / 0) is never >= cutoff.  Metrics: gsim_db_components'
 *     -- GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with alpha == beta, finite and >= 0 (symmetric bit for bit).  cutoff in (0, 1];
 *     rows of at most 4096 bits, N < 2^32;
 *   - degree: degree(i) is the number of rows j != i with score(i, j) >= cutoff;
 *   - core: row i is a core iff degree(i) + 1 >= min_pts -- the row counts itself (scikit-learn's min_samples).  min_pts >= 1;
 *     min_pts == 1 makes every row a core, all-zero rows included;
 *   - clusters: the connected components of the graph on the CORE rows whose edges are the pairs with score >= cutoff, numbered 0, 1,
 *     ... in ascending order of their smallest core row;
 *   - border: a non-core row with at least one core neighbour is a border row and joins the cluster of its ANCHOR: the core neighbour
 *     with the highest score, among equal scores the smallest row -- the order gsim_db_mst's kernel encodes as (score bits << 32) | ~row.
 *     Textbook DBSCAN leaves this to the visit order; here it is fixed, so the output is a function of the table;
 *   - noise: every other row; label_of = GSIM_DBSCAN_NOISE;
 *   - outputs: label_of[N] the cluster number or GSIM_DBSCAN_NOISE (no row base); *nclusters their count; degree[N] (or NULL) the
 *     degrees; anchor[N] (or NULL) -- a core: its own row, a border row: its anchor, both plus the handle's row base, noise:
 *     GSIM_DBSCAN_NOISE; first_row[c] (or NULL) cluster c's smallest core row plus the row base; sizes[c] (or NULL) its cores plus its
 *     border rows.  The first *nclusters entries of first_row and sizes are written, the rest are left untouched.
 * Consequences: the output is byte-identical from run to run and does not depend on how the passes are cut into launches
 * (GSIM_DBSCAN_LAUNCH_PAIRS, read once per handle); with min_pts == 1, label_of, first_row and sizes equal
 * gsim_db_components' at that cutoff byte for byte; the result equals gsim_dbscan applied to gsim_db_neighbors(cutoff)'s CSR; restricted
 * to the core rows, the partition is the one gsim_components gives on the core-induced subgraph.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / label_of / nclusters, a cutoff outside (0, 1] or NaN, min_pts == 0, an
 * unknown metric, asymmetric weights or weights that are negative or not finite, rows wider than 4096 bits, N >= 2^32.  N == 0:
 * GSIM_OK, *nclusters = 0.  GSIM_ERR_STATE: a table not on a GPU, a multi-shard handle, a folded table; degrees that do not add up to
 * twice the kept pairs, hooks other than cores - clusters, or cores + borders + noise other than N (none can happen).  GSIM_ERR_NOMEM as
 * elsewhere, nothing leaked.
 * Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found.  Device memory of the
 * call, allocated and freed by it: 28 B x N (4 B of degree, 4 B of forest, 8 B of anchor key, 4 B of label_of and 8 B of label
 * scratch per row), 4 B x N more for each of anchor / first_row / sizes asked for, 4 B x N for popcounts, the zero-padded copy of the
 * rows where their width is not 128, 256, ... 4096 bits (as the neighbour lists), and the scan's scratch. */
#define GSIM_DBSCAN_NOISE 0xFFFFFFFFu
typedef struct {
    uint64_t rows;           /* N                                                                                              */
    uint64_t launches_count; /* launches of the degree pass's tile kernel                                                      */
    uint64_t launches_link;  /* launches of the link pass's tile kernel (each followed by one of the flatten kernel)           */
    uint64_t pairs;          /* pairs scored by EACH pass: N (N - 1) / 2                                                       */
    uint64_t kept;           /* pairs with score >= cutoff, counted in the degree pass: the sum of the degrees is twice this   */
    uint64_t cores;          /* rows with degree + 1 >= min_pts                                                                */
    uint64_t borders;        /* non-core rows with a core neighbour                                                            */
    uint64_t noise;          /* the others: cores + borders + noise = N                                                        */
    uint64_t clusters;       /* *nclusters                                                                                     */
    uint64_t unions;         /* successful hooks = cores - clusters                                                            */
    uint64_t cas_failed;     /* diagnostic, NOT reproducible: compare-and-swaps that lost a race                               */
    double count_ms;         /* HIP events on the handle's stream: the degree pass                                             */
    double link_ms;          /* ... the link pass, its flatten launches included                                               */
    double label_ms;         /* ... numbering, label_of, anchor, first_row and sizes, on the device                            */
    double d2h_ms;           /* outputs to the host                                                                            */
    double wall_ms;          /* the whole call, host clock                                                                     */
    double clock_mhz;        /* as gsim_graph_stats.clock_mhz, over the launches of both passes                                */
} gsim_dbscan_stats;
int gsim_db_dbscan(gsim_db* db, float cutoff, uint32_t min_pts, int metric, float alpha, float beta,
                   uint32_t* label_of /* N */, uint32_t* nclusters, uint32_t* degree /* N, or NULL */, uint32_t* anchor /* N, or NULL */,
                   uint32_t* first_row /* N, or NULL */, uint32_t* sizes /* N, or NULL */, gsim_dbscan_stats* stats /* or NULL */);
/* The same rule on a symmetric scored CSR graph (host code, no device; gsim_components' and gsim_mst's companion), e.g.
 * gsim_db_neighbors' output: degree(i) is the length of row i's list, self edges not counted; a core's own row, a border row's anchor
 * and first_row carry no row base.  label_of / anchor (or NULL): nrows; first_row / sizes (or NULL): capacity nrows, the first
 * *nclusters entries written.  GSIM_ERR_INVALID for a malformed graph (gsim_components' checks), a NaN score or min_pts == 0;
 * nrows == 0 is legal. */
int gsim_dbscan(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows, uint32_t min_pts,
                uint32_t* label_of, uint32_t* anchor /* or NULL */, uint32_t* first_row /* or NULL */, uint32_t* sizes /* or NULL */,
                uint64_t* nclusters);

/* ---- HDBSCAN: core scores, mutual-reachability forests, the condensed tree and the selection of clusters ------------------------- */
/* Hierarchical density clustering (HDBSCAN: Campello, Moulavi, Sander, PAKDD 2013; Campello, Moulavi, Zimek, Sander, TKDD 2015; no
 * counterpart in the reference) of a single-shard, unfolded handle with N rows: DBSCAN at every cutoff at once, and the clusters that
 * persist over the longest range of levels picked from that hierarchy.  Its O(N^2) part is one k-nearest-neighbour fold (the core
 * scores) and gsim_db_mst's Boruvka scans with another value per pair; none of the graph is stored, memory is O(N).  The level of the
 * hierarchy is the similarity itself: the textbook's density 1 / distance is infinite for duplicates, a similarity of 1.0 is not.
 * THE RULE:
 *   - preconditions: gsim_db_mst's.  N < 2^32 rows of at most 4096 bits; GSIM_METRIC_TANIMOTO, or GSIM_METRIC_TVERSKY with alpha ==
 *     beta, finite and >= 0; cutoff in (0, 1]; score(i, j) is bit for bit the `score` gsim_db_search returns, NaN (0 / 0) is never >=
 *     cutoff.  min_pts counts the row itself, as in gsim_db_dbscan: 1 <= min_pts <= GSIM_KNN_MAX_K + 1;
 *   - core score: for min_pts >= 2, core(i) is the score of the LAST entry of row i's list in gsim_db_knn(k = min_pts - 1, cutoff, ...)
 *     where that list is full (min_pts - 1 entries); otherwise core(i) = 0.0f: the row is not dense at any level >= cutoff.  For
 *     min_pts == 1, core(i) = 1.0f for every row, all-zero rows included.  Consequence: for every t >= cutoff, core(i) >= t iff row i
 *     is a core of gsim_db_dbscan(t, min_pts);
 *   - mutual-reachability score: m(i, j) = min(score(i, j), core(i), core(j)).  The pair is an edge iff score(i, j) >= cutoff and
 *     m(i, j) >= cutoff;
 *   - forest (gsim_db_mreach_mst): gsim_db_mst's rule with m in place of the score.  The pairs a < b that are edges, in the strict
 *     total ORDER E: (m descending, a ascending, b ascending); Kruskal takes them in that order and keeps an edge iff its ends are not
 *     yet connected.  Output: the kept edges in order E, the handle's row base added to a and b, `score` = m.  Ties are the normal
 *     case here -- every edge that a row's own core score caps carries that value -- and order E is what makes the forest unique.
 * Consequences: (1) with min_pts == 1 the edges equal gsim_db_mst's byte for byte; (2) for every t >= cutoff, gsim_mst_cut(edges, t)
 * restricted to the rows with core >= t is the partition gsim_db_dbscan(t, min_pts) gives on its core rows (DBSCAN*: border rows are
 * noise), and every other row is a singleton of the cut; (3) the result equals gsim_mreach_mst applied to gsim_db_neighbors(cutoff)'s
 * CSR; (4) the output is byte-identical from run to run and does not depend on how the passes are cut into launches: the scans read
 * GSIM_MST_LAUNCH_PAIRS and the core pass reads GSIM_KNN_LAUNCH_PAIRS (read once per handle).
 *
 * THE CONDENSED TREE AND THE SELECTION (gsim_mst_hdbscan: host code on any forest in order E, gsim_db_mst's output included; rows
 * without any row base).  Inputs: the edges, nrows, `floor` <= every edge score (the cutoff of the call that made the forest),
 * min_cluster_size >= 2, flags.
 *   - equal scores are ONE event, so nothing depends on the order of tied merges.  For each distinct edge score s, a NODE AT s is a
 *     connected component of {edges with score >= s} that contains an edge of score exactly s; its children are the maximal components
 *     of {edges with score > s} inside it: nodes, or single rows;
 *   - every tree of the forest with at least min_cluster_size rows starts a ROOT CLUSTER, born at `floor`, at the tree's top node;
 *     the rows of smaller trees are noise;
 *   - a cluster C born at b walks down from its node.  At a node of level s: the rows of the children smaller than min_cluster_size
 *     leave C at s.  With no other ("large") child, C ends.  With exactly one, C continues as that child.  With two or more, C ends at
 *     s and each large child is a new cluster born at s, with parent C; the rows of those children leave C at s;
 *   - stability(C) = the sum, over the rows in C at its birth, of (the level at which the row left C - b), in double.  It is summed
 *     as (number of rows that leave at a node) x (double(s) - double(b)): every term is >= 0, one term per node on C's way down;
 *   - selection GSIM_HDBSCAN_EOM (0, "excess of mass"), bottom-up: a cluster without child clusters is selected and S^ = its stability.
 *     Otherwise let sub = the sum of S^ over its child clusters: if stability(C) >= sub, C is selected, every descendant is deselected
 *     and S^ = stability(C) -- equality selects the parent --, else S^ = sub.  GSIM_HDBSCAN_LEAF (1): exactly the clusters without child
 *     clusters are selected.  GSIM_HDBSCAN_NO_ROOTS (flag bit 2, with either): a root cluster that has child clusters is never selected;
 *   - the selected clusters are numbered 0, 1, ... in ascending order of their smallest row.  A row carries the number of the selected
 *     cluster it was in at that cluster's birth, else GSIM_HDBSCAN_NOISE;
 *   - outputs: label_of[nrows]; *nclusters; leave[nrows] (or NULL): the level at which the row left the last cluster it was in, 0.0f
 *     if it was in none; first_row / sizes / birth / stability (each or NULL; capacity nrows, the first *nclusters entries written, the
 *     rest left untouched): the selected cluster's smallest row, its rows at birth, its birth level and its stability.
 * GSIM_ERR_INVALID: NULL edges with nedges > 0, NULL label_of with nrows > 0, NULL nclusters, gsim_mst_linkage's edge checks (a >= b,
 * b >= nrows, a NaN score, nedges >= nrows, a score above its predecessor's, an edge whose ends are already connected), a floor above
 * an edge score or NaN, min_cluster_size < 2, unknown flags.  nrows == 0 is legal.
 *
 * gsim_db_core_scores writes core[N] (useful on its own: the similarity of the k-th neighbour is the usual local-density and outlier
 * score).  Its gsim_knn_stats (or NULL) describe the core pass: `entries` is the number of rows with core >= cutoff, `csr_ms` the tail
 * kernel that reads the lists' last entries; no CSR is built and no list is copied to the host.
 * gsim_db_mreach_mst writes the forest and, where core is not NULL, core[N].
 * gsim_db_hdbscan is gsim_db_mreach_mst followed by gsim_mst_hdbscan with floor = cutoff, in one call: label_of without row base (as
 * gsim_db_dbscan), first_row with the handle's row base added.
 * Errors of the three device calls: GSIM_ERR_INVALID, GSIM_ERR_STATE and GSIM_ERR_NOMEM exactly as gsim_db_mst, plus GSIM_ERR_INVALID
 * for min_pts == 0 or min_pts > GSIM_KNN_MAX_K + 1, NULL core (gsim_db_core_scores, N > 0), NULL label_of (N > 0) / nclusters,
 * min_cluster_size < 2 and unknown flags (gsim_db_hdbscan).  N == 0: GSIM_OK.  N == 1 on a resident table: no edge, core 0.0f (1.0f
 * for min_pts == 1).
 * Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found.  Device memory of a
 * forest call, allocated and freed by it: gsim_db_mst's, plus 4 B x N for the core scores, plus -- during the core pass only, freed
 * before the first scan -- gsim_db_knn's lists, N x (min_pts - 1) x 8 B, and 4 B x N of list lengths.  Lists built in pieces are not
 * offered: where N x (min_pts - 1) x 8 B does not fit, the call returns GSIM_ERR_NOMEM. */
#define GSIM_HDBSCAN_NOISE 0xFFFFFFFFu
#define GSIM_HDBSCAN_EOM 0u
#define GSIM_HDBSCAN_LEAF 1u
#define GSIM_HDBSCAN_NO_ROOTS 2u
typedef struct {
    gsim_mst_stats mst;       /* the scans, the bookkeeping, the sort and the copy of the edges, as gsim_db_mst reports them     */
    uint64_t core_launches;   /* the core pass: launches of the k-NN fold kernel (0 for min_pts == 1)                            */
    uint64_t core_inserts;    /* ... list insertions made                                                                       */
    uint64_t core_rows;       /* rows with core >= cutoff                                                                       */
    double core_kernel_ms;    /* ... HIP events around its fold launches                                                        */
    double core_tail_ms;      /* ... the kernel that reads the lists' last entries                                              */
} gsim_mreach_stats;
typedef struct {
    gsim_mreach_stats forest; /* gsim_db_mreach_mst's part                                                                      */
    uint64_t clusters;        /* *nclusters                                                                                     */
    uint64_t noise;           /* rows labelled GSIM_HDBSCAN_NOISE                                                               */
    double select_ms;         /* the condensed tree and the selection, host clock                                               */
    double wall_ms;           /* the whole call, host clock                                                                     */
} gsim_hdbscan_stats;
int gsim_db_core_scores(gsim_db* db, uint32_t min_pts, float cutoff, int metric, float alpha, float beta,
                        float* core /* N */, gsim_knn_stats* stats /* or NULL */);
int gsim_db_mreach_mst(gsim_db* db, uint32_t min_pts, float cutoff, int metric, float alpha, float beta,
                       gsim_mst_edge* edges /* capacity N - 1 */, uint64_t* nedges, float* core /* N, or NULL */,
                       gsim_mreach_stats* stats /* or NULL */);
int gsim_db_hdbscan(gsim_db* db, uint32_t min_pts, uint32_t min_cluster_size, float cutoff, int metric, float alpha, float beta,
                    uint32_t flags, uint32_t* label_of /* N */, uint64_t* nclusters, float* leave /* N, or NULL */,
                    uint32_t* first_row /* N, or NULL */, uint32_t* sizes /* N, or NULL */, float* birth /* N, or NULL */,
                    double* stability /* N, or NULL */, gsim_hdbscan_stats* stats /* or NULL */);
/* The forest's rule on a symmetric scored CSR graph (host code, no device; gsim_mst's companion), e.g. gsim_db_neighbors' output:
 * core(i) is the (min_pts - 1)-th largest score of row i's list, self edges not counted (a pair listed twice counts twice), 0.0f where
 * the list is shorter, 1.0f for min_pts == 1; a listed pair is an edge iff both rows' lists are long enough; then Kruskal in order E
 * over min(score, core, core).  edges: capacity nrows - 1, rows without any row base; core: nrows, or NULL.  GSIM_ERR_INVALID:
 * gsim_mst's checks, or min_pts == 0; nrows == 0 is legal. */
int gsim_mreach_mst(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows, uint32_t min_pts,
                    gsim_mst_edge* edges, uint64_t* nedges, float* core /* or NULL */);
int gsim_mst_hdbscan(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows, float floor, uint32_t min_cluster_size, uint32_t flags,
                     uint32_t* label_of /* nrows */, uint64_t* nclusters, float* leave /* nrows, or NULL */,
                     uint32_t* first_row /* or NULL */, uint32_t* sizes /* or NULL */, float* birth /* or NULL */,
                     double* stability /* or NULL */);

/* ---- per-bit column counts and iSIM library statistics ---------------------------------------------------------------------------- */
/* The column-wise questions about a table, a row range or a cluster (a gsim_rowset): how often is each bit set, how tight is the set,
 * which row is its medoid, which rows are outliers.  All of them are O(N) once the per-bit column counts c_k of the set's n rows are
 * known (iSIM: Lopez-Perez, Kim, Miranda-Quintana, "iSIM: instant similarity", Digital Discovery 2024): the sum over all pairs i < j
 * of |x_i AND x_j| is sum_k c_k (c_k - 1) / 2, that of |x_i XOR x_j| is sum_k c_k (n - c_k).  No counterpart in the reference.
 * WHAT THE STATISTIC IS: a ratio of sums over all pairs.  It is not the mean of the pairwise Tanimoto scores; gsim_db_histogram
 * remains the way to the true distribution of the scores.
 *
 * gsim_db_bit_counts, THE RESULT RULE:
 *   - the counted rows are the rows of [row_begin, row_end) that are in `rs`, or all of them when rs is NULL; the indices carry no
 *     row base, as in gsim_db_knn;
 *   - counts[k], k < fp_bits, is the number of counted rows whose bit k is set; bit k is bit k % 32 of word k / 32 of the row (the
 *     row-set bitmap's convention); *counted (or NULL) is the number of counted rows;
 *   - an empty range or an empty set gives GSIM_OK with zeros;
 *   - the output is integer: byte-identical from run to run, independent of the route a row set takes (streamed under its bitmap or
 *     gathered through its list: gsim_db_search_rows' rule and its GSIM_SUBSET_GATHER_MAX_PERMILLE, applied to the set's size and the
 *     table's) and of how the pass is cut into launches (GSIM_PROFILE_LAUNCH_ROWS, read once per handle, 0 = automatic;
 *     INTEGRATION.md).  The counts of ranges that partition a range add up to its counts.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / counts, row_begin > row_end or row_end past the count, a row set made
 * for another handle, a table of 2^32 rows or more, rows wider than 4096 bits.  GSIM_ERR_STATE: a table not on a GPU (N == 0: GSIM_OK
 * with zeros), a multi-shard handle, a folded table, a table that changed after the row set was made.  GSIM_ERR_NOMEM: the call's
 * device memory cannot be had; nothing leaked.
 * Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found (a gsim_db_search
 * before and after returns identical bytes).  One streaming pass over the rows read; device memory of the call: fp_bits + 1 64-bit
 * counters, freed by the call.  Tables from gsim_db_generate and gsim_db_attach_device_rows work; no host copy is needed.
 *
 * gsim_db_overlap_sums, THE RESULT RULE:
 *   - sums[i], i < row_end - row_begin, is the sum of weights[k] over the bits k set in row row_begin + i, exact in uint64 (at most
 *     4096 x (2^32 - 1)); popc[i] (or NULL) is that row's popcount.  weights has fp_bits entries, in host memory;
 *   - with weights = the counts of a set (they fit in 32 bits: N < 2^32) sums[i] is S_i, the row's total overlap with the set,
 *     sum over the set's rows j of |x_i AND x_j| -- row i itself included when it is a member.  The row need not belong to the set:
 *     "how close is every row to this cluster's profile" is the same call;
 *   - the output is integer: byte-identical from run to run, independent of the kernel that computes it (rows of whole 256-bit groups
 *     go through the matrix cores, every other width through a VALU kernel) and of GSIM_PROFILE_LAUNCH_ROWS.  Ranges concatenate.
 * GSIM_ERR_INVALID: NULL db / weights, NULL sums with a non-empty range, a bad range, N >= 2^32, rows wider than 4096 bits.
 * GSIM_ERR_STATE, GSIM_ERR_NOMEM and execution as gsim_db_bit_counts; device memory of the call: 8 bytes per row of the range (12 with
 * popc) and the weights' 32 bit planes (fp_bits x 4 bytes), freed by the call -- ranges are how a table too long for that is done. */
#define GSIM_PROFILE_STREAMED 1u /* gsim_profile_stats.route: the rows were streamed (under the set's bitmap, if any)   */
#define GSIM_PROFILE_GATHERED 2u /* ... gathered through the set's list                                                  */
#define GSIM_PROFILE_MATRIX 4u   /* ... gsim_db_overlap_sums ran on the matrix cores                                     */
#define GSIM_PROFILE_VALU 8u     /* ... on the VALU kernel                                                               */
typedef struct {
    uint64_t rows_read;    /* rows the kernels visited: the range, or the set's rows in it on the gather route         */
    uint64_t rows_counted; /* bit counts: *counted; overlap sums: the rows of the range                                 */
    uint64_t launches;     /* kernel launches of the pass                                                               */
    uint64_t route;        /* GSIM_PROFILE_* bits; 0 when nothing ran                                                   */
    double kernel_ms;      /* HIP events on the handle's stream around the pass                                         */
    double d2h_ms;         /* outputs to the host                                                                       */
    double wall_ms;        /* the whole call, host clock                                                                */
} gsim_profile_stats;
int gsim_db_bit_counts(gsim_db* db, const gsim_rowset* rs /* or NULL */, uint64_t row_begin, uint64_t row_end,
                       uint64_t* counts /* fp_bits */, uint64_t* counted /* or NULL */, gsim_profile_stats* stats /* or NULL */);
int gsim_db_overlap_sums(gsim_db* db, const uint32_t* weights /* fp_bits */, uint64_t row_begin, uint64_t row_end,
                         uint64_t* sums /* row_end - row_begin */, uint32_t* popc /* or NULL, same length */,
                         gsim_profile_stats* stats /* or NULL */);
/* The iSIM index of a set of n rows from its column counts (host code, no device, no handle).  With a = sum c_k (c_k - 1) / 2 (pairs
 * of ones), d = sum (n - c_k) (n - c_k - 1) / 2 (pairs of zeros) and dis = sum c_k (n - c_k) (mismatches), all exact integers (128-bit:
 * they pass 2^64 at n near 2^32 and 4096 bits), the index is numerator / denominator as listed below: each converted to double with
 * one round-to-nearest conversion, then one double divide.  A zero denominator gives 0.0 (n < 2; a Tanimoto index over all-zero rows),
 * as "NaN counts as 0.0" elsewhere.  Once more: a ratio of sums over all pairs, not the mean of the pairwise scores.
 * GSIM_ERR_INVALID: NULL counts / value, fp_bits == 0, a count above n, n >= 2^32, an unknown index. */
#define GSIM_ISIM_TANIMOTO 0        /* a / (a + dis)           */
#define GSIM_ISIM_RUSSELL_RAO 1     /* a / (a + d + dis)       */
#define GSIM_ISIM_SIMPLE_MATCHING 2 /* (a + d) / (a + d + dis) */
int gsim_isim(const uint64_t* counts, uint32_t fp_bits, uint64_t n, int index, double* value);
/* Complementary similarity: out[i], i < m, is the same index of the n - 1 rows left when row i is removed from the set; the lowest
 * value marks the medoid, the highest the outliers.  Row i is a MEMBER of the counted set, given by sums[i] (gsim_db_overlap_sums with
 * weights = counts) and popc[i].  With C = sum c_k: a_i = a - sums[i] + popc[i], dis_i = dis - n popc[i] - C + 2 sums[i],
 * d_i = d - (fp_bits - popc[i]) (n - 1) + (C - sums[i]); the same conversions and divide.  GSIM_ERR_INVALID: gsim_isim's, NULL sums /
 * popc / out with m > 0, popc[i] > fp_bits, m > 0 with n == 0, and a row whose sums / popc no member of the set can have (one of the
 * three terms would be negative). */
int gsim_isim_complement(const uint64_t* counts, uint32_t fp_bits, uint64_t n, int index,
                         const uint64_t* sums, const uint32_t* popc, uint64_t m, double* out /* m */);

/* ---- centroid clustering: nearest-centre assignment, per-label column counts, k-means --------------------------------------------- */
/* "Give me K clusters of this library": the two passes of Lloyd's iteration on fingerprints and the loop over them.  The centroid of
 * a cluster is its majority vote per bit (BitBIRCH's floor(sum / n + 0.5)).  No counterpart in the reference.  The labels that
 * gsim_db_leader, gsim_db_maxmin (`nearest`) and gsim_butina return are valid inputs of gsim_db_label_counts as they are.
 *
 * gsim_db_assign, THE RESULT RULE:
 *   - S[c, i] is what gsim_db_scores_queries(db, centres, m, row_begin, row_end, ...) returns: the centre is the left side (alpha
 *     weighs the centre's own bits), the reference's one f32 divide, 0 / 0 is 0.0f;
 *   - label[i], i < row_end - row_begin, is the centre c with the greatest f32 S[c, i]; among centres whose f32 scores are equal the
 *     LOWEST index wins.  The rule is stated on the rounded f32 scores, not on the exact fractions: two different c / den that round
 *     to the same float tie, and the lower index wins whatever a cross-multiplied comparison would say;
 *   - score[i] (or NULL) is that S[label[i], i], bit for bit;
 *   - an all-zero row (every score 0.0) gets label 0 and score 0.0;
 *   - metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite alpha >= 0, beta >= 0, asymmetric included;
 *   - ranges concatenate; the row base plays no part (indices as in gsim_db_bit_counts); the output is byte-identical from run to run
 *     and does not depend on how the call is cut into launches (GSIM_ASSIGN_LAUNCH_PAIRS, read once per handle).
 * GSIM_ERR_INVALID, checked before any device state: NULL db, m == 0 or m > GSIM_ASSIGN_MAX_CENTRES, NULL centres / label with a
 * non-empty range, row_begin > row_end or row_end past the count, an unknown metric, Tversky alpha / beta negative or not finite, a
 * table of 2^32 rows or more, rows wider than 4096 bits.  GSIM_ERR_STATE: a multi-shard handle, a folded table, a table not on a GPU.
 * GSIM_ERR_NOMEM: the call's device memory cannot be had; nothing leaked.  An empty range: GSIM_OK, outputs untouched.
 * Execution: as gsim_db_scores -- on the handle's stream under the one-call-at-a-time rule, every temporary freed, the search state
 * left as it was found.  Device memory of a call: the centres (zero-padded to whole 256-bit groups) and their popcounts, 8 bytes per
 * row of the range (labels and scores), and per SLAB of at most 2^20 rows 4 bytes a row (popcounts) plus, for rows that are not whole
 * 256-bit groups, the slab's zero-padded copy: never a padded copy of the table. */
#define GSIM_ASSIGN_MAX_CENTRES 65536u
typedef struct {
    uint64_t rows, centres;          /* row_end - row_begin, m                                               */
    uint64_t launches;               /* launches of the assign kernel                                        */
    uint64_t pairs;                  /* m * rows                                                             */
    double prepare_ms;               /* popcounts and zero-padded copies (centres and slabs)                 */
    double kernel_ms;                /* HIP events on the handle's stream: all assign launches               */
    double d2h_ms;                   /* labels and scores to the host                                        */
    double wall_ms;
    double clock_mhz;                /* as gsim_scores_stats.clock_mhz                                       */
} gsim_assign_stats;
int gsim_db_assign(gsim_db* db, const uint32_t* centres /* host, m x fp_bits/32 words */, uint32_t m,
                   uint64_t row_begin, uint64_t row_end, int metric, float alpha, float beta,
                   uint32_t* label /* row_end - row_begin */, float* score /* or NULL, same length */,
                   gsim_assign_stats* stats /* or NULL */);

/* gsim_db_label_counts, THE RESULT RULE (labels[i] is the label of row row_begin + i; host memory):
 *   - counts[l * fp_bits + k], l < nlabels, is the number of rows of the range with label l whose bit k is set (bit k: as
 *     gsim_db_bit_counts); sizes[l] (or NULL) is the number of rows with label l.  A row labelled GSIM_LABEL_NONE is counted nowhere;
 *   - the counters are uint32 (a table has fewer than 2^32 rows; 10^5 labels x 1024 bits are 400 MB, not 800): gsim_isim and
 *     gsim_isim_complement take uint64 counts -- widen a label's row before it goes there;
 *   - row l of counts equals gsim_db_bit_counts over the row set {i : labels[i] == l}; the counts of ranges that partition a range add
 *     up; an empty range gives GSIM_OK with zeros;
 *   - the output is integer: byte-identical from run to run, independent of the way a row's bits are added
 *     and of how the pass is cut into launches (GSIM_LABELS_LAUNCH_ROWS, read once per handle, 0 = automatic).
 * GSIM_ERR_INVALID, checked before any device state: NULL db / counts, nlabels == 0, NULL labels with a non-empty range, a label
 * >= nlabels other than GSIM_LABEL_NONE, row_begin > row_end or row_end past the count, a table of 2^32 rows or more, rows wider than
 * 4096 bits.  GSIM_ERR_STATE and GSIM_ERR_NOMEM: as gsim_db_bit_counts.  Execution: as gsim_db_bit_counts.  Device memory of the
 * call: nlabels x fp_bits 32-bit counters, nlabels + 1 segment starts, 20 bytes per row of the range (labels, sort keys and row
 * numbers before and behind the sort) and the sort's scratch, freed by the call. */
#define GSIM_LABEL_NONE 0xFFFFFFFFu /* == GSIM_LEADER_NONE: the row is counted nowhere */
typedef struct {
    uint64_t rows_read;    /* rows of the range                                                                         */
    uint64_t rows_counted; /* ... whose label is not GSIM_LABEL_NONE                                                    */
    uint64_t labels;       /* nlabels                                                                                   */
    uint64_t launches;     /* launches of the counting kernel                                                           */
    double sort_ms;        /* HIP events: labels to the device, keys, the sort, the segment starts                      */
    double kernel_ms;      /* ... the counting launches                                                                 */
    double d2h_ms;         /* counts to the host                                                                        */
    double wall_ms;        /* the whole call, host clock                                                                */
} gsim_label_stats;
int gsim_db_label_counts(gsim_db* db, const uint32_t* labels /* host, row_end - row_begin */, uint32_t nlabels,
                         uint64_t row_begin, uint64_t row_end,
                         uint32_t* counts /* nlabels x fp_bits */, uint32_t* sizes /* nlabels, or NULL */,
                         gsim_label_stats* stats /* or NULL */);

/* The majority-vote centroids of labelled rows from gsim_db_label_counts' output (host code, no device, no handle): bit k of centre l
 * is set iff 2 * counts[l * fp_bits + k] >= sizes[l] (a tie sets the bit).  A label with sizes[l] == 0 keeps previous[l * words ..],
 * or is all zeros when previous is NULL; words = fp_bits / 32.  GSIM_ERR_INVALID: NULL counts / sizes / centres, nlabels == 0,
 * fp_bits 0 or not a multiple of 32, a count above its label's size. */
int gsim_label_centroids(const uint32_t* counts, const uint32_t* sizes, uint32_t nlabels, uint32_t fp_bits,
                         const uint32_t* previous /* nlabels x words, or NULL */, uint32_t* centres /* nlabels x words */);

/* gsim_db_kmeans, THE RESULT RULE (Lloyd's iteration over the whole table of N rows, m centres):
 *   - C_0 = init.  Iteration t = 0, 1, ...: labels_t = gsim_db_assign(C_t) over [0, N).  Stop if t > 0 and labels_t == labels_(t-1)
 *     (converged), or once t + 1 == max_iter.  Otherwise C_(t+1) = gsim_label_centroids(gsim_db_label_counts(labels_t), previous =
 *     C_t): an empty cluster keeps its centre;
 *   - centres (m x words) are the C_t that the returned label[N] / score[N] (or NULL) were assigned to, so gsim_db_assign(centres)
 *     reproduces them exactly; sizes[m] (or NULL) are the sizes of the returned labels.
 * GSIM_ERR_INVALID: max_iter == 0, NULL init / centres, NULL label with N > 0, and what gsim_db_assign refuses; GSIM_ERR_STATE: as
 * the two calls, and a table without rows; GSIM_ERR_NOMEM: as the two calls.  Execution: as gsim_db_assign; the labels stay on the device between iterations, per iteration
 * only the counts and sizes come down and the centres go up. */
typedef struct {
    uint64_t iterations;   /* assignments made: t + 1 at the stop                                                       */
    uint64_t converged;    /* 1: the last two assignments were equal                                                    */
    uint64_t changed_last; /* rows whose label differed between the last two assignments (N after a single one)        */
    double assign_ms;      /* kernel time of the assignments (prepare + kernel of gsim_assign_stats)                    */
    double counts_ms;      /* ... of the label counts (sort + kernel + d2h of gsim_label_stats)                         */
    double update_ms;      /* host clock: the majority votes and the centres' way up                                    */
    double wall_ms;
} gsim_kmeans_stats;
int gsim_db_kmeans(gsim_db* db, const uint32_t* init /* m x words */, uint32_t m, uint32_t max_iter,
                   int metric, float alpha, float beta,
                   uint32_t* centres /* m x words */, uint32_t* label /* N */, float* score /* or NULL */,
                   uint32_t* sizes /* m, or NULL */, gsim_kmeans_stats* stats /* or NULL */);

/* ---- how good a labelling is, and which row stands for a cluster: score sums by label, silhouettes, exact medoids ----------------- */
/* Every call above that returns labels (gsim_butina, gsim_db_leader, gsim_db_components / gsim_mst_cut, gsim_db_dbscan,
 * gsim_db_hdbscan, gsim_db_kmeans, gsim_db_maxmin's `nearest`) can be judged and given representatives by one all-pairs pass over the
 * labelled rows; neither the score matrix nor a graph is stored.  No counterpart in the reference.
 *
 * gsim_db_label_sums, THE RESULT RULE (labels[i] is the label of row row_begin + i, as in gsim_db_label_counts; host memory):
 *   - a row labelled GSIM_LABEL_NONE is neither an owner nor a candidate: own_q = 0, other_label = GSIM_LABEL_NONE, other_q = 0.
 *     sizes[l] (or NULL) is the number of rows with label l;
 *   - s(i, j) is the reference's one f32 divide with row i as the query side -- alpha weighs i's own bits, exactly as gsim_db_knn
 *     scores an owner against a candidate --, 0 / 0 is 0.0f.  Metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite
 *     alpha >= 0, beta >= 0: every ORDERED pair is scored, so symmetry is not needed;
 *   - q(s) = (uint32) floor(s * 2^31).  The product is exact in f32 (a power of two), the conversion truncates: scores of 2^-8 and
 *     above convert exactly, smaller ones lose less than 2^-31.  Every sum is therefore a sum of INTEGERS: byte-identical from run to
 *     run, independent of the order of addition and of how the call is cut into launches; with fewer than 2^32 rows it stays below 2^63;
 *   - Q[i, l] is the sum of q(s(i, j)) over the rows j of the range with labels[j] == l and j != i; own_q[i] = Q[i, labels[i]];
 *   - other_label[i] is the label l != labels[i] with sizes[l] > 0 of the greatest MEAN Q[i, l] / sizes[l].  Means are compared as
 *     exact fractions (Q1 * n2 against Q2 * n1, 96-bit products), never as rounded doubles; among equal means the LOWEST label wins.
 *     other_q[i] = Q[i, other_label[i]]; when no other label has rows, other_label[i] = GSIM_LABEL_NONE and other_q[i] = 0;
 *   - GSIM_LABEL_SUMS_OWN_ONLY (bit 0 of flags) computes own_q and sizes only: other_label / other_q may be NULL and are not written,
 *     and only the pairs inside a cluster are scored -- the sum over the labels of sizes[l]^2 of them, not n^2.  The medoid route;
 *   - owners and candidates are the rows of the range; the row base plays no part (indices as in gsim_db_bit_counts);
 *   - launch_pairs: a launch of the kernel scores at most this many owner x candidate pairs, and at least one tile of 256 owners
 *     against 256 candidates; 0: priced by the row width, as GSIM_KNN_LAUNCH_PAIRS = 0 is.  The result does not depend on it.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / own_q, NULL other_label / other_q without GSIM_LABEL_SUMS_OWN_ONLY,
 * nlabels == 0, NULL labels with a non-empty range, a label >= nlabels other than GSIM_LABEL_NONE, an unknown flag bit, row_begin >
 * row_end or row_end past the count, an unknown metric, Tversky alpha / beta negative or not finite, a table of 2^32 rows or more, rows
 * wider than 4096 bits.  GSIM_ERR_STATE: a table not on a GPU, a folded table, a multi-shard handle.  GSIM_ERR_NOMEM: the call's
 * device memory cannot be had; nothing leaked.  An empty range: GSIM_OK, sizes zeroed.
 * Execution: on the handle's stream under the one-call-at-a-time rule, every temporary freed, the search state left as it was found.
 * Owner tiles are independent and their candidates are not split over workgroups (as gsim_db_knn): a short range against nothing else
 * has little parallelism.  Device memory of a call, with n_lab labelled rows of the range: their label-sorted copy, zero-padded to WP
 * words (n_lab x WP x 4 bytes; WP = 4, 8, 16, 32, 64 or 128, the first that holds a row), 4 bytes a row of popcounts, the sort's 20 bytes
 * per row of the range and its scratch, nlabels + 1 segment starts, 32 bytes a row of carried state, 20 bytes per row of the range of
 * outputs (8 with GSIM_LABEL_SUMS_OWN_ONLY). */
#define GSIM_LABEL_SUMS_OWN_ONLY 1u
typedef struct {
    uint64_t rows;            /* row_end - row_begin                                                                    */
    uint64_t rows_labelled;   /* ... whose label is not GSIM_LABEL_NONE: n_lab                                          */
    uint64_t labels_nonempty; /* labels with at least one row                                                           */
    uint64_t pairs;           /* ordered pairs scored, i != j: n_lab^2 - n_lab, own-only: the sum of sizes[l]^2 - n_lab */
    uint64_t launches;        /* launches of the fold kernel                                                            */
    double sort_ms;           /* HIP events: labels to the device, keys, the sort, the segment starts                   */
    double gather_ms;         /* ... the sorted copy, its popcounts, the carried state's first values                   */
    double kernel_ms;         /* ... all fold launches                                                                  */
    double d2h_ms;            /* ... the outputs back to row order and to the host                                      */
    double wall_ms;           /* the whole call, host clock                                                             */
    double clock_mhz;         /* as gsim_knn_stats.clock_mhz                                                            */
} gsim_label_sums_stats;
int gsim_db_label_sums(gsim_db* db, const uint32_t* labels /* host, row_end - row_begin */, uint32_t nlabels,
                       uint64_t row_begin, uint64_t row_end, int metric, float alpha, float beta,
                       uint32_t flags, uint64_t launch_pairs /* 0 = automatic */,
                       uint64_t* own_q, uint32_t* other_label, uint64_t* other_q /* each row_end - row_begin */,
                       uint32_t* sizes /* nlabels, or NULL */, gsim_label_sums_stats* stats /* or NULL */);

/* The silhouette of every row on the distance 1 - s, from gsim_db_label_sums' output (host code, no device, no handle).  For a row i
 * with label L, sizes[L] >= 2 and other_label[i] != GSIM_LABEL_NONE, in IEEE doubles, one rounding per operation, in this order:
 *     a = ((double) own_q[i] / (double) (sizes[L] - 1)) * 0x1p-31         the mean score to its own cluster's other rows
 *     b = ((double) other_q[i] / (double) sizes[other_label[i]]) * 0x1p-31  ... to the nearest other cluster
 *     d = 1.0 - fmin(a, b)                                                 max(1 - a, 1 - b)
 *     sil[i] = d > 0 ? (a - b) / d : 0.0
 * (the conversions of integers above 2^53 round to nearest even; the scalings by 2^-31 are exact).  A singleton, a row without
 * another cluster and a GSIM_LABEL_NONE row get 0.0.  label_mean[l] (or NULL) is the sum of sil over label l's rows, added in
 * ascending row order from 0.0, divided by (double) sizes[l]; an empty label gives 0.0.  *mean (or NULL) is the sum over all
 * labelled rows in ascending row order divided by their number; no labelled row gives 0.0.
 * GSIM_ERR_INVALID, nothing written: NULL labels / own_q / other_label / other_q / sizes with n > 0, NULL sizes / sil where they
 * have entries, nlabels == 0, a label >= nlabels other than GSIM_LABEL_NONE, an other_label equal to the row's own label or
 * >= nlabels other than GSIM_LABEL_NONE, an other_label without rows, a sizes[] that disagrees with labels. */
int gsim_label_silhouette(const uint32_t* labels, const uint64_t* own_q, const uint32_t* other_label,
                          const uint64_t* other_q, const uint32_t* sizes, uint64_t n, uint32_t nlabels,
                          double* sil /* n */, double* label_mean /* nlabels, or NULL */, double* mean /* or NULL */);

/* The exact medoid of every label (host code): medoid[l] is the row i < n with labels[i] == l of the greatest own_q[i] -- the row
 * most similar to the rest of its cluster --, the LOWEST row among equals; GSIM_LABEL_NONE for a label without rows.
 * GSIM_ERR_INVALID, nothing written: NULL labels / own_q with n > 0, NULL medoid, nlabels == 0, n >= 2^32, a label >= nlabels other
 * than GSIM_LABEL_NONE. */
int gsim_label_medoids(const uint32_t* labels, const uint64_t* own_q, uint64_t n, uint32_t nlabels,
                       uint32_t* medoid /* nlabels */);

/* ---- label-grouped search: the best hit and the hit count of every cluster ------------------------------------------------------- */
/* A gsim_labelset is a labelling of ONE single-shard, unfolded handle on the device -- the output of gsim_butina, gsim_db_leader,
 * gsim_db_components / gsim_mst_cut, gsim_db_dbscan, gsim_db_hdbscan, gsim_db_kmeans or gsim_db_maxmin's `nearest`, as it is --;
 * gsim_db_search_labels answers, per query and in one pass over the table, "the best hit of every cluster, best clusters first" (the
 * diverse hit list) and "how many hits has each cluster above the cutoff" (the enrichment).  It is gsim_db_search_group transposed:
 * that call reduces over the queries per row, this one over the rows per label.  No counterpart in the reference.
 * gsim_db_search_labels, THE RESULT RULE, per query q (labels[r] is the label of table row r, without the row base):
 *   - pair score: gsim_db_search's -- score = metric(query, row), then score = score >= cutoff ? score : 0, NaN becoming 0;
 *   - a row labelled GSIM_LABEL_NONE is never scored, kept or counted;
 *   - the kept rows are all labelled rows when cutoff <= 0, else the labelled rows with score != 0;
 *   - label_kept[q, l] (or NULL) is the number of kept rows with label l: with cutoff <= 0 that is sizes[l].  rows_kept[q] (or NULL) is
 *     their sum over l; with no GSIM_LABEL_NONE row it equals gsim_db_search's approx;
 *   - label_best[q, l] (or NULL) is the kept row of label l that comes first in (score descending, row ascending) order, as a gsim_hit:
 *     `row` includes the row base, `score`, `common` and `popc_db` are bit for bit what gsim_db_search returns for that row.  A label
 *     without a kept row gets {row = 0xFFFFFFFF, score = 0, common = 0, popc_db = 0};
 *   - approx[q] (or NULL) is the number of labels with at least one kept row;
 *   - hits[q * k ..] are the first min(k, approx[q]) label bests in (score descending, row ascending) order, hit_labels[q * k ..] their
 *     labels, counts[q] their number.  k == 0 is legal and returns no hits; k is the stride, as in gsim_db_search.
 * Identities the rule implies:
 *   - with labels[r] = r the call returns gsim_db_search's hits, counts and approx byte for byte, and hit_labels = row - row_base;
 *   - with one label it returns gsim_db_search at k = 1;
 *   - label_best[q, l] and label_kept[q, l] are the hit and the approx of gsim_db_search_rows at k = 1 on the row set
 *     {r : labels[r] == l}.
 * Metrics: GSIM_METRIC_TANIMOTO, and GSIM_METRIC_TVERSKY with any finite alpha >= 0, beta >= 0 (no streaming filter is involved, so
 * scores above 1 are harmless: the candidate key orders any float).
 * Lifetime: a label set belongs to the handle it was made for, takes 4 bytes per table row of that handle's device memory, is
 * immutable and serves any number of searches; destroy it before its handle.  gsim_labelset_sizes: sizes[l] = rows with label l,
 * *labelled (or NULL) = rows whose label is not GSIM_LABEL_NONE, *nonempty (or NULL) = labels with at least one row.
 * Execution: on the handle's stream under the one-call-at-a-time rule.  Several queries may share a table pass -- an execution detail:
 * every query gets what a call with nq = 1 returns.  Per pass the table of (query, label) entries lives either in every workgroup's LDS
 * (while one query's nlabels x 8 bytes, 12 when rows are counted under a cutoff, fit 144 KiB) or in global memory; the output is
 * byte-identical from run to run and depends on neither the route nor launch_rows.  launch_rows: a scan launch reads at most this
 * many rows, in whole chunks and at least one chunk; 0: sized by the row width and the queries of the pass, as gsim_db_search_group
 * sizes its launches.  There is no environment knob.  The call leaves the search state as it found it: a gsim_db_search before and
 * after returns identical bytes, the back-off counters and the lanes are untouched.  Device memory of a call: the queries are answered
 * in tiles of at most 16 (fewer where 16 x nlabels exceeds 2^27), a tile takes tile x nlabels x 24 bytes, and the ranking nlabels x 8
 * bytes plus the radix sort's scratch (about as much again); every temporary is freed on return.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / out / ls / hits / hit_labels / counts, NULL labels with a non-empty
 * table, NULL queries with nq > 0, nlabels == 0, a label >= nlabels other than GSIM_LABEL_NONE, a label set made for another handle,
 * an unknown metric, Tversky alpha / beta negative or not finite, rows wider than 4096 bits, a table of 2^32 rows or more.  *out is
 * cleared on failure.  GSIM_ERR_STATE: a table not on a GPU, a folded table, a multi-shard handle.  GSIM_ERR_NOMEM: the call's device
 * memory cannot be had; nothing leaked.  nq == 0 and an empty table: GSIM_OK. */
typedef struct gsim_labelset gsim_labelset;
typedef struct {
    uint64_t queries;       /* nq                                                                                     */
    uint64_t labels;        /* nlabels                                                                                */
    uint64_t passes;        /* passes over the table                                                                  */
    uint64_t passes_lds;    /* ... whose (query, label) table lived in the workgroups' LDS                            */
    uint64_t passes_global; /* ... in global memory                                                                   */
    uint64_t launches;      /* kernel launches: the scans', a finish per tile, a sort and an emission per query       */
    double scan_ms;         /* HIP events: all scan launches                                                          */
    double finish_ms;       /* ... the finish, the ranking, the emission                                              */
    double d2h_ms;          /* ... the outputs to the host                                                            */
    double wall_ms;         /* the whole call, host clock                                                             */
} gsim_label_search_stats;
int gsim_labelset_create(gsim_db* db, const uint32_t* labels /* host, one per table row */, uint32_t nlabels, gsim_labelset** out);
int gsim_labelset_sizes(const gsim_labelset* ls, uint32_t* sizes /* nlabels */, uint64_t* labelled /* or NULL */, uint64_t* nonempty /* or NULL */);
int gsim_labelset_destroy(gsim_labelset* ls);
int gsim_db_search_labels(gsim_db* db, const gsim_labelset* ls, const uint32_t* queries, uint32_t nq, uint32_t k,
                          float cutoff, int metric, float alpha, float beta,
                          uint64_t launch_rows /* 0 = automatic */,
                          gsim_hit* hits /* nq x k */, uint32_t* hit_labels /* nq x k */, uint32_t* counts /* nq */,
                          uint64_t* approx /* nq, or NULL */, uint64_t* rows_kept /* nq, or NULL */,
                          gsim_hit* label_best /* nq x nlabels, or NULL */, uint32_t* label_kept /* nq x nlabels, or NULL */,
                          gsim_label_search_stats* stats /* or NULL */);

/* ---- complete- and average-linkage dendrograms ------------------------------------------------------------------------------------ */
/* gsim_db_mst is single linkage, which chains.  gsim_db_linkage builds the two other dendrograms asked for on a few thousand to a few
 * tens of thousands of rows -- cluster representatives from gsim_label_medoids, a hit list, a screening deck --: complete linkage and
 * average linkage (UPGMA), on the dense similarity matrix, which never leaves the device.  No counterpart in the reference.
 * gsim_db_linkage, THE RESULT RULE, on the n = row_end - row_begin rows of a single-shard, unfolded handle, n <= GSIM_LINKAGE_MAX_ROWS:
 *   - linkages: GSIM_LINKAGE_COMPLETE, GSIM_LINKAGE_AVERAGE.  Metrics: those of gsim_db_mst -- GSIM_METRIC_TANIMOTO, or
 *     GSIM_METRIC_TVERSKY with alpha == beta, finite and >= 0;
 *   - leaves: s(i, j) for i < j is the score gsim_db_scores gives with the LOWER row on the left; 0 / 0 is 0.0f.  Every pair has a
 *     score in [0, 1], so the dendrogram is always complete: exactly n - 1 merges (n >= 1);
 *   - the similarity of two clusters, complete linkage: the MINIMUM of s over the pairs between them -- an f32, exact;
 *   - ... average linkage: the exact fraction Q / (|A| |B|), Q the sum of q(s) over the pairs between them, q(s) = (uint32) floor(s *
 *     2^31) as in gsim_db_label_sums.  Means are compared as exact fractions by cross-multiplication in 128 bits, never as rounded
 *     doubles;
 *   - a cluster is identified by its smallest row.  At every step the pair of live clusters (a < b) that comes first in ORDER L =
 *     (similarity descending, a ascending, b ascending) is merged.  L is total, so the dendrogram is unique, ties included;
 *   - merges[m], m = 0 .. n - 2, in the order of execution: a, b the smallest rows of the two clusters, a < b, with row_begin and the
 *     row base added; left, right in scipy's numbering WITHIN the range, as gsim_mst_merge -- leaf i is id i, merge m creates id
 *     n + m, `left` is the cluster of `a`; size the new cluster's rows;
 *     score, complete linkage: the minimum, exact; sum_q = q(score);
 *     score, average linkage: (float) (((double) sum_q / (double) pairs) * 0x1p-31) with pairs = |A| |B|, one rounding per operation;
 *     sum_q = Q, exact.
 * What the rule implies:
 *   - scores never increase along the list (both linkages are reducible: a merged cluster is no closer to a third than the closer of
 *     its halves was);
 *   - the edges (a, b, score) given to gsim_mst_cut(t) (without the row offsets) are the flat clusters at t in gsim_components'
 *     numbering: no cut call of its own is needed;
 *   - the output is byte-identical from run to run and does not depend on launch_steps.
 * Execution: the matrix-core pass of gsim_db_scores fills the matrix; ONE workgroup then runs the nearest-neighbour chain on it (a
 * scan of one matrix row per step), at most launch_steps steps to a launch (0: sized so that a launch stays near 5 ms), and the host
 * puts the n - 1 merges it executed into order L's sequence.  On the handle's stream under the
 * one-call-at-a-time rule, every temporary freed, the search state left as it was found.  Device memory of a call, with n4 = n rounded
 * up to a multiple of 4: complete linkage 4 B x n x n4 (the score matrix itself); average linkage 8 B x n x n4 (the Q matrix) plus one
 * staging slab of f32 scores (GSIM_SCORES_STAGE_BYTES, at least 32 rows); 32 B x n of state (sizes, chain, executed merges); and what
 * the score pass takes: popcounts and, where the width is not 256, 512, ... 4096 bits, the zero-padded copy of the rows.  n = 65 536
 * with average linkage is 32 GiB.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / nmerges, row_begin > row_end or row_end past the count, n above
 * GSIM_LINKAGE_MAX_ROWS, an unknown linkage or metric, Tversky alpha != beta, negative or not finite, rows wider than 4096 bits, NULL
 * merges with n > 1.  n == 0 and n == 1: GSIM_OK, *nmerges = 0.  GSIM_ERR_STATE: a table not on a GPU, a folded table, a multi-shard
 * handle.  GSIM_ERR_NOMEM: the call's device memory cannot be had; nothing leaked. */
#define GSIM_LINKAGE_COMPLETE 0
#define GSIM_LINKAGE_AVERAGE 1
#define GSIM_LINKAGE_MAX_ROWS 65536u
typedef struct {
    uint32_t a, b;        /* smallest row of either cluster, a < b, row_begin and row base added */
    uint32_t left, right; /* scipy numbering within the range, as gsim_mst_merge                 */
    uint32_t size;
    float score;
    uint64_t sum_q;
} gsim_linkage_merge; /* 32 bytes */
typedef struct {
    uint64_t rows;         /* n                                                                                      */
    uint64_t merges;       /* n - 1                                                                                  */
    uint64_t scans;        /* nearest-neighbour scans of the chain: one matrix row each                              */
    uint64_t chain_max;    /* the deepest the chain got                                                              */
    uint64_t launches;     /* launches of the chain kernel                                                           */
    uint64_t launch_steps; /* chain steps to a launch: the argument, or what 0 chose                                 */
    double matrix_ms;      /* host clock, the stream waited for: the score pass and the mirror / widening kernel     */
    double chain_ms;       /* ... all chain launches                                                                 */
    double order_ms;       /* ... the host's replay into order L's sequence                                          */
    double d2h_ms;         /* ... the executed merges to the host                                                    */
    double wall_ms;        /* the whole call                                                                         */
    double clock_mhz;      /* as gsim_knn_stats.clock_mhz, over the chain launches                                   */
} gsim_linkage_stats;
int gsim_db_linkage(gsim_db* db, uint64_t row_begin, uint64_t row_end, int linkage, int metric, float alpha, float beta,
                    uint32_t launch_steps /* 0 = automatic */, gsim_linkage_merge* merges /* n - 1 */, uint64_t* nmerges,
                    gsim_linkage_stats* stats /* or NULL */);
/* The same rule on a matrix in host memory (host code, no device, no handle, no row base; what gsim_mst is to gsim_db_mst): scores
 * holds n rows of ld floats of which only the entries i < j are read (-0.0f is read as 0.0f).  *scans (or NULL) is the number of
 * nearest-neighbour scans the chain took.  GSIM_ERR_INVALID: NULL scores with n > 1, NULL nmerges, NULL merges with n > 1, ld < n,
 * n above GSIM_LINKAGE_MAX_ROWS, an unknown linkage, a NaN or an entry outside [0, 1] in the upper triangle. */
int gsim_linkage(const float* scores /* n rows of ld floats, only i < j read */, uint64_t n, uint64_t ld, int linkage,
                 gsim_linkage_merge* merges /* n - 1 */, uint64_t* nmerges, uint64_t* scans /* or NULL */);

/* ---- Jarvis-Patrick clustering and shared-nearest-neighbour graphs --------------------------------------------------------------- */
/* Jarvis-Patrick clustering (Jarvis & Patrick 1973) joins two rows when they are in each other's nearest-neighbour lists and those
 * lists have enough rows in common; it needs no similarity threshold tuned to the data and works on exactly the lists gsim_db_knn
 * builds.  Its building block, the shared-nearest-neighbour (SNN) count of two rows, is returned by gsim_db_snn for callers that want
 * the SNN graph itself.  No counterpart in the reference.
 * THE RULE, on a single-shard, unfolded handle with N rows:
 *   - lists: L(i) is the set of rows in list i of gsim_db_knn(db, k, cutoff, metric, alpha, beta, 0, N) -- that call's metrics,
 *     asymmetric Tversky included, since every list is taken from its owner's side.  i is never in L(i); an all-zero row has an empty
 *     list and is in nobody's list;
 *   - shared(i, j) = |L(i) & L(j)|.  With GSIM_SNN_CLOSED the lists count their owners (the 1973 paper's convention):
 *     shared(i, j) = |L(i) & L(j)| + [j in L(i)] + [i in L(j)].  mutual(i, j): j in L(i) and i in L(j);
 *   - links: a pair {i, j}, i != j, is a link at level l when it is mutual and shared(i, j) >= kmins[l]; with GSIM_SNN_EITHER "mutual"
 *     is relaxed to "j in L(i) or i in L(j)".  kmins[0] < kmins[1] < ..., 1 <= nlevels <= GSIM_COMPONENTS_MAX_LEVELS, each value in
 *     [0, k], or [0, k + 2] with GSIM_SNN_CLOSED.  kmin = 0 without GSIM_SNN_EITHER is the mutual k-NN graph.  Level 0 is the loosest;
 *   - the partition at level l: the connected components of the graph on the N rows whose edges are the links of level l;
 *   - numbering and outputs: exactly gsim_db_components' -- the clusters of a level are numbered in ascending order of their smallest
 *     row; cluster_of[l * N + i], nclusters[l], first_row[l * N + c] (or NULL; + the handle's row base), sizes[l * N + c] (or NULL);
 *     the entries at and after nclusters[l] of a first_row / sizes stripe are left untouched.
 * Consequences: level l + 1 refines level l; a single-level call and the matching stripe of a multi-level call are byte-identical; the
 * output is byte-identical from run to run and does not depend on GSIM_KNN_LAUNCH_PAIRS (the lists are unique because gsim_db_knn's
 * order is total); gsim_db_jarvis_patrick equals gsim_jarvis_patrick applied to gsim_db_knn's CSR (without a row base), and
 * gsim_db_snn's counts equal gsim_snn's on it.
 * gsim_db_snn returns a gsim_graph whose gsim_graph_shape / _copy bytes are exactly gsim_db_knn's for the whole table, and per entry
 * e = (i, j) of it, through gsim_graph_copy_shared: shared[e] = shared(i, j) | (mutual(i, j) ? GSIM_SNN_MUTUAL_BIT : 0).  Only
 * GSIM_SNN_CLOSED is a flag of this call.  gsim_graph_get_stats and gsim_graph_get_snn_stats answer for it; the k-NN, join and k-NN
 * join accessors return GSIM_ERR_INVALID, as gsim_graph_copy_shared and gsim_graph_get_snn_stats do for every other graph.
 * gsim_db_jarvis_patrick keeps the graph on the device: the fold of gsim_db_knn leaves the lists there (8 B x N x k), one kernel writes
 * each list's rows in ascending order (4 B x N x k), one kernel intersects, for every entry (i, j), the two sorted lists and feeds the
 * links to one union-find forest per level (4 B x N each), and gsim_db_components' labelling numbers the trees (its outputs on the
 * device and 8 B x N of scratch plus the scan's); beside that, what gsim_db_knn takes for popcounts and padded rows.  All of it is
 * freed by the call.
 * The stats: rows, k, entries (of all lists), mutual_entries (entries with the mutual bit: twice the mutual pairs) and links[l]
 * (entries (i, j) with [mutual or GSIM_SNN_EITHER] and shared >= kmins[l]; gsim_db_snn: none) and unions (successful hooks = the sum
 * over the levels of N - nclusters[l]) are reproducible; cas_failed is a diagnostic and is not.
 * GSIM_ERR_INVALID, checked before any device state and in this order: NULL db (and NULL out), gsim_db_knn's checks of k, cutoff and
 * metric, unknown flag bits, NULL kmins / cluster_of / nclusters, nlevels outside [1, 8], kmins not strictly ascending or out of range,
 * rows wider than 4096 bits, N >= 2^32.  GSIM_ERR_STATE as gsim_db_knn.  N == 0: GSIM_OK, nclusters[l] = 0 (an empty graph); N == 1:
 * one singleton.  Execution: on the handle's stream under the one-call-at-a-time rule; the search state is left as it was found. */
#define GSIM_SNN_CLOSED 1u /* the lists count their owners */
#define GSIM_SNN_EITHER 2u /* gsim_db_jarvis_patrick / gsim_jarvis_patrick: one-sided pairs may link too */
#define GSIM_SNN_MUTUAL_BIT 0x80000000u
typedef struct {
    uint64_t rows;           /* N                                                                                   */
    uint64_t k;
    uint64_t entries;        /* entries of all lists (gsim_db_knn's nnz)                                            */
    uint64_t mutual_entries; /* entries (i, j) with i in L(j)                                                       */
    uint64_t links[8];       /* entries meeting level l's condition; [nlevels ..) zero                              */
    uint64_t unions;         /* successful hooks = sum over levels of (N - nclusters[l])                            */
    uint64_t cas_failed;     /* diagnostic, NOT reproducible: compare-and-swaps that lost a race                    */
    uint64_t launches;       /* launches of the fold kernel, as gsim_knn_stats                                      */
    uint64_t pairs;          /* owner x candidate pairs scored                                                      */
    uint64_t inserts;        /* list insertions made                                                                */
    double knn_ms;           /* HIP events on the handle's stream: all fold launches                                */
    double sort_ms;          /* ... the kernel that sorts every list's rows                                         */
    double link_ms;          /* ... the intersection kernel (and the flatten that follows it)                       */
    double label_ms;         /* ... numbering and outputs (gsim_db_snn: offsets and compaction)                     */
    double d2h_ms;           /* outputs to the host                                                                 */
    double wall_ms;          /* the whole call, host clock                                                          */
    double clock_mhz;        /* as gsim_knn_stats.clock_mhz                                                         */
} gsim_snn_stats;
int gsim_db_snn(gsim_db* db, uint32_t k, float cutoff, int metric, float alpha, float beta, uint32_t flags, gsim_graph** out);
int gsim_graph_copy_shared(const gsim_graph* g, uint32_t* shared /* nnz */);
int gsim_graph_get_snn_stats(const gsim_graph* g, gsim_snn_stats* out);
int gsim_db_jarvis_patrick(gsim_db* db, uint32_t k, const uint32_t* kmins, uint32_t nlevels, float cutoff, int metric, float alpha,
                           float beta, uint32_t flags, uint32_t* cluster_of /* nlevels x N */, uint32_t* nclusters /* nlevels */,
                           uint32_t* first_row /* nlevels x N, or NULL */, uint32_t* sizes /* nlevels x N, or NULL */,
                           gsim_snn_stats* stats /* or NULL */);
/* The same rule on any CSR of lists (host code, no device, no handle, no row base): list r is indices[indptr[r] .. indptr[r + 1]), of
 * any length and in any order.  gsim_snn: shared[e] for every entry e, as gsim_graph_copy_shared gives it (flags: GSIM_SNN_CLOSED).
 * gsim_jarvis_patrick: cluster_of [nlevels x nrows], nclusters [nlevels], first_row / sizes (or NULL) [nlevels x nrows], entries at
 * and after nclusters[l] untouched; kmins only has to ascend strictly.  GSIM_ERR_INVALID: NULL arguments, unknown flag bits, nlevels
 * outside [1, 8], kmins not strictly ascending, a malformed graph (gsim_butina's checks), a list that names its own row or names a row
 * twice.  nrows == 0 is legal. */
int gsim_snn(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, uint32_t flags, uint32_t* shared /* nnz */);
int gsim_jarvis_patrick(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, const uint32_t* kmins, uint32_t nlevels,
                        uint32_t flags, uint32_t* cluster_of, uint32_t* first_row /* or NULL */, uint32_t* sizes /* or NULL */,
                        uint32_t* nclusters /* nlevels */);

/* ---- popcount-bounded search: a query reads only the rows whose popcount lets them matter ----------------------------------------- */
/* A query with a bits set and a row with b bits set share at most min(a, b) bits, so their Tanimoto score is at most
 * min(a, b) / max(a, b): at a cutoff of 0.7 only the rows with 0.7 a <= b <= a / 0.7 can pass, and a top-k query needs only the
 * popcounts whose bound reaches the k-th best score (Swamidass and Baldi's bound; chemfp, FPSim2 and Arthor search this way).  A
 * gsim_popindex is the table's rows ordered by popcount; gsim_db_search_bounded answers gsim_db_search's question and reads only a
 * window of that order.  Opt-in: no other call looks at an index.  No counterpart in the reference.
 * The index of a table of N rows: `order` (gsim_popindex_order) is the permutation of the rows sorted by (popcount ascending, row
 * ascending), row base included; first[b] (gsim_popindex_first, b = 0 .. fp_bits + 1) is the number of rows with a popcount below b,
 * so first[fp_bits + 1] = N and the rows with popcount b are order[first[b] .. first[b + 1]).  With GSIM_POPINDEX_ROWS the index also
 * keeps a copy of the rows in that order.
 * The bound: for a query popcount a and a row popcount b,
 *     ub[b] = max over c in [max(0, a + b - fp_bits), min(a, b)] of s(a, b, c),
 * s the f32 score gsim_db_search computes from the three counts, NaN (0 / 0) taken as 0.  The maximum is found by enumerating c, not
 * from a closed form, so it is exact -- f32 roundings included -- for Tanimoto and for Tversky with any alpha and beta: no row with
 * popcount b scores above ub[b], and some pair of fingerprints attains it.  gsim_popcount_bounds computes the same table on the host
 * (no device, no handle; ub holds fp_bits + 1 floats); for Tanimoto ub[b] = (float) min(a, b) / (float) max(a, b), 0 for a = b = 0.
 * gsim_db_search_bounded, THE RESULT RULE: for every query, hits, counts and approx are byte for byte what gsim_db_search returns on
 * the same handle with the same arguments -- whatever the index's flags, the route and the number of stages, from run to run, and for
 * cutoff <= 0 as well (approx = N).  k is the stride of `hits` and k == 0 is legal, as there.
 * Execution (fixed here, so that `stats` can be checked).  Per query, with k clamped to N:
 *   - cutoff window (cutoff > 0): B = {b : ub[b] >= cutoff}; the window is the hull [min B, max B], its rows are
 *     order[first[min B] .. first[max B + 1]).  B empty: zero hits, approx 0, no launch.  cutoff <= 0: the window is the whole order;
 *   - top-k narrowing, when cutoff <= 0 or approx == NULL (the hits of a narrowed scan are exact, its count of rows above the cutoff
 *     is not), k >= 1, the window holds more than T = max(4 k, 4096) rows, and the metric is Tanimoto or Tversky with finite
 *     alpha >= 0, beta >= 0, alpha + beta >= 1 (gsim_db_search_group's condition: scores within [0, 1]).  Stage 1 scans the smallest
 *     hull of the window's buckets, taken in descending ub with ties to the lower b, that holds at least T rows.  It is final when
 *     that hull is the window, or when it returns k hits and every bucket of the window outside it has ub < s_k, the last hit's
 *     score -- strictly: an outside row with an equal score and a lower row number would displace a hit.  Otherwise stage 2 scans,
 *     in full, the hull of {b in the window : ub[b] >= s_k}, or the whole window when stage 1 returned fewer than k hits, and its
 *     result is the answer;
 *   - the route of a scan of n rows: with GSIM_POPINDEX_ROWS the slots of the copy are STREAMED while 4 n <= 3 N; without the copy
 *     the rows are GATHERED through `order` while gsim_db_search_rows would gather a set of n rows (GSIM_SUBSET_GATHER_MAX_PERMILLE).
 *     Past that the query is answered by a PLAIN scan of the whole table (the four-kernel pipeline of the ordinary search), whichever
 *     stage asked.  Both limits are estimates.
 * stats: rows_scanned sums the rows of every scan (N for a plain one), rows_window the cutoff windows; every query is counted once,
 * in queries_plain if a plain scan answered it, else in queries_one_stage or queries_two_stage (a query without narrowing, or with
 * an empty window, is a one-stage query).
 * The call runs on the handle's stream under the one-call-at-a-time rule, answers the queries one after another and leaves the
 * search state as it found it: a gsim_db_search before and after returns identical bytes; the back-off counters, the lanes and the
 * pipeline slots are untouched.  The bound table of a query popcount is computed on the device once per call and popcount.
 * Lifetime: an index belongs to ONE single-shard, unfolded, finalized handle of fewer than 2^32 rows -- made by gsim_db_finalize,
 * gsim_db_generate or gsim_db_attach_device_rows: it is built from the rows on the device --, lives in that handle's device memory
 * (4 bytes per row; with GSIM_POPINDEX_ROWS N x row bytes more; the build takes 4 bytes per row of popcounts -- two 16-bit arrays,
 * before and behind the sort -- and the radix sort's scratch, about 6 bytes per row, besides; both are freed on return), is immutable
 * and serves any number of searches; destroy it before its handle.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / out / ix / first / order / ub / queries / hits / counts, unknown
 * flag bits, a table of 2^32 rows or more, an index made for another handle, an unknown metric; gsim_popcount_bounds: fp_bits not a
 * positive multiple of 32 up to 32768, popc_query above fp_bits.  *out is cleared on failure.  GSIM_ERR_STATE: a table not on a GPU,
 * a multi-shard handle, a folded table, a table that changed after the index was made.  GSIM_ERR_NOMEM as elsewhere. */
typedef struct gsim_popindex gsim_popindex;
#define GSIM_POPINDEX_ROWS 1u  /* also keep a popcount-ordered COPY of the rows (N x row bytes more HBM): windows stream instead of gathering */
typedef struct {
    uint64_t rows_scanned;      /* rows offered to the filter, summed over queries and stages                             */
    uint64_t rows_window;       /* rows of the cutoff window (N when cutoff <= 0), summed over queries                    */
    uint64_t queries_one_stage; /* queries answered by one window scan (or by none: an empty window)                      */
    uint64_t queries_two_stage; /* ... by two                                                                             */
    uint64_t queries_plain;     /* ... by a plain scan of the whole table                                                 */
    uint64_t launches;          /* kernel launches: a bound table per distinct popcount; per scan the scan, the compaction and the select (k > 8192: three for it) */
    double bounds_ms;           /* HIP events around the bound tables and their copies                                    */
    double kernel_ms;           /* ... around every scan and its tail, summed                                             */
    double wall_ms;             /* the whole call, host clock                                                             */
} gsim_popindex_stats;
int gsim_popindex_create(gsim_db* db, uint32_t flags, gsim_popindex** out);
int gsim_popindex_first(const gsim_popindex* ix, uint64_t* first /* fp_bits + 2 */);
int gsim_popindex_order(const gsim_popindex* ix, uint32_t* order /* N entries, row base included */);
int gsim_popindex_destroy(gsim_popindex* ix);
int gsim_popcount_bounds(uint32_t fp_bits, uint32_t popc_query, int metric, float alpha, float beta, float* ub /* fp_bits + 1 */); /* host */
int gsim_db_search_bounded(gsim_db* db, const gsim_popindex* ix, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff,
                           int metric, float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx,
                           gsim_popindex_stats* stats /* or NULL */);

/* ---- exact duplicates and exact-row lookup: a hash table over the rows -------------------------------------------------------------- */
/* Which rows of a table are the same fingerprint, and is this fingerprint in the table and where: O(N) to build and O(1) per lookup
 * with a hash table over the rows, where gsim_db_components at cutoff 1.0 is O(N^2) and a scan at cutoff 1.0 reads the table per
 * query -- and neither finds an all-zero row, whose score is NaN.  Opt-in: no other call looks at an index.  No counterpart in the
 * reference.
 * Two rows are IDENTICAL when all their fp_bits / 32 words are equal.  Nothing else defines the groups: all-zero rows are identical
 * to one another and form an ordinary group.
 * THE RESULT RULE.  gsim_rowhash_groups: first[i] is the lowest-numbered row identical to row i, the handle's row base included;
 * size[i] is the number of rows identical to row i, itself included (either array may be NULL, not both).  stats: rows = N, groups =
 * the number of distinct rows, repeated_groups = the groups of size >= 2, largest_group = the largest size, slots as below,
 * launches = the kernel launches of the build; for N = 0 every count is 0 and no launch is made.  gsim_rowhash_rowset returns the
 * row set {i : first[i] == i + row_base} of the index's handle -- one representative per group, gsim_rowset_count = groups -- or,
 * with GSIM_ROWHASH_REPEATS, its complement: an ordinary gsim_rowset for gsim_db_search_rows, gsim_db_bit_counts and every other
 * consumer, destroyed with gsim_rowset_destroy and independent of the index afterwards.  gsim_rowhash_find: per query, row[q] = the
 * lowest table row identical to query q, row base included, and size[q] (size may be NULL) = the size of that row's group; when no
 * row is identical, row[q] = GSIM_ROW_NONE and size[q] = 0.  gsim_rowhash_find_db: the same for the rows [lrow_begin, lrow_end) of
 * another finalized, single-shard, unfolded handle with the same fp_bits on the same device (the left-handle convention of the
 * joins); `left` may be the index's own handle, and then row[] is first[] of that range.  gsim_duplicates (host, no device, no
 * handle): the same first / size (either or both may be NULL) and *ngroups (or NULL) = the number of distinct rows, on host rows,
 * without a base.  Every output is byte-identical from run to run: none depends on the order in which the rows reached the table.
 * THE HASH.  gsim_row_hash is the library's 64-bit hash of a row of W = fp_bits / 32 words w[0 .. W); the device computes the same
 * values.  All arithmetic is on uint32_t (mod 2^32), >> is a logical shift, rotl16 swaps the halves of a word:
 *     k(i) = (i + 1) * 0x9E3779B9
 *     a(i) = (w[i] ^ k(i)) * 0x85EBCA6B;            a(i) ^= a(i) >> 15;          A = the sum of a(i) over i
 *     b(i) = (rotl16(w[i]) + k(i)) * 0xC2B2AE35;    b(i) ^= b(i) >> 13;          B = the sum of b(i) over i
 *     m1(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 *     m2(x): x ^= x >> 15; x *= 0x2C1B3C6D; x ^= x >> 12; x *= 0x297A2D39; x ^= x >> 15
 *     lo = m1(A ^ m2(B));   hi = m2(B ^ lo);   hash = (uint64_t) hi << 32 | lo
 * A word's contribution depends on its position, the contributions are summed, and one avalanche (a bijection of (A, B)) ends it.
 * The table of N rows has slots(N) = 0 slots for N = 0, else the smallest power of two >= 2 N, at least 1024 (stats.slots); a row's
 * first slot is hash & (slots - 1), and a probe goes on to the next slot, wrapping at the end.  Correctness never rests on the
 * hash: rows are compared word by word, equal hashes only cost probes.
 * Execution: the build streams the table once (launches of at most 32 GiB of rows), every row entering the table by atomic
 * operations on its slot alone -- no workgroup waits for another --, then a second pass gives every row its group's first row and
 * size; a lookup hashes, probes and compares, read-only.  The calls run on the handle's stream under the one-call-at-a-time rule
 * and leave the search state as they found it: a gsim_db_search before and after returns identical bytes.
 * Lifetime: an index belongs to ONE single-shard, unfolded, finalized handle -- made by gsim_db_finalize, gsim_db_generate or
 * gsim_db_attach_device_rows: it is built from the rows on the device --, lives in that handle's device memory (8 bytes per slot,
 * i.e. 16 to 32 bytes per row and at least 8 KiB, plus 8 bytes per row for first and size; N / 8 bytes of host memory for the
 * representatives' bitmap), is immutable and serves any number of lookups; destroy it before its handle.
 * GSIM_ERR_INVALID, checked before any device state: NULL db / out / ix / row / queries with nq > 0, both first and size NULL,
 * unknown flag bits, a table whose last row number with its base would be GSIM_ROW_NONE or beyond, the left handle's errors (NULL,
 * a range past its rows or with its begin past its end, other fp_bits); gsim_row_hash and gsim_duplicates: fp_bits not a positive
 * multiple of 32 up to 32768, NULL rows with nrows > 0, NULL hash, 2^32 - 1 rows or more.  *out is cleared on failure.
 * GSIM_ERR_STATE: a table not on a GPU, a multi-shard handle, a folded table, a table that changed after the index was made (its
 * row count or its row base; gsim_rowhash_get_stats and gsim_rowhash_groups read the index alone and still answer), the left
 * table's states and "different devices".  GSIM_ERR_NOMEM as elsewhere. */
typedef struct gsim_rowhash gsim_rowhash;
#define GSIM_ROW_NONE 0xFFFFFFFFu
#define GSIM_ROWHASH_REPEATS 1u   /* gsim_rowhash_rowset: the rows that are NOT their group's first row */
#pragma push_macro("slots")       /* (a translation unit that includes Qt has `slots` as a keyword macro) */
#undef slots
typedef struct {
    uint64_t rows;            /* N                                                                                            */
    uint64_t groups;          /* distinct rows                                                                                */
    uint64_t repeated_groups; /* groups of two rows or more                                                                   */
    uint64_t largest_group;   /* the largest size (0 for N = 0)                                                               */
    uint64_t slots;           /* slots(N)                                                                                     */
    uint64_t launches;        /* kernel launches of the build: the slots' initialisation, the inserting passes, the finish    */
    double kernel_ms;         /* HIP events around the inserting passes (insert_ms) and the finish, summed                    */
    double wall_ms;           /* the whole build, host clock                                                                  */
} gsim_rowhash_stats;
#pragma pop_macro("slots")
int gsim_rowhash_create(gsim_db* db, uint32_t flags /* 0 */, gsim_rowhash** out);
int gsim_rowhash_get_stats(const gsim_rowhash* ix, gsim_rowhash_stats* out);
int gsim_rowhash_groups(const gsim_rowhash* ix, uint32_t* first /* N or NULL */, uint32_t* size /* N or NULL */);
int gsim_rowhash_rowset(const gsim_rowhash* ix, uint32_t flags, gsim_rowset** out);
int gsim_rowhash_find(const gsim_rowhash* ix, const uint32_t* queries, uint64_t nq, uint32_t* row, uint32_t* size /* or NULL */);
int gsim_rowhash_find_db(const gsim_rowhash* ix, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint32_t* row,
                         uint32_t* size /* or NULL */);
int gsim_rowhash_destroy(gsim_rowhash* ix);
int gsim_row_hash(const uint32_t* rows, uint64_t nrows, uint32_t fp_bits, uint64_t* hash /* nrows */); /* host */
int gsim_duplicates(const uint32_t* rows, uint64_t nrows, uint32_t fp_bits, uint32_t* first /* nrows or NULL */,
                    uint32_t* size /* nrows or NULL */, uint64_t* ngroups /* or NULL */); /* host */

/* ---- instrumentation ------------------------------------------------------ */
int gsim_db_enable_timing(gsim_db* db, int enable); /* resets the accumulators */
int gsim_db_get_timing(gsim_db* db, gsim_timing* out); /* synchronises the stream */
/* With timing enabled: one byte per query of the handle's LAST gsim_db_search / _each / _timed call (first min(n, queries) bytes of
 * `flags`; *written = how many) -- 1 its own single launch handed it back, 2 run again behind a launch that did not close its query,
 * 4 its block's checksum never matched, 8 routed around the single launch by the back-off, 16 large k: publishing launch or
 * bin-ranked emission handed it back, 32 large k: routed around those by a back-off.  For the tests that compare the pipelined
 * entry point with one query at a time. */
int gsim_debug_query_flags(gsim_db* db, uint8_t* flags, uint32_t n, uint32_t* written);
/* Litmus tests of the hardware behaviours the single launch rests on, with its own instructions (gsim_litmus.hip; nothing of the product
 * calls them).  test 1: aligned 16-byte write-through (sc1) stores are seen whole by 16-byte sc1 loads of another workgroup; test 2: a
 * 16-byte system-scope store into pinned host memory is whole for a host that polls one of its words and then reads the others (how
 * gsim_db_search reads a result header); test 3: entry then header from one lane -- how often a reader sees the header first, and that
 * a re-read always finds the entry; test 4: the same with the product's shape (entries stored by another wave, a workgroup barrier, then
 * the header).  `workgroups` even (pairs of writer + reader; test 2: one writer each), `iterations` stores per slot
 * (64 slots per pair; test 2: one per workgroup).  stats[8] = {loads (test 2: host observations), torn values, headers seen, entries
 * behind their header at the first read, entries that never caught up, re-reads, workgroups that ran out of time, stores}. */
int gsim_debug_litmus(int device, int test, uint32_t workgroups, uint32_t iterations, unsigned long long* stats);
/* score of every (common, popc_db) pair for a query of popcount a, computed ON
 * THE DEVICE with the scan kernel's arithmetic: out[c * (max_b+1) + b].  Used
 * by the parity tests to pin the f32 divide bit for bit. */
int gsim_debug_score_table(int device, int metric, float alpha, float beta, uint32_t a,
                           uint32_t max_b, uint32_t max_c, float* out);

/* The constants of the matrix-core pass's division-free pre-filter (gsim_prefilter.h) for query
 * popcounts 0..max_qa: without a cutoff for every threshold bin, out[(qa * 512 + bin) * 4 + i],
 * with one for the cutoff's level, out[qa * 4 + i]; i = {ka, kb, u, v}.  device >= 0: computed by
 * a kernel on that device; device < 0: computed on the host by the same code.  The parity tests
 * compare the two (the exhaustive filter-never-rejects-an-accepted-pair test runs on the host). */
int gsim_debug_prefilter_constants(int device, int metric, float alpha, float beta, uint32_t max_qa,
                                   int has_cutoff, float cutoff, float* out);

/* The device sort behind k > 8192 and the folded tables' re-score (launch_sort_desc: tiles sorted in LDS, positions by
 * counting): keys[0 .. n), n a power of two, sorted in place, descending; equal keys (the callers pad with zeros) keep a
 * deterministic order.  For the parity tests. */
int gsim_debug_sort_desc(int device, unsigned long long* keys, uint32_t n);

const char* gsim_last_error(void);
const char* gsim_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUSIM_HIP_H */
