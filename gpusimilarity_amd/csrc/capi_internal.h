// capi_internal.h -- what the translation units of the C-ABI implementation (capi_*.cpp) share: the per-shard and
// per-handle state, error plumbing, and the host-side steps one TU implements and another calls.  Internal; the ABI is
// include/gpusim_hip.h.  No exception crosses the ABI.
#pragma once

#include "../../include/gpusim_hip.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "capi_knobs.h"
#include "capi_owned.h"
#include "gsim_device.h"
#include "gsim_synth.h"

namespace gsim_host
{

extern thread_local std::string g_last_error;

int fail(int code, const std::string& msg);
int fail_hip(hipError_t e, const char* what);

#define GSIM_HIP(call)                                   \
    do {                                                 \
        hipError_t e__ = (call);                         \
        if (e__ != hipSuccess) return fail_hip(e__, #call); \
    } while (0)
// device memory whose shortage is GSIM_ERR_NOMEM, the caller's to handle
#define GSIM_ALLOC(buf, bytes, what)                                                                 \
    do {                                                                                             \
        if ((buf).grow(bytes) != hipSuccess) return fail(GSIM_ERR_NOMEM, "device memory for " what); \
    } while (0)

#ifdef GSIM_TEST_HOOKS
int env_int(const char* name, int dflt);
#endif
// Test hook (compiled only with -DGSIM_TEST_HOOKS: testhooks/libgsim_hip.so, never the shipped library):
// GSIM_TEST_ALIAS_DEVICES=N makes the library present N logical devices that all
// live on physical device 0, so that the in-process multi-device code -- gsim_db_finalize(db, dev, n > 1), the shard
// fan-out and host merge of search_one / the batch path / folded tables, gsim_next_device's round robin,
// gpusimserver --gpus N -- runs on a one-GPU box exactly as it would on N GPUs (own stream, state and scratch per
// shard; only the physical device index differs).
int alias_devices();
int phys_device(int logical);
hipError_t set_device(int logical);

// Host memory the kernels write and the host reads WHILE the kernel still runs (completion words, result blocks): it has
// to be coherent (fine-grained) whatever the runtime's default for pinned memory is (HIP_HOST_COHERENT).
// Portable: pinned for, and mapped into, EVERY device of the process -- a multi-device handle's kernels on GPU 1..7 read
// queries from and write blocks into buffers that were allocated while another device was current.
constexpr unsigned kHostPolled = hipHostMallocPortable | hipHostMallocCoherent;
constexpr unsigned kHostPinned = hipHostMallocPortable; // staging the kernels read (queries) or copies go through
constexpr int kTimingRing = 1024;
// single-launch path: 4096 summary keys + the checkpoint tickets (kFusedCheckpoints x 9 counters, 128 B apart) + the
// arrival counters (128 B apart)
constexpr size_t kTicketWords = static_cast<size_t>(gsim::kFusedCheckpoints) * 9 * 32;
constexpr size_t kSummBytes = 4096 * 4 + kTicketWords * 4 + static_cast<size_t>(gsim::kFusedArriveWords) * 128;
constexpr int kQueryRing = 16;
constexpr int kPipe = 8; // single queries of one gsim_db_search_each call enqueued ahead of the one being waited for (< kQueryRing)

// The launch sequence of a single query on a shard ("Routes of a single query"; plan_query picks it)
enum class Route : uint8_t { kClassic, kRanked, kPublishBinrank, kPublishRadix };
// A route's back-off: after a hand-back (a second scan) the next base << min(streak + lead, 6) queries go around it -- the streak
// with this hand-back (lead 1) or before it (lead 0) -- once the streak is min_streak.  It counts even with GSIM_FUSED_BACKOFF=0.
struct Backoff {
    uint32_t base, lead, min_streak, streak = 0, skip = 0;
    bool take() { return skip > 0 ? (skip--, true) : false; } // route around it this time?
    void succeeded() { streak = 0; }
    void handed_back(bool enabled)
    {
        const uint32_t e = std::min(streak + lead, 6u);
        streak = std::min(streak + 1, 6u);
        if (enabled && streak >= min_streak) skip = base << e;
    }
};
struct ShardBlock { const void* out; uint8_t why; }; // one shard's result block of a query, and its slot's kQ* bits

struct Shard {
    int device = 0;
    int num_cus = 256;
    int cu_share = 1;       // > 1: a LANE of another shard -- its grids are sized for num_cus / cu_share compute units (see `lanes`)
    // Small tables, gsim_db_search_each: the query's launch streams for half its time and selects for the other half, and
    // launches on one stream serialise.  Two lanes = two half-grid copies of this shard's search state (own stream, per-query
    // state, regions, exchange buffer; the SAME rows): consecutive queries alternate between them, so one query's scan
    // overlaps the other's selection (capi_query.cpp search_each_pipelined; made on first use).
    std::vector<Shard> lanes;
    uint64_t first_row = 0; // offset inside the handle's table
    uint64_t nrows = 0;
    uint32_t W = 0;         // words per row ON THE DEVICE (table width / fold factor)
    void* d_rows = nullptr; // what the kernels read: rows_owned, or borrowed (attached rows; a lane borrows its shard's)
    DevBuf<> rows_owned;    // the table where the handle made it (empty for borrowed rows)
    DevBuf<uint16_t> d_rowpop; // popc(row) side array of the matrix-core batch pass (2 B per row, made on first use)
    bool rowpop_valid = false;
    hipStream_t stream = nullptr; // the stream in use (own or caller's)
    gsim::ScanGeometry geo{};
    gsim::ScanGeometry fgeo{}; // single-launch path: fewer waves on small tables (every wave gets >= 4 chunks)
    bool state_dirty = false; // set when an enqueue failed: the device state is re-zeroed before the next one
    DevBuf<uint32_t> d_query;
    DevBuf<gsim::QueryState> d_state;
    DevBuf<unsigned long long> d_cand;
    DevBuf<uint32_t> d_cand_cb;
    DevBuf<uint32_t> d_seg_count;
    DevBuf<unsigned long long> d_final;
    DevBuf<uint32_t> d_final_cb;
    uint32_t final_cap = 0;
    // folded tables: the storage's FULL fingerprints in HBM too (when they fit), and the re-score's buffers
    DevBuf<uint32_t> d_full;
    DevBuf<uint32_t> d_fq;               // the full query (+ one word: the NaN flag)
    HostBuf<uint32_t> h_fq{kHostPinned}; // ... its pinned staging
    DevBuf<unsigned long long> d_key2;   // re-scored keys, 2 x 64 Ki (the sort's second buffer)
    DevBuf<uint32_t> d_cb2;
    DevBuf<unsigned long long> d_large; // k > kSelectCap: the gathered top-k keys and the sort's second buffer, 2 x next_pow2(k) entries
    uint32_t large_cap = 0;
    DevBuf<gsim::LargeKState> d_lk;
    DevBuf<uint32_t> d_bincur;    // kScanBins cursors of launch_fused_binsort (zero between queries) + kScanBins words: the bins' first positions
    bool classic_ready = false; // candidate / finalist scratch of the four-kernel pipeline (allocated on first use)
    uint64_t cand_slots = 0;    // gsim_db_search_rows: slots of d_cand / d_cand_cb and words of d_seg_count where one of its geometries needed
    uint32_t seg_waves = 0;     // more than geo's (0: as geo -- capi_subset.cpp grows them, never shrinks)
    DevBuf<> d_pub;          // single-launch path: the workgroups' published-candidate regions (128 KB each)
    DevBuf<> d_hdr;          // ... and their headers (64 B each)
    DevBuf<uint32_t> d_summ; // single-launch path: per-wave checkpoint summaries (16 KB, zero between queries)
    HostBuf<uint32_t> h_done{kHostPolled}; // single-launch path: pinned words, one per pipeline slot (since round 3 only their address is used: "the caller polls the header")
    uint32_t epoch = 0;
    uint32_t pub_tag = 0;           // the last single launch's FusedArgs::pub_tag
    // One synchronous query in flight on this shard (gsim_db_search: slot 0; gsim_db_search_each: up to kPipe, slot = query mod kPipe):
    // how it was enqueued, what its caller waits for, and why it had to be run again.
    struct PipeSlot {
        bool inflight = false;  // enqueued by a synchronous caller and not finished yet (whatever route it took)
        Route route = Route::kClassic; // how it was enqueued (valid until the next enqueue): kRanked announces itself in the header ...
        uint32_t epoch = 0;     // ... with this epoch; the publishing routes say "handed back" with header flag 2
        Event ev;               // recorded behind the last kernel of an enqueue that is not the single launch's own: the caller waits
        bool ev_set = false;    // for THIS query, not for the queries enqueued behind it on the stream
        bool rerun = false;     // it ran behind a launch that left the per-query state dirty: not to be trusted, run again
        uint8_t why = 0;        // kQ* bits: how it was routed and why it was run again (gsim_debug_query_flags)
    } slot[kPipe];
    HostBuf<char> h_pipe{kHostPolled}; // kPipe pinned result blocks (gsim_db_search_each)
    // the synchronous routes' back-offs (plan_query takes them, finish_query_sync feeds them): queries skipped after a hand-back
    Backoff ranked_backoff{1, 1, 2};   // the single launch (scores that tie heavily): 4, 8, ... 64, from two hand-backs in a row
    Backoff publish_backoff{1, 1, 0};  // the publishing launch: 2, 4, ... 64
    Backoff binrank_backoff{16, 0, 0}; // the bin-ranked emission (ties in the top bins): 16, 32, ... 1024, by the radix tail instead
    DevBuf<unsigned long long> d_dbg; // GSIM_FUSED_DEBUG: per-workgroup phase timestamps
    DevBuf<uint32_t> d_gqueries; // gsim_db_search_group: the call's queries and, behind them, their popcounts (grown, never shrunk)
    HostBuf<uint32_t> h_gqpop{kHostPinned}; // ... the popcounts' pinned staging
    DevBuf<uint32_t> d_pqueries; // gsim_db_search_bounded: the call's queries (grown, never shrunk: a screening loop pays no allocation per call)
    DevBuf<float> d_pbounds;     // ... the bound table of one query popcount, fp_bits + 1 floats
    HostBuf<float> h_pbounds{kHostPinned}; // ... and its pinned copy
    DevBuf<> d_result;
    // pinned host staging; queries go through a ring so that back-to-back
    // asynchronous searches never overwrite a query whose upload is still queued
    HostBuf<uint32_t> h_query{kHostPinned}; // kQueryRing slots of W words
    std::vector<Event> q_ev; // scan-done event per slot (asynchronous searches)
    bool q_pending[kQueryRing] = {};
    uint32_t q_next = 0;
    HostBuf<unsigned char> h_result{kHostPolled};
    HostBuf<gsim::QueryState> h_state{kHostPinned}; // staging for the running totals
    // timing
    std::vector<Event> ev; // 3 per slot
    uint32_t ev_used = 0;
    std::vector<Event> bev; // multi-query passes: 2 per slot
    uint32_t bev_used = 0;
    unsigned long long base_ncand = 0, base_nfinal = 0, base_nredo = 0; // device totals when timing was enabled
    // multi-query batches (allocated on first use)
    gsim::ScanGeometry bgeo{};
    uint32_t bq_cap = 0;          // queries the batch buffers hold
    uint32_t bseg_cap = 0;        // candidate slots per wave segment, now / at most (grown on overflow) / number of segments
    uint32_t bseg_max = 0, bseg_waves = 0;
    DevBuf<uint32_t> d_bqueries;
    DevBuf<uint32_t> d_bqpop;
    DevBuf<gsim::BatchQueryState> d_bstate;
    DevBuf<unsigned long long> d_bcand;
    DevBuf<uint32_t> d_bcand_cb;
    DevBuf<uint32_t> d_bcand_q;
    DevBuf<uint32_t> d_bseg_count;
    DevBuf<unsigned long long> d_bfin_key;
    DevBuf<uint32_t> d_bfin_cb;
    DevBuf<uint32_t> d_bflags; // [0] overflow flags, [1] ticket
    DevBuf<gsim::BatchRare> d_brare;
    HostBuf<gsim::BatchRare> h_brare{kHostPinned}; // pinned
    HostBuf<uint32_t> h_bflags{kHostPinned};
    HostBuf<uint32_t> h_bqueries{kHostPinned}; // pinned staging: queries + popcounts
    HostBuf<unsigned char> h_bresult{kHostPinned};
    DevBuf<unsigned char> d_bresult; // the select kernel writes here; one bulk copy to h_bresult
    // in-process collective route (gsim_db_set_comm, capi_comm.cpp): every shard's gather buffer holds one slot per
    // shard (an in-place all-gather: the shard's own kernels write slot `index of the shard`)
    DevBuf<unsigned char> d_gather;
    DevBuf<unsigned char> d_merged; // first shard only: the merged blocks of a batch (single queries merge straight into h_result)
    Event gather_ev;                // loop-back comm (aliased devices): "this shard's block is in its slot"
    Event cev[3];                   // first shard, timing: scan done / gather done / merge done
    // gsim_db_neighbors: the pair buffer (sort keys + scores), grown to what a call needed and kept for the next one
    DevBuf<unsigned long long> d_nbr_keys;
    DevBuf<float> d_nbr_vals;
    uint64_t nbr_cap = 0;
    Stream own_stream; // (last: free_shard's `s = Shard{}` releases in this order, the stream behind everything enqueued on it)
};

} // namespace gsim_host

// resize() without zero-filling: the rows are copied in right away, by several threads, which then
// also take the first-touch page faults in parallel
template <class T> struct NoInitAllocator : std::allocator<T> {
    template <class U> struct rebind {
        using other = NoInitAllocator<U>;
    };
    template <class U> void construct(U* p) noexcept { ::new (static_cast<void*>(p)) U; }
    template <class U, class... Args> void construct(U* p, Args&&... args) { ::new (static_cast<void*>(p)) U(std::forward<Args>(args)...); }
};

// A row set (gsim_rowset_*, capi_subset.cpp): device memory of the handle it was made for, immutable.
struct gsim_rowset {
    gsim_db* owner = nullptr;
    int device = 0;
    uint64_t nrows = 0;       // rows of the owner's table when the set was made
    uint64_t count = 0;       // selected rows
    uint32_t row_base = 0;    // ... and its row base then (what gsim_rowset_rows adds)
    gsim_host::DevBuf<uint32_t> d_bits; // rowset_words(nrows) + kRowsetPadWords words
    gsim_host::DevBuf<uint32_t> d_list; // count rows, ascending, without the row base
};

// A label set (gsim_labelset_*, capi_label_search.cpp): device memory of the handle it was made for, immutable.
struct gsim_labelset {
    gsim_db* owner = nullptr;
    int device = 0;
    uint64_t nrows = 0;          // rows of the owner's table when the set was made
    uint32_t nlabels = 0;
    uint64_t labelled = 0;       // rows whose label is not GSIM_LABEL_NONE
    uint64_t nonempty = 0;       // labels with at least one row
    std::vector<uint32_t> sizes; // nlabels, counted on the host
    gsim_host::DevBuf<uint32_t> d_labels; // nrows labels
};

// A popcount index (gsim_popindex_*, capi_popindex.cpp): device memory of the handle it was made for, immutable.
// tests/popindex_front_errors_cases.py hands the fronts a stand-in (FakePopindex: zeroed memory that begins as this struct does, with
// `owner`, `device`, `nrows`, `fp_bits`, `row_base`, `flags` set) to reach the checks that read an index before any device state.  That
// holds while those six fields stay first, in this order, and while gsim_db_search_bounded reads nothing behind them ahead of
// check_table_state: move a field, or read `first` earlier, and change the stand-in with it.
struct gsim_popindex {
    gsim_db* owner = nullptr;
    int device = 0;
    uint64_t nrows = 0;          // rows of the owner's table when the index was made
    uint32_t fp_bits = 0;
    uint32_t row_base = 0;       // ... and its row base then (what gsim_popindex_order adds)
    uint32_t flags = 0;
    std::vector<uint64_t> first; // fp_bits + 2: rows with a popcount below b
    gsim_host::DevBuf<uint32_t> d_order; // nrows rows in (popcount, row) order, without the row base
    gsim_host::DevBuf<uint32_t> d_rows;  // GSIM_POPINDEX_ROWS: the rows in that order
};

// A row-hash index (gsim_rowhash_*, capi_rowhash.cpp): device memory of the handle it was made for, immutable.
// tests/rowhash_front_errors_cases.py hands the fronts a stand-in (FakeRowhash: zeroed memory that begins as this struct does, with
// `owner`, `device`, `nrows`, `fp_bits`, `row_base` set) to reach the checks that read an index before any device state.  That holds
// while those fields stay first, in this order, and while the fronts read nothing behind `stats` ahead of their state checks.
struct gsim_rowhash {
    gsim_db* owner = nullptr;
    int device = 0;
    uint64_t nrows = 0;          // rows of the owner's table when the index was made
    uint32_t fp_bits = 0;
    uint32_t row_base = 0;       // ... and its row base then (what the outputs add)
    uint32_t flags = 0;
    gsim_rowhash_stats stats{};  // of the build
    uint64_t nslots = 0;
    std::vector<uint32_t> bits;  // rowset_words(nrows): bit r says row r is its group's first
    gsim_host::DevBuf<uint32_t> d_slots;            // 2 x nslots words: {row, count}
    gsim_host::DevBuf<unsigned long long> d_groups; // nrows: first | size << 32, without the row base
};

struct gsim_db {
    uint32_t fp_bits = 0;
    uint32_t W = 0;
    uint64_t nrows = 0;
    std::vector<uint32_t, NoInitAllocator<uint32_t>> host_rows; // host copy (reference: m_data)
    bool has_host_copy = false;
    bool finalized = false;
    std::vector<gsim_host::Shard> shards;
    std::vector<uint64_t> slice_first; // first row of every add_rows slice (reference: one storage each)
    uint32_t fold_requested = 1;       // gsim_db_set_fold_factor
    uint32_t fold = 1;                 // effective factor (divides W), fixed at finalize
    bool fold_full_on_device = true;   // gsim_db_set_fold_full_on_device
    uint32_t row_base = 0;
    gsim_host::Knobs knobs;                 // the environment's tuning knobs as gsim_db_create found them
    bool timing = false;
    gsim_timing acc{};
    unsigned long long dense_batches = 0; // multi-query passes whose dense cutoff the matrix-core pass counted itself
    unsigned long long batch_regrown = 0; // batches run again with larger candidate segments
    std::atomic<unsigned long long> large_k_published{0}; // shard queries with k > kSelectCap scanned by the single launch
    // why synchronous queries were run a second time / routed around the single launch (host-side counts, gsim_timing.rerun_*)
    unsigned long long lane_queries = 0; // shard queries of gsim_db_search_each answered by a half-grid lane
    unsigned long long rerun_own = 0, rerun_behind = 0, rerun_torn = 0, rerun_publish = 0, backoff_skips = 0;
    size_t query_flags_at = 0;        // ... the query search_one is answering
    std::vector<uint8_t> query_flags; // kQ* bits of every query of the last gsim_db_search / _each call (timing enabled)
    std::vector<gsim_host::ShardBlock> blocks; // collect_blocks, kept across queries: one query's shard blocks, their hits, list ends
    std::vector<gsim_hit> merged;
    std::vector<size_t> merged_ends;
    unsigned long long blocks_checked = 0, blocks_rechecked = 0, blocks_torn = 0; // single launch, synchronous callers: result blocks whose checksum
                                                               // did not match at first sight / never did (re-run)
    gsim_comm* comm = nullptr; // gsim_db_set_comm: shard results meet through an RCCL all-gather + merge_kernel instead of on the host
    size_t comm_root = 0;      // ... on this shard's device (every device's buffer holds all blocks after the gather)
    // One search at a time per handle (the reference serialises searches behind a function-static
    // mutex, fingerprintdb_cuda.cu:236): concurrent callers queue here.
    std::mutex search_mutex;
};

namespace gsim_host
{

inline uint32_t next_pow2_u32(uint64_t x)
{
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p > 0x80000000ull ? 0x80000000u : static_cast<uint32_t>(p);
}

// milliseconds since t0: the wall time a call's stats report
inline double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

inline uint32_t popcount_words(const uint32_t* q, uint32_t W)
{
    uint32_t a = 0;
    for (uint32_t i = 0; i < W; i++) a += static_cast<uint32_t>(__builtin_popcount(q[i]));
    return a;
}

// ---- the host side of a tile call: what the callers of the tile and fold kernels (neighbours, joins, k-NN, histograms,
// components, the spanning forest) and of the matrix kernels (scores, assign) do before and after their launches ----

// One side's rows as those kernels read them: popc of every row and, where the rows are not WP words already, their zero-padded
// copy (nbr_prepare_kernel).
class PaddedRows
{
    DevBuf<uint32_t> pop_, pad_;
    uint32_t W_ = 0, WP_ = 0;
    const uint32_t* rows_ = nullptr;

public:
    // Room for n rows of W words.  A shortage is GSIM_ERR_NOMEM, "device memory for <what>", as GSIM_ALLOC; without labels it is
    // reported the way GSIM_HIP reports a failed call.
    int alloc(uint64_t n, uint32_t W, uint32_t WP, const char* what_pop = nullptr, const char* what_pad = nullptr)
    {
        W_ = W;
        WP_ = WP;
        if (!what_pop) {
            GSIM_HIP(pop_.grow(n * 4));
            if (WP != W) GSIM_HIP(pad_.grow(n * WP * 4));
            return GSIM_OK;
        }
        if (pop_.grow(n * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, std::string("device memory for ") + what_pop);
        if (WP != W && pad_.grow(n * WP * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, std::string("device memory for ") + what_pad);
        return GSIM_OK;
    }
    // Enqueues the preparation of d_rows[0 .. n), n at most alloc's; rows() and pop() are those rows' from here on.
    int prepare(const void* d_rows, uint64_t n, hipStream_t st)
    {
        GSIM_HIP(gsim::launch_nbr_prepare(d_rows, n, W_, WP_, pad_, pop_, st));
        rows_ = WP_ != W_ ? static_cast<const uint32_t*>(pad_) : static_cast<const uint32_t*>(d_rows);
        return GSIM_OK;
    }
    const uint32_t* rows() const { return rows_; } // WP words each
    const uint32_t* pop() const { return pop_; }
};

// The clock a call's launches ran at: the kernels' stamps (stamp_begin / stamp_end of gsim_device_common.h, four device words per launch: shader cycles
// and the 100 MHz wall clock at either end) and their sum over the launches, the rounds of a call included.
class LaunchClocks
{
    DevBuf<unsigned long long> own_;
    unsigned long long* d_ = nullptr;
    std::vector<unsigned long long> h_;
    double cyc_ = 0.0, ticks_ = 0.0;

public:
    static constexpr size_t kWords = 4; // per launch
    // the device words: inside the caller's control block, which the caller zeroes and may read back itself ...
    void view(unsigned long long* d_words) { d_ = d_words; }
    // ... or a buffer of their own for n launches
    int own(size_t n, const char* what)
    {
        if (own_.grow(kWords * n * 8) != hipSuccess) return fail(GSIM_ERR_NOMEM, std::string("device memory for ") + what);
        d_ = own_;
        return GSIM_OK;
    }
    unsigned long long* at(size_t l) const { return d_ + kWords * l; } // launch l's (the kernel argument `clk`)
    hipError_t zero(size_t n, hipStream_t st) { return hipMemsetAsync(d_, 0, kWords * n * 8, st); }
    // enqueues the copy of n launches' words to the host; add() them once the stream has been waited for
    hipError_t fetch(size_t n, hipStream_t st)
    {
        h_.assign(kWords * n, 0);
        return n ? hipMemcpyAsync(h_.data(), d_, h_.size() * 8, hipMemcpyDeviceToHost, st) : hipSuccess;
    }
    void add() { add(h_.data(), h_.size() / kWords); }
    // n launches' words the caller read back with its control block
    void add(const unsigned long long* h, size_t n)
    {
        for (size_t l = 0; l < n; l++) {
            cyc_ += static_cast<double>(h[kWords * l + 2] - h[kWords * l]);
            ticks_ += static_cast<double>(h[kWords * l + 3] - h[kWords * l + 1]);
        }
    }
    double mhz() const { return ticks_ > 0.0 ? cyc_ / ticks_ * 100.0 : 0.0; } // wall clock: 100 MHz
};

enum QueryMode { kAuto = 0, kClassic = 1 };
// Per-query record of the synchronous routes (Shard::PipeSlot::why -> gsim_db::query_flags -> gsim_debug_query_flags)
constexpr uint8_t kQHandedBack = 1;   // the single launch ran the query and handed it back itself (gsim_timing.handed_back counts these)
constexpr uint8_t kQRerunBehind = 2;  // run again because a launch ahead of it on the stream ended without closing its query
constexpr uint8_t kQTorn = 4;         // run again because its block's checksum never matched
constexpr uint8_t kQSkipFused = 8;    // routed around the single launch by the back-off after earlier hand-backs
constexpr uint8_t kQPublishBack = 16; // large k: the publishing launch or the bin-ranked emission handed it back
constexpr uint8_t kQSkipPublish = 32; // large k: routed around the publishing launch / the bin-ranked emission by a back-off
constexpr uint32_t kBatchMaxQ = 256; // queries per batch call on a shard (larger requests are split)

// capi_lifecycle.cpp
int free_shard(Shard& s);
int setup_shard(gsim_db* db, Shard& s);
// capi_query.cpp: the single-query path
int ensure_result_capacity(Shard& s, uint32_t k);
int enqueue_query(gsim_db* db, Shard& s, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha, float beta,
                  uint32_t row_base, void* out, bool caller_syncs, QueryMode mode = kAuto, uint32_t pipe_slot = 0);
int wait_stream(hipStream_t st);
int finish_query_sync(gsim_db* db, Shard& s, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha, float beta,
                      uint32_t row_base, void* out, uint32_t pipe_slot = 0);
int search_one(gsim_db* db, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha, float beta, gsim_hit* hits,
               uint32_t* count, uint64_t* approx);
int check_search_args(gsim_db* db, const uint32_t* queries, int metric);
int ensure_classic_scratch(Shard& s);
int rezero_dirty_state(Shard& s);
gsim::ScanArgs scan_args(const Shard& s, const uint32_t* query_words, const uint32_t* query, uint32_t* query_dev, uint32_t k, float cutoff, int metric,
                         float alpha, float beta);
int enqueue_scan_tail(gsim_db* db, Shard& s, const gsim::ScanArgs& a, const gsim::ScanGeometry& g, uint32_t row_base, uint64_t approx_if_no_cutoff,
                      void* out);
// capi_subset.cpp: the candidate scratch for a scan of geometry g behind which enqueue_scan_tail runs (row sets, group queries)
int ensure_subset_scratch(Shard& s, const gsim::ScanGeometry& g);
// ... one such scan for a query (row sets, bounded searches) and the wait for its block in s.h_result.  `a`: the query's scan_args,
// at most a.k hits wanted; `enqueue(a, launches)` launches the scan of geometry g on s.stream, adds what it launched to `launches` and
// may adjust `a` for the tail; all_rows: what the tail reports as approx without a cutoff; ev: timed, or null.  The scratch and
// result-capacity checks, the events, the tail and the wait are the two halves in capi_subset.cpp; the kernel time and the launches
// are added to *cost.
struct ScanStepCost {
    double kernel_ms = 0.0;
    uint32_t launches = 0;
};
int begin_restricted_scan(Shard& s, gsim::ScanArgs& a, const gsim::ScanGeometry& g, EventPair* ev);
int finish_restricted_scan(gsim_db* db, Shard& s, const gsim::ScanArgs& a, const gsim::ScanGeometry& g, uint64_t all_rows, EventPair* ev,
                           ScanStepCost* cost);
template <class Enqueue>
int run_restricted_scan(gsim_db* db, Shard& s, gsim::ScanArgs a, const gsim::ScanGeometry& g, uint64_t all_rows, EventPair* ev, Enqueue&& enqueue,
                        ScanStepCost* cost)
{
    int rc = begin_restricted_scan(s, a, g, ev);
    if (rc == GSIM_OK) rc = enqueue(a, cost->launches);
    return rc == GSIM_OK ? finish_restricted_scan(db, s, a, g, all_rows, ev, cost) : rc;
}
// ... and the answer it left there: at most k hits, their number, the header's approx (or null).  Returns the number of hits.
uint32_t take_scan_result(const Shard& s, uint32_t k, gsim_hit* hits, uint32_t* count, uint64_t* approx);
// ... and its route rule (GSIM_SUBSET_GATHER_MAX_PERMILLE): gather a set of `selected` rows through its list, or stream under its bitmap?
bool subset_gather_applies(const gsim_db* db, const Shard& s, uint64_t selected);
// capi_batch.cpp: multi-query passes
int enqueue_batch(gsim_db* db, Shard& s, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, int metric, float alpha,
                  float beta, uint32_t row_base, void* results, bool allow_mfma = true);
int run_batch(gsim_db* db, const uint32_t* qb, uint32_t nb, uint32_t k, float cutoff, int metric, float alpha, float beta,
              const std::vector<void*>& outs);
int search_batched(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k, uint32_t kout, float cutoff, int metric, float alpha,
                   float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx);
// capi_folded.cpp
void fold_row(const uint32_t* row, uint32_t W, uint32_t F, uint32_t* out);
void fold_rows_mt(const uint32_t* rows, uint64_t nrows, uint32_t W, uint32_t F, uint32_t* out);
int search_folded(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, gsim_hit* hits, uint32_t* counts,
                  uint64_t* approx);
// capi_merge.cpp
bool hit_before(const gsim_hit& x, const gsim_hit& y);
uint32_t merge_canonical_lists(const std::vector<gsim_hit>& lists, const std::vector<size_t>& ends, uint32_t k, gsim_hit* out);
// capi_comm.cpp: the collective route of a multi-device handle
int search_one_comm(gsim_db* db, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha, float beta, gsim_hit* hits,
                    uint32_t* count, uint64_t* approx);
int search_batch_comm(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k, uint32_t kout, float cutoff, int metric, float alpha,
                      float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx);
// capi_batch.cpp: nb <= kBatchMaxQ queries on one shard, result blocks in device memory at `out` (the per-shard half of
// gsim_db_search_batch_device)
int batch_to_device(gsim_db* db, Shard& s, const uint32_t* qb, uint32_t nb, uint32_t k, float cutoff, int metric, float alpha,
                    float beta, uint32_t row_base, unsigned char* out);
// capi_debug.cpp: timing, the phase profile of instrumented runs
int drain_timing(gsim_db* db, Shard& s);
int read_totals(Shard& s, unsigned long long* ncand, unsigned long long* nfinal, unsigned long long* nredo = nullptr);
void dump_fused_phases(Shard& s);

} // namespace gsim_host
