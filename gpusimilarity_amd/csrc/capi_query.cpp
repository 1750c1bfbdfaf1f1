// capi_query.cpp -- the single-query path of the C ABI: the route a query takes on a shard (plan_query chooses; the four
// routes and what their callers wait for: DESIGN.md section 3, "Routes of a single query"), their launch sequences,
// completion, the shard fan-out + host merge of FingerprintDB::search (fingerprintdb_cuda.cu:341-381), gsim_db_search / _each / _device.
#include "capi_internal.h"

#include <chrono>

namespace gsim_host
{

// Scratch of the four-kernel pipeline (per-wave candidate segments + finalists: the worst case is every row a candidate, 24 B per
// row).  The single-launch path keeps its candidates in LDS and needs none of it, so it is only allocated when a query takes the
// classic pipeline: k above the publishing route's, widths without a specialised scan, or a query handed back.
int ensure_classic_scratch(Shard& s)
{
    if (s.classic_ready) return GSIM_OK;
    GSIM_HIP(set_device(s.device));
    const uint64_t slots = static_cast<uint64_t>(s.geo.nwaves) * s.geo.seg_cap;
    GSIM_HIP(s.d_cand.grow(static_cast<size_t>(slots) * 8));
    GSIM_HIP(s.d_cand_cb.grow(static_cast<size_t>(slots) * 4));
    GSIM_HIP(s.d_seg_count.grow(static_cast<size_t>(s.geo.nwaves) * 4));
    const uint32_t cap = next_pow2_u32(slots);
    if (s.d_final.bytes() < static_cast<size_t>(cap) * 8) {
        // (the publishing route's smaller list: nothing is in flight on it when a classic query is about to be enqueued
        //  behind it on the same stream -- but the free must not overtake the kernels)
        if (s.d_final) GSIM_HIP(hipStreamSynchronize(s.stream));
        s.final_cap = 0;
    }
    GSIM_HIP(s.d_final.grow(static_cast<size_t>(cap) * 8));
    s.final_cap = cap; // (it counts d_final alone, which the publishing routes share: set with it, whatever becomes of d_final_cb)
    GSIM_HIP(s.d_final_cb.grow(static_cast<size_t>(cap) * 4));
    s.classic_ready = true;
    return GSIM_OK;
}

// The finalist list alone, sized by what the single launch can publish (its workgroups' regions): all a synchronous caller's
// large-k query needs behind the publishing launch -- 16 MB, not the four-kernel pipeline's 24 bytes per row.
int ensure_publish_scratch(Shard& s)
{
    if (s.d_final) return GSIM_OK;
    GSIM_HIP(set_device(s.device));
    const uint32_t cap = next_pow2_u32(static_cast<uint64_t>(s.fgeo.nwaves / 4) * gsim::kFusedRegion);
    GSIM_HIP(s.d_final.grow(static_cast<size_t>(cap) * 8));
    s.final_cap = cap;
    return GSIM_OK;
}

int ensure_result_capacity(Shard& s, uint32_t k)
{
    const size_t need = gsim_result_block_bytes(k);
    if (need > s.d_result.bytes()) {
        GSIM_HIP(set_device(s.device));
        GSIM_HIP(s.d_result.grow(need));
    }
    GSIM_HIP(s.h_result.grow(need));
    return GSIM_OK;
}

bool fused_applies(const gsim_db* db, const Shard& s, uint32_t k)
{
    if (!db->knobs.fused || k == 0 || k > gsim::kFusedMaxK || s.nrows == 0 || !gsim::fused_supported(s.fgeo)) return false;
    // thresholds need >= k summary keys; without them every row is published (tiny tables only)
    return s.nrows <= 8192 || (gsim::fused_summary_keys(s.fgeo.nwaves, k) != 0 && gsim::fused_final_keys(s.fgeo.nwaves / 4, k) != 0);
}

// Largest k of the publishing route (at most kFusedPublishMaxK; round 5: 32768).  Measured at 100 M rows (profiles/r06_large_k.txt):
// k = 50 000 2.18 -> 1.93 ms (0.83 of the roofline), 100 000 2.31 -> 2.17; at 131 072 and beyond the waves' stores
// overflow before the first useful election and the queries are handed back: slower than the four-kernel pipeline
constexpr uint32_t kPublishMaxK = 100000;
static_assert(kPublishMaxK <= gsim::kFusedPublishMaxK, "the publishing launch's own limit");
// Largest k whose published rows are bin-ranked; above it they go through the radix select + sort (measured: 100 M rows, k = 100 000
// 2.31 ms bin-ranked with hand-backs for crowded bins, 2.11 ms by the radix tail; at k = 50 000 1.94 against 1.97).  128 / 256-bit rows
// score coarsely: from k ~ 10 000 on a top bin holds more than the emission takes (7 % of the k = 32 768 queries of an 8 M x 128-bit soak
// were handed back), so their large k takes the radix tail.
constexpr uint32_t kBinrankMaxK = 65536, kBinrankMaxKNarrow = 8192;

// k in (fused_select_max_k, kPublishMaxK]: the single launch scans and publishes (kFusedPublishOnly), the large-k kernels
// rank what it published -- from k = 2049, as the selectors' own ranking of thousands of rows is issue-bound.
// Every width with a register scan: 128 / 256-bit rows are seeded like the ranking launch (plan_query).
bool fused_publish_applies(const gsim_db* db, const Shard& s, uint32_t k)
{
    if (!db->knobs.fused || k <= static_cast<uint32_t>(db->knobs.fused_select_max_k) || k > kPublishMaxK || s.nrows == 0 || !gsim::fused_supported(s.fgeo))
        return false;
    if (s.fgeo.ragged_words || s.fgeo.ragged_loads) return false;
    if (gsim::fused_summary_keys(s.fgeo.nwaves, k, gsim::fused_publish_max_m(k)) == 0) return false; // (no thresholds: every row would be published)
    if (s.nrows < static_cast<uint64_t>(db->knobs.publish_min_rows_per_k) * k) return false; // (a short table: the thresholds come late and most of it is published)
    return k <= 65536u || s.nrows >= 32ull * k; // (measured: 1 M rows, k = 100 000 -- a tenth of the table -- 286 us classic, 303 published)
}

namespace
{
// The route of one query on one shard, whether the narrow-row seed runs ahead of the single launch, and the
// kQSkip* bits of the back-offs that routed it around a launch.  Back-offs are taken for synchronous callers only.
struct QueryPlan { Route route = Route::kClassic; bool seed = false; uint8_t why = 0; };

QueryPlan plan_query(gsim_db* db, Shard& s, uint32_t k, bool caller_syncs, QueryMode mode)
{
    QueryPlan p;
    if (mode != kAuto) return p;
    // (k between the knob fused_select_max_k and kFusedMaxK: the single launch could rank it, the publishing route is preferred)
    if (fused_publish_applies(db, s, k)) {
        if (caller_syncs && s.publish_backoff.take()) p.why |= kQSkipPublish; // (tables whose publishing launches hand every query back)
        else p.route = Route::kPublishRadix;
    }
    if (p.route == Route::kClassic && fused_applies(db, s, k)) {
        if (caller_syncs && s.ranked_backoff.take()) p.why |= kQSkipFused;
        else p.route = Route::kRanked;
    }
    if (p.route == Route::kPublishRadix && caller_syncs) {
        // The caller reads the block, so a hand-back costs a second run, not a wrong answer: bin-ranked emission (two launches, not
        // the radix tail's four and a gap), up to kBinrankMaxK.
        if (k <= ((s.fgeo.lanes_per_row != 0 && s.fgeo.lanes_per_row <= 2) ? kBinrankMaxKNarrow : kBinrankMaxK)) {
            if (s.binrank_backoff.take()) p.why |= kQSkipPublish;
            else if (db->knobs.largek_binrank) p.route = Route::kPublishBinrank;
        }
    }
    if (p.why) db->backoff_skips++;
    // Narrow rows (128 / 256 bits): a wave's LDS store (2048 slots) fills before the first in-loop threshold is elected (~12 us), so
    // sparse tables were handed back (1/64 of the queries at 256 bits, nearly all at 128).  A strided sample first leaves a starting
    // threshold.  (Ragged word counts too: they never take the publishing routes, and every launch route has k > 0.)
    const bool narrow = (s.geo.lanes_per_row != 0 && s.geo.lanes_per_row <= 2) || s.fgeo.ragged_words;
    p.seed = p.route != Route::kClassic && narrow && s.nrows > 1500ull * s.fgeo.nwaves;
    return p;
}

// The tag of a launch's published lists (FusedArgs::pub_tag): never 0 (what the regions hold when they are allocated), and its
// low 26 bits -- the part a header carries -- never 0 either.
uint32_t next_pub_tag(Shard& s)
{
    do s.pub_tag++;
    while ((s.pub_tag & 0x3FFFFFFu) == 0);
    return s.pub_tag;
}

// Large-k device state, zeroed when made (its kernels leave it zero): d_lk, the d_bincur cursors (`bincur`), `large` keys in d_large
int ensure_largek_scratch(Shard& s, bool bincur, uint32_t large)
{
    if (large > s.large_cap) {
        s.large_cap = 0;
        GSIM_HIP(s.d_large.grow(static_cast<size_t>(large) * 8));
        s.large_cap = large;
    }
    bool fresh = false;
    GSIM_HIP(s.d_lk.grow(sizeof(gsim::LargeKState), &fresh));
    if (fresh) GSIM_HIP(hipMemsetAsync(s.d_lk, 0, sizeof(gsim::LargeKState), s.stream));
    if (bincur) {
        GSIM_HIP(s.d_bincur.grow(static_cast<size_t>(gsim::kScanBins) * 8, &fresh)); // (cursors + the layout)
        if (fresh) GSIM_HIP(hipMemsetAsync(s.d_bincur, 0, static_cast<size_t>(gsim::kScanBins) * 8, s.stream));
    }
    return GSIM_OK;
}

// One query's enqueue on one shard: its kernel arguments, where its block goes, its ring slot and the synchronous caller's
// pipeline slot, and the gsim_timing events (null: timing off; ev[0] before the scan, ev[1] behind it, ev[2] behind the last kernel)
struct QueryLaunch {
    gsim_db* db;
    Shard& s;
    gsim::ScanArgs a;
    uint32_t k, row_base, ring, pipe_slot;
    void* out;
    bool caller_syncs;
    Event* ev;
};

// The single launch's arguments: ranking the query, or publishing only (kFusedPublishOnly: M up to fused_publish_max_m, no final threshold)
gsim::FusedArgs fused_args(const gsim_db* db, Shard& s, uint32_t k, bool publish)
{
    gsim::FusedArgs f{};
    f.pub = s.d_pub;
    f.hdr = s.d_hdr;
    f.arrive = s.d_summ + 4096 + kTicketWords;
    f.summ = s.d_summ;
    f.summ_keys = publish ? gsim::fused_summary_keys(s.fgeo.nwaves, k, gsim::fused_publish_max_m(k)) : gsim::fused_summary_keys(s.fgeo.nwaves, k);
    f.final_keys = publish ? 0 : gsim::fused_final_keys(s.fgeo.nwaves / 4, k);
    f.tickets = s.d_summ + 4096;
    // grid-wide waits give up after 2 ms + four scan times at 4 TB/s (only reached when the GPU is shared)
    f.wait_ticks = static_cast<uint32_t>(std::min<uint64_t>(200000ull + static_cast<uint64_t>(s.nrows) * s.W * 4 / 10000ull, 0xFFFFFFFFull));
    const uint32_t xflags = static_cast<uint32_t>(db->knobs.fused_flags);
    f.xflags = publish ? (xflags & ~4u) | gsim::kFusedPublishOnly : xflags;
    f.pub_tag = next_pub_tag(s);
    return f;
}

// The narrow-row seed (plan_query): xflags bit 2 says the sample kernel (its own size rule) left a threshold in QueryState::gtau.
hipError_t seed_threshold(const QueryLaunch& q, gsim::FusedArgs& f)
{
    bool seeded = false;
    const hipError_t e = gsim::launch_sample(q.a, q.s.geo, 1u, q.s.stream, &seeded);
    if (seeded) f.xflags |= 4u;
    return e;
}

// The finalist count the last large-k query left in pinned memory: the last word of h_done's 64-byte block
static_assert(kPipe <= 15, "the large-k hint word shares h_done's 64-byte block with the pipeline's completion words");
uint32_t* largek_hint(const Shard& s)
{
    return s.h_done + 15;
}

// Large k: the k-th largest finalist key by a radix select on the device (the finalist count never reaches the host: nothing
// here waits), the keys at or above it gathered and sorted in global memory (sized by k); `flags` to the emission
int enqueue_largek_tail(const gsim_db* db, Shard& s, const gsim::ScanArgs& a, uint32_t row_base, uint64_t approx_if_no_cutoff, uint32_t flags,
                        void* out)
{
    const uint32_t np2 = next_pow2_u32(a.k);
    const int rc = ensure_largek_scratch(s, false, np2);
    if (rc != GSIM_OK) return rc;
    // (one workgroup in one launch up to 32 Ki finalists, the grid's eight passes beyond, chosen by the finalist
    // count the previous large-k query left in pinned memory: a wrong guess is slower, never wrong)
    uint32_t* hint = largek_hint(s);
    const bool one_block = *static_cast<volatile uint32_t*>(hint) <= static_cast<uint32_t>(db->knobs.largek_one_block_max);
    GSIM_HIP(gsim::launch_largek_select(a, s.d_final, s.final_cap, s.d_lk, s.d_large, np2, hint, one_block, s.stream));
    // (tiles sorted, then positions by counting + the hits + the header + the state's reset in one launch)
    GSIM_HIP(gsim::launch_largek_sort_emit(a, s.d_large, np2, s.d_lk, row_base, approx_if_no_cutoff, flags, out, s.stream));
    return GSIM_OK;
}
int enqueue_largek_tail(QueryLaunch& q, uint32_t flags)
{
    return enqueue_largek_tail(q.db, q.s, q.a, q.row_base, q.s.nrows, flags, q.out);
}

// The four-kernel pipeline: sample (kSampleChunks chunks per scan wave) -> scan -> compact -> select (`select`) or the large-k tail; gated
// (a.gate) behind a launch.
constexpr uint32_t kSampleChunks = 4;
// The kernels read the query from its pinned ring slot (no upload op) and the last one re-zeroes the per-query state (no memset op).
int enqueue_classic(QueryLaunch& q, bool select, bool mark_scan_start, bool mark_scan_end)
{
    Shard& s = q.s;
    if (s.nrows > 0) GSIM_HIP(gsim::launch_sample(q.a, s.geo, kSampleChunks, s.stream));
    if (mark_scan_start && q.ev) GSIM_HIP(hipEventRecord(q.ev[0], s.stream));
    if (s.nrows > 0) GSIM_HIP(gsim::launch_scan(q.a, s.geo, s.stream));
    if (!q.caller_syncs) { // the ring slot is free once the scan has run
        GSIM_HIP(hipEventRecord(s.q_ev[q.ring], s.stream));
        s.q_pending[q.ring] = true;
    }
    if (mark_scan_end && q.ev) GSIM_HIP(hipEventRecord(q.ev[1], s.stream));
    if (s.nrows > 0) GSIM_HIP(gsim::launch_compact(q.a, s.geo, s.d_final, s.d_final_cb, s.final_cap, s.stream));
    if (!select) return enqueue_largek_tail(q, 1u);
    GSIM_HIP(gsim::launch_select(q.a, s.d_final, s.d_final_cb, s.final_cap, q.row_base, q.out, s.stream));
    return GSIM_OK;
}

// kRanked: ONE kernel does scan + publish + select.  Synchronous callers poll the block's header: the closing workgroup stores
// {count, flags | epoch << 8, approx} in ONE 16-byte write when the hits are out (a separate completion word meant waiting for
// its acknowledgement over PCIe: ~1.3 us per query).  Enqueue-only callers get the classic kernels behind it, gated.
int enqueue_ranked(QueryLaunch& q, bool seed)
{
    Shard& s = q.s;
    gsim::FusedArgs f = fused_args(q.db, s, q.k, false);
    f.result = q.out;
    f.row_base = q.row_base;
    f.done_flag = q.caller_syncs ? s.h_done + q.pipe_slot : nullptr; // (non-null = "the caller polls the header")
    f.epoch = ++s.epoch & 0xFFFFFFu;
    if (f.epoch == 0) f.epoch = ++s.epoch & 0xFFFFFFu; // 0: what a clean header holds
    if (q.caller_syncs) static_cast<gsim_result_header*>(q.out)->flags = 0;
    if (q.db->knobs.fused_debug) GSIM_HIP(s.d_dbg.grow((static_cast<size_t>(s.fgeo.nwaves / 4) * 24 + 8) * 8));
    f.dbg = s.d_dbg;
    if (q.ev) GSIM_HIP(hipEventRecord(q.ev[0], s.stream));
    if (seed) GSIM_HIP(seed_threshold(q, f));
    GSIM_HIP(gsim::launch_fused(q.a, s.fgeo, f, s.stream));
    if (q.ev) GSIM_HIP(hipEventRecord(q.ev[1], s.stream));
    if (q.caller_syncs) {
        s.slot[q.pipe_slot].epoch = f.epoch;
        return GSIM_OK;
    }
    q.a.gate = &s.d_state->redo; // the classic kernels behind it run only if it handed the query back
    return enqueue_classic(q, q.k <= static_cast<uint32_t>(gsim::kSelectCap), false, false);
}

// kPublishBinrank / kPublishRadix -- large k: the single launch's scan (0.88 of the HBM roofline, the classic scan 0.82 + compaction)
// stops after publishing, the large-k kernels rank what it published.  A synchronous caller re-runs a hand-back (finish_query_sync)
// instead of paying for three gated launches, ~4.5 us each, behind every query.
int enqueue_publish(QueryLaunch& q, Route route, bool seed)
{
    Shard& s = q.s;
    gsim::FusedArgs f = fused_args(q.db, s, q.k, true);
    const int rc = ensure_largek_scratch(s, true, 0);
    if (rc != GSIM_OK) return rc;
    if (q.ev) GSIM_HIP(hipEventRecord(q.ev[0], s.stream));
    if (seed) GSIM_HIP(seed_threshold(q, f));
    GSIM_HIP(gsim::launch_fused(q.a, s.fgeo, f, s.stream));
    q.db->large_k_published++;
    if (route == Route::kPublishBinrank) {
        GSIM_HIP(gsim::launch_fused_binsort(q.a, f, s.fgeo.nwaves / 4, s.d_final, s.final_cap, s.d_bincur, s.stream));
        if (q.ev) GSIM_HIP(hipEventRecord(q.ev[1], s.stream));
        GSIM_HIP(gsim::launch_binrank_emit(q.a, s.d_final, s.final_cap, s.d_bincur, s.d_lk, q.row_base, s.nrows, 1u, q.out, s.stream));
        return GSIM_OK;
    }
    // the hand-off kernel makes the published lists the finalists
    GSIM_HIP(gsim::launch_fused_handoff(q.a, f, s.fgeo.nwaves / 4, s.d_final, s.final_cap, s.stream));
    q.a.gate = &s.d_state->redo;
    if (!q.caller_syncs) return enqueue_classic(q, false, false, true);
    if (q.ev) GSIM_HIP(hipEventRecord(q.ev[1], s.stream));
    return enqueue_largek_tail(q, 1u | 0x80000000u); // (flag 31: no gated kernels ran, a hand-back makes the block say so)
}

// Enqueue one query on one shard; the result block ends up at `out`, which is device memory or device-visible pinned host memory
// (zero-copy).  Nothing here synchronises with the host, whatever k.
int enqueue_query_impl(gsim_db* db, Shard& s, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha,
                       float beta, uint32_t row_base, void* out, bool caller_syncs, QueryMode mode, uint32_t pipe_slot)
{
    Shard::PipeSlot& sl = s.slot[pipe_slot]; // (only touched for synchronous callers)
    GSIM_HIP(set_device(s.device));
    int rc = rezero_dirty_state(s);
    if (rc != GSIM_OK) return rc;
    const QueryPlan p = plan_query(db, s, k, caller_syncs, mode);
    // the four-kernel pipeline's scratch wherever it runs (gated or not); behind a synchronous caller's publishing launch, its finalists'
    rc = p.route == Route::kClassic || !caller_syncs ? ensure_classic_scratch(s) : p.route != Route::kRanked ? ensure_publish_scratch(s) : GSIM_OK;
    if (rc != GSIM_OK) return rc;
    const uint32_t ring = s.q_next++ % kQueryRing;
    uint32_t* hq = s.h_query + static_cast<size_t>(ring) * s.W;
    if (s.q_pending[ring]) { // only set by asynchronous searches
        GSIM_HIP(hipEventSynchronize(s.q_ev[ring]));
        s.q_pending[ring] = false;
    }
    std::memcpy(hq, query, static_cast<size_t>(s.W) * 4); // `query` is already folded for a folded table

    // (the kernels read hq -- hipHostMalloc memory: device-visible at the same address; a.gate: null, set behind a launch)
    QueryLaunch q{db, s, scan_args(s, query, hq, s.d_query, k, cutoff, metric, alpha, beta), k, row_base, ring, pipe_slot, out, caller_syncs, nullptr};
    gsim::ScanArgs& a = q.a;
    if (s.geo.lanes_per_row == 0 || s.nrows == 0) {
        // generic-width scan reads the query per word: give it a device copy
        GSIM_HIP(hipMemcpyAsync(s.d_query, hq, static_cast<size_t>(s.W) * 4, hipMemcpyHostToDevice, s.stream));
        a.query = s.d_query;
    }
    if (db->timing && s.ev_used < kTimingRing) {
        if (s.ev.size() < static_cast<size_t>(3 * (s.ev_used + 1))) {
            for (int i = 0; i < 3; i++) {
                Event e;
                GSIM_HIP(e.create());
                s.ev.push_back(std::move(e));
            }
        }
        q.ev = &s.ev[3 * s.ev_used];
    }
    if (caller_syncs) {
        sl.route = p.route;
        sl.ev_set = false;
        sl.rerun = false; // (a slot is enqueued again only after it was finished: a flag still set here is stale -- ADVICE r05)
        sl.inflight = true;
        if (mode == kAuto) sl.why = p.why; // (a re-run, kClassic, keeps what the first run recorded)
    }
    switch (p.route) {
    case Route::kRanked: rc = enqueue_ranked(q, p.seed); break;
    case Route::kPublishBinrank:
    case Route::kPublishRadix: rc = enqueue_publish(q, p.route, p.seed); break;
    case Route::kClassic: rc = enqueue_classic(q, k <= static_cast<uint32_t>(gsim::kSelectCap), true, true); break;
    }
    if (rc != GSIM_OK) return rc;
    if (q.ev) {
        GSIM_HIP(hipEventRecord(q.ev[2], s.stream));
        s.ev_used++;
    }
    if (!caller_syncs || p.route == Route::kRanked) return GSIM_OK; // (kRanked announces itself in the block's header)
    // A synchronous query that does not end in the single launch's self-announcing block is waited for through an event of its
    // own: the stream holds up to kPipe - 1 later queries of a pipelined call, and waiting for IT to drain idled the device between
    // batches of eight (k = 8192 at 1 M rows: 74 us a query for 59 us of kernels).
    GSIM_HIP(sl.ev.create(hipEventDisableTiming));
    GSIM_HIP(hipEventRecord(sl.ev, s.stream));
    sl.ev_set = true;
    return GSIM_OK;
}
} // namespace

// A previous enqueue failed half way (state_dirty): the per-query state may not be zero -- re-zeroed before the next one
int rezero_dirty_state(Shard& s)
{
    if (!s.state_dirty) return GSIM_OK;
    GSIM_HIP(hipMemsetAsync(s.d_state, 0, offsetof(gsim::QueryState, redo_why), s.stream)); // (the per-query part)
    if (s.d_lk) GSIM_HIP(hipMemsetAsync(s.d_lk, 0, sizeof(gsim::LargeKState), s.stream));   // (a large-k enqueue may have failed between its radix passes)
    GSIM_HIP(hipMemsetAsync(s.d_summ, 0, kSummBytes, s.stream));
    if (s.d_bincur) GSIM_HIP(hipMemsetAsync(s.d_bincur, 0, static_cast<size_t>(gsim::kScanBins) * 4, s.stream));
    s.state_dirty = false;
    return GSIM_OK;
}

// A query's kernel arguments on a shard: `query_words` on the host (for its popcount), `query` / `query_dev` as the kernels read it
gsim::ScanArgs scan_args(const Shard& s, const uint32_t* query_words, const uint32_t* query, uint32_t* query_dev, uint32_t k, float cutoff, int metric,
                         float alpha, float beta)
{
    gsim::ScanArgs a{};
    a.rows = s.d_rows;
    a.nrows = s.nrows;
    a.W = s.W;
    a.query = query;
    a.query_dev = query_dev;
    a.qpop = popcount_words(query_words, s.W);
    a.k = k;
    a.cutoff = cutoff;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cand = s.d_cand;
    a.cand_cb = s.d_cand_cb;
    a.seg_count = s.d_seg_count;
    a.state = s.d_state; // (zero between queries: a query's last kernel re-zeroes it)
    return a;
}

// The four-kernel pipeline's tail behind a scan of the caller's own (capi_subset.cpp): compaction of the candidate segments of
// geometry g, then the select kernel or, above kSelectCap, the large-k select and sort -- as enqueue_classic runs them.
int enqueue_scan_tail(gsim_db* db, Shard& s, const gsim::ScanArgs& a, const gsim::ScanGeometry& g, uint32_t row_base, uint64_t approx_if_no_cutoff,
                      void* out)
{
    GSIM_HIP(gsim::launch_compact(a, g, s.d_final, s.d_final_cb, s.final_cap, s.stream));
    if (a.k <= static_cast<uint32_t>(gsim::kSelectCap)) {
        GSIM_HIP(gsim::launch_select(a, s.d_final, s.d_final_cb, s.final_cap, row_base, out, s.stream));
        return GSIM_OK;
    }
    return enqueue_largek_tail(db, s, a, row_base, approx_if_no_cutoff, 1u, out);
}

int enqueue_query(gsim_db* db, Shard& s, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha,
                  float beta, uint32_t row_base, void* out, bool caller_syncs, QueryMode mode, uint32_t pipe_slot)
{
    const int rc = enqueue_query_impl(db, s, query, k, cutoff, metric, alpha, beta, row_base, out, caller_syncs, mode, pipe_slot);
    if (rc != GSIM_OK) s.state_dirty = true;
    return rc;
}

// Wait for a stream: poll for a short while (a query takes ~2 ms and the blocking
// wait's interrupt wake-up costs 10-20 us), then block.
static int wait_event(hipEvent_t ev)
{
    for (int i = 0; i < 200000; i++) {
        hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return GSIM_OK;
        if (e != hipErrorNotReady) return fail_hip(e, "hipEventQuery");
    }
    GSIM_HIP(hipEventSynchronize(ev));
    return GSIM_OK;
}

int wait_stream(hipStream_t st)
{
    for (int i = 0; i < 200000; i++) {
        hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return GSIM_OK;
        if (e != hipErrorNotReady) return fail_hip(e, "hipStreamQuery");
    }
    GSIM_HIP(hipStreamSynchronize(st));
    return GSIM_OK;
}

// kRanked's block, announced by the header's epoch (before the stream reports the kernel retired).  `done`: the header arrived (no:
// the launch ended without closing the query); `torn`: its hits never matched its checksum (both false on entry).
static int wait_ranked_block(gsim_db* db, Shard& s, void* out, uint32_t k, uint32_t want, bool& done, bool& torn)
{
    volatile uint32_t* flag = &static_cast<gsim_result_header*>(out)->flags; // (flags | epoch << 8: one 16-byte store with the rest of the header)
    for (uint64_t spins = 0;; spins++) {
        if ((*flag >> 8) == want) {
            done = true;
            break;
        }
        if ((spins & 0x3FFu) == 0x3FFu) { // now and then: did the launch fail or end without the header?
            const hipError_t e = hipStreamQuery(s.stream);
            if (e == hipSuccess) {
                done = (*flag >> 8) == want;
                break;
            }
            if (e != hipErrorNotReady) return fail_hip(e, "hipStreamQuery");
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    gsim_result_header* h = static_cast<gsim_result_header*>(out);
    if (done && !(*flag & 2u)) {
        // The block validates itself: the closing workgroup put the sum of the words of all hits (+ epoch * kBlockCheckMul)
        // into the upper half of approx.  The hits were stored write-through at system scope and every selector waited for
        // their acknowledgements before its ticket, so they are in host memory when the header is -- on the platforms this
        // was soaked on.  Whether an acknowledgement means host visibility is the platform's business: if the
        // sums differ the hits are still on their way -- look again for a while, then let the stream drain; a block that
        // stays wrong is re-run on the four-kernel pipeline (gsim_timing.blocks_rechecked / blocks_torn count both).
        // (test hook, no production use: GSIM_TEST_TORN_EVERY=n makes every n-th block fail its check for good, so that the
        // re-run of a torn block -- with later queries of the call already enqueued behind it -- is exercised)
#ifdef GSIM_TEST_HOOKS
        static const int torn_every = env_int("GSIM_TEST_TORN_EVERY", 0);
        const uint32_t spoil = (torn_every > 0 && ++db->blocks_checked % static_cast<unsigned>(torn_every) == 0) ? 1u : 0u;
#else
        const uint32_t spoil = 0;
#endif
        auto block_ok = [&]() -> bool {
            const uint32_t n = h->count <= k ? h->count : k;
            const volatile uint32_t* w = reinterpret_cast<const volatile uint32_t*>(h + 1);
            uint32_t sum = 0;
            for (uint32_t i = 0; i < 3u * n; i++) sum += w[i];
            return static_cast<uint32_t>(h->approx >> 32) == sum + want * gsim::kBlockCheckMul + spoil;
        };
        bool good = block_ok();
        if (!good) {
            db->blocks_rechecked++;
            for (int spins = 0; spins < (spoil ? 2 : 20000) && !good; spins++) good = block_ok();
            if (!good) {
                (void) hipStreamSynchronize(s.stream);
                std::atomic_thread_fence(std::memory_order_acquire);
                good = block_ok();
            }
            if (!good) {
                db->blocks_torn++;
                torn = true; // (re-run by the caller; the kernel itself closed the query and left the state clean)
            }
        }
    }
    if (done) {
        *flag &= 0xFFu; // the header as every other route leaves it
        h->approx &= 0xFFFFFFFFull;
    }
    if (s.d_dbg && done) dump_fused_phases(s); // phase profile of this query (instrumented runs only)
    return GSIM_OK;
}

// Wait for the result block of a synchronous enqueue on `s` (it was given s.h_result or any pinned block `out`) and run the query
// again, on the four-kernel pipeline, when its route handed it back, its block is torn, or it ran behind a launch that failed.
int finish_query_sync(gsim_db* db, Shard& s, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha,
                      float beta, uint32_t row_base, void* out, uint32_t pipe_slot)
{
    Shard::PipeSlot& sl = s.slot[pipe_slot];
    sl.inflight = false;
    const bool backoff = db->knobs.fused_backoff != 0;
    auto run_again = [&]() -> int { // the four-kernel pipeline, waited for
        int rc = enqueue_query(db, s, query, k, cutoff, metric, alpha, beta, row_base, out, true, kClassic, pipe_slot);
        if (rc == GSIM_OK) rc = wait_stream(s.stream);
        sl.inflight = false;
        sl.ev_set = false;
        return rc;
    };
    if (sl.rerun) {
        // Enqueued behind a single launch that ended without closing its query (below): this one ran on per-query state
        // nobody had re-zeroed -- WHATEVER route it took (a classic or publishing query behind the failed launch
        // shared that state too) -- and a block's checksum only covers the block's own hits: run it again.  The stream had
        // drained when the flag was set, so its own kernels are over.
        sl.rerun = false;
        sl.why |= kQRerunBehind;
        db->rerun_behind++;
        return run_again();
    }
    if (sl.route != Route::kRanked) {
        const int rc = sl.ev_set ? wait_event(sl.ev) : wait_stream(s.stream);
        sl.ev_set = false;
        if (rc != GSIM_OK || sl.route == Route::kClassic) return rc;
        if (!(static_cast<const gsim_result_header*>(out)->flags & 2u)) {
            s.publish_backoff.succeeded();
            if (sl.route == Route::kPublishBinrank) s.binrank_backoff.succeeded();
            return GSIM_OK;
        }
        // handed back (heavy ties; the emission cleared the per-query state): by the bin-ranked emission or the launch itself
        (sl.route == Route::kPublishBinrank ? s.binrank_backoff : s.publish_backoff).handed_back(backoff);
        sl.why |= kQPublishBack;
        db->rerun_publish++;
        return run_again();
    }
    bool done = false, torn = false;
    const int rc = wait_ranked_block(db, s, out, k, sl.epoch, done, torn);
    if (rc != GSIM_OK) return rc;
    if (done && !torn && !(static_cast<const gsim_result_header*>(out)->flags & 2u)) {
        s.ranked_backoff.succeeded();
        return GSIM_OK;
    }
    if (torn) {
        sl.why |= kQTorn;
        db->rerun_torn++;
    } else if (done) { // handed back: the per-query state is zero again (the last selector reset it), `redo` is set
        s.ranked_backoff.handed_back(backoff);
        sl.why |= kQHandedBack;
        db->rerun_own++;
    } else {
        // The launch ended without closing the query: the state is re-zeroed, and the later queries of a pipelined call --
        // the stream has drained, so they have all run already, on that state -- are run again, whichever
        // route they took (every slot in flight, not only the single launch's)
        s.state_dirty = true;
        sl.why |= kQRerunBehind;
        db->rerun_behind++;
        for (uint32_t j = 0; j < static_cast<uint32_t>(kPipe); j++)
            if (j != pipe_slot && s.slot[j].inflight) s.slot[j].rerun = true;
    }
    return run_again();
}

// One query's answer from db->blocks (one per shard that ran it): the slots' `why` bits into query_flags[q], approx summed, the
// hits copied (a single-shard handle) or merged across shards (fingerprintdb_cuda.cu:363-380)
static void collect_blocks(gsim_db* db, size_t q, uint32_t k, gsim_hit* hits, uint32_t* count, uint64_t* approx)
{
    const bool one = db->shards.size() == 1;
    uint64_t ap = 0;
    db->merged.clear();
    db->merged_ends.clear();
    for (const ShardBlock& b : db->blocks) {
        if (q < db->query_flags.size()) db->query_flags[q] |= b.why;
        const gsim_result_header* h = static_cast<const gsim_result_header*>(b.out);
        const gsim_hit* hh = reinterpret_cast<const gsim_hit*>(h + 1);
        ap += h->approx;
        if (one) {
            std::memcpy(hits, hh, sizeof(gsim_hit) * h->count);
            *count = h->count;
        } else {
            db->merged.insert(db->merged.end(), hh, hh + h->count);
            db->merged_ends.push_back(db->merged.size());
        }
    }
    if (!one) *count = merge_canonical_lists(db->merged, db->merged_ends, k, hits);
    if (approx) *approx = ap;
}

// One query through the single-query pipeline on every shard, host merge across shards
// (FingerprintDB::search, fingerprintdb_cuda.cu:341-381).
int search_one(gsim_db* db, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha, float beta,
               gsim_hit* hits, uint32_t* count, uint64_t* approx)
{
    if (db->comm) return search_one_comm(db, query, k, cutoff, metric, alpha, beta, hits, count, approx);
    for (auto& s : db->shards) {
        int rc = ensure_result_capacity(s, k);
        if (rc != GSIM_OK) return rc;
        // the select kernel writes the block straight into pinned host memory
        rc = enqueue_query(db, s, query, k, cutoff, metric, alpha, beta,
                           db->row_base + static_cast<uint32_t>(s.first_row), s.h_result, true);
        if (rc != GSIM_OK) return rc;
    }
    db->blocks.clear();
    for (auto& s : db->shards) {
        GSIM_HIP(set_device(s.device));
        int rc = finish_query_sync(db, s, query, k, cutoff, metric, alpha, beta,
                                   db->row_base + static_cast<uint32_t>(s.first_row), s.h_result);
        if (rc != GSIM_OK) return rc;
        db->blocks.push_back({s.h_result, s.slot[0].why});
    }
    collect_blocks(db, db->query_flags_at, k, hits, count, approx);
    return GSIM_OK;
}

// Two half-grid lanes of a shard (Shard::lanes), made on first use: the same rows, half the compute units each, own
// stream / per-query state / regions / exchange buffer.
constexpr int kLanes = 2; // (three and four lanes, of a quarter or a half of the CUs each, measured slower: profiles/r06_each_lanes.txt)
int ensure_lanes(gsim_db* db, Shard& s)
{
    if (!s.lanes.empty()) return GSIM_OK;
    s.lanes.resize(kLanes);
    for (auto& l : s.lanes) {
        l.device = s.device;
        l.cu_share = kLanes;
        l.first_row = s.first_row;
        l.nrows = s.nrows;
        l.W = s.W;
        l.d_rows = s.d_rows; // (borrowed)
        const int rc = setup_shard(db, l);
        if (rc != GSIM_OK) {
            for (auto& x : s.lanes) (void) free_shard(x);
            s.lanes.clear();
            return rc;
        }
    }
    return GSIM_OK;
}

// Does a pipelined call alternate this shard's queries between its two lanes?  Only where the single launch ranks the query
// itself (k up to fused_select_max_k) or publishes for the large-k kernels (two small launches rank -- per lane), on a table
// small enough that the chain behind the scan is a large part of the launch.
constexpr uint64_t kLanesMaxBytes = 4096ull << 20; // (larger shards are HBM-bound: nothing to overlap)
bool lanes_apply(const gsim_db* db, const Shard& s, uint32_t k, uint32_t nq)
{
    if (db->knobs.each_lanes < 2 || nq < 4 || s.stream != s.own_stream || s.d_dbg || db->knobs.fused_debug) return false;
    if (s.nrows * s.W * 4ull > kLanesMaxBytes) return false;
    if (s.nrows < 65536) return false; // (tiny tables: the half grid is no smaller than the whole one)
    return fused_publish_applies(db, s, k) || fused_applies(db, s, k);
}

// gsim_db_search_each on a single-shard handle: the queries still run strictly one after the other on the GPU (one
// stream, one per-query state), but up to kPipe of them are enqueued ahead of the one the host is waiting for, each with
// its own pinned result block and completion word -- the next kernel starts when the previous one retires instead of
// after a host round trip (flag seen, hits copied, next launch: ~8 us per query).
// Round 6, small tables (lanes_apply): consecutive queries alternate between the shard's two half-grid lanes, whose
// launches run side by side -- one query's scan overlaps the other's selection.
int search_each_pipelined(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k, uint32_t kout, float cutoff, int metric,
                          float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx)
{
    // every shard of the handle (round 5: a multi-device handle used to pay a host round trip per query -- enqueue on all
    // shards, wait, merge, next query): up to kPipe queries are enqueued ahead on EVERY shard's stream, each with its own
    // pinned block per shard; the host merges query q's blocks while the devices run q + 1 ... q + kPipe - 1
    const size_t nsh = db->shards.size();
    const size_t blk = gsim_result_block_bytes(k);
    std::vector<char> use_lanes(nsh, 0);
    for (size_t i = 0; i < nsh; i++) {
        Shard& s = db->shards[i];
        if (s.nrows && lanes_apply(db, s, k, nq) && ensure_lanes(db, s) == GSIM_OK &&
            (fused_applies(db, s.lanes[0], k) || fused_publish_applies(db, s.lanes[0], k))) // (the half grid's own geometry must carry the route too)
            use_lanes[i] = 1; // (no lanes: the shard itself, as before)
    }
    auto pipe_blocks = [&](Shard& s) -> int {
        GSIM_HIP(set_device(s.device));
        GSIM_HIP(s.h_pipe.grow(blk * kPipe));
        return GSIM_OK;
    };
    for (size_t i = 0; i < nsh; i++) {
        int rc = pipe_blocks(db->shards[i]);
        if (use_lanes[i])
            for (auto& l : db->shards[i].lanes)
                if (rc == GSIM_OK) rc = pipe_blocks(l);
        if (rc != GSIM_OK) return rc;
    }
    // query q of the call on shard i: which search state answers it, and in which of its pipeline slots
    auto state_of = [&](size_t i, uint32_t q) -> Shard& { return use_lanes[i] ? db->shards[i].lanes[q % db->shards[i].lanes.size()] : db->shards[i]; };
    auto slot_of = [&](size_t i, uint32_t q) -> uint32_t { return (use_lanes[i] ? q / static_cast<uint32_t>(db->shards[i].lanes.size()) : q) % kPipe; };
    uint32_t issued = 0;
    for (uint32_t done = 0; done < nq; done++) {
        for (; issued < nq && issued - done < static_cast<uint32_t>(kPipe); issued++) {
            for (size_t i = 0; i < nsh; i++) {
                if (db->shards[i].nrows == 0) continue;
                Shard& s = state_of(i, issued);
                const uint32_t slot = slot_of(i, issued);
                const int rc = enqueue_query(db, s, queries + static_cast<size_t>(issued) * db->W, k, cutoff, metric, alpha, beta,
                                             db->row_base + static_cast<uint32_t>(s.first_row), s.h_pipe + slot * blk, true, kAuto, slot);
                if (rc != GSIM_OK) return rc;
                if (use_lanes[i]) db->lane_queries++;
            }
        }
        db->blocks.clear();
        for (size_t i = 0; i < nsh; i++) {
            if (db->shards[i].nrows == 0) continue;
            Shard& s = state_of(i, done);
            const uint32_t slot = slot_of(i, done);
            GSIM_HIP(set_device(s.device));
            void* out = s.h_pipe + slot * blk;
            const int rc = finish_query_sync(db, s, queries + static_cast<size_t>(done) * db->W, k, cutoff, metric, alpha, beta,
                                             db->row_base + static_cast<uint32_t>(s.first_row), out, slot);
            if (rc != GSIM_OK) return rc;
            db->blocks.push_back({out, s.slot[slot].why});
        }
        collect_blocks(db, done, k, hits + static_cast<size_t>(done) * kout, &counts[done], approx ? &approx[done] : nullptr);
    }
    return GSIM_OK;
}

int check_search_args(gsim_db* db, const uint32_t* queries, int metric)
{
    if (!db || !queries) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (!db->finalized) return fail(GSIM_ERR_STATE, "table not finalized (no rows on a GPU)");
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    return GSIM_OK;
}

} // namespace gsim_host

using namespace gsim_host;

// gsim_db_search, and gsim_db_search_each (`each`): its queries one by one, never a shared table pass
static int search_host(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t kout, float cutoff, int metric, float alpha, float beta,
                       gsim_hit* hits, uint32_t* counts, uint64_t* approx, bool each)
{
    int rc = check_search_args(db, queries, metric);
    if (rc != GSIM_OK) return rc;
    if ((!hits && kout && nq) || (!counts && nq)) return fail(GSIM_ERR_INVALID, "NULL output");
    std::lock_guard<std::mutex> guard(db->search_mutex);
    // kout is the stride of the caller's hits array; the search itself never asks for more hits than the
    // table has rows (result blocks, pinned buffers and the select's capacity scale with k: a wild count
    // from a client must not size them)
    const uint32_t k = static_cast<uint32_t>(std::min<uint64_t>(kout, db->nrows));
    const size_t nsh = db->shards.size();
    db->query_flags.assign(db->timing ? nq : 0, 0); // (gsim_debug_query_flags: how each query of this call was routed / re-run)
    if (db->fold > 1) {
        if (metric != GSIM_METRIC_TANIMOTO) return fail(GSIM_ERR_INVALID, "folded tables support Tanimoto only");
        return search_folded(db, queries, nq, kout, cutoff, hits, counts, approx);
    }
    const bool batched = !each && nq >= 4 && k <= static_cast<uint32_t>(gsim::kSelectCap) && k > 0 && gsim::batch_supported(db->W);
    if (batched)
        return db->comm ? search_batch_comm(db, queries, nq, k, kout, cutoff, metric, alpha, beta, hits, counts, approx)
                        : search_batched(db, queries, nq, k, kout, cutoff, metric, alpha, beta, hits, counts, approx);
    if (each && nsh >= 1 && !db->comm && nq > 1 && k > 0 && db->nrows > 0 && !db->shards[0].d_dbg &&
        !db->knobs.fused_debug)
        return search_each_pipelined(db, queries, nq, k, kout, cutoff, metric, alpha, beta, hits, counts, approx);
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t* query = queries + static_cast<size_t>(q) * db->W;
        db->query_flags_at = q;
        rc = search_one(db, query, k, cutoff, metric, alpha, beta, hits + static_cast<size_t>(q) * kout, &counts[q],
                        approx ? &approx[q] : nullptr);
        if (rc != GSIM_OK) return rc;
    }
    return GSIM_OK;
}

extern "C" {

int gsim_db_search(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t kout, float cutoff, int metric,
                   float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx)
{
    return search_host(db, queries, nq, kout, cutoff, metric, alpha, beta, hits, counts, approx, false);
}

int gsim_db_search_timed(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t kout, float cutoff, int metric, float alpha,
                         float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx, double* seconds)
{
    int rc = check_search_args(db, queries, metric);
    if (rc != GSIM_OK) return rc;
    if ((!hits && kout && nq) || (!counts && nq) || (!seconds && nq)) return fail(GSIM_ERR_INVALID, "NULL output");
    if (db->fold > 1) return fail(GSIM_ERR_STATE, "gsim_db_search_timed does not support folded tables");
    std::lock_guard<std::mutex> guard(db->search_mutex);
    const uint32_t k = static_cast<uint32_t>(std::min<uint64_t>(kout, db->nrows));
    db->query_flags.assign(db->timing ? nq : 0, 0);
    for (uint32_t q = 0; q < nq; q++) {
        db->query_flags_at = q;
        const auto t0 = std::chrono::steady_clock::now();
        rc = search_one(db, queries + static_cast<size_t>(q) * db->W, k, cutoff, metric, alpha, beta, hits + static_cast<size_t>(q) * kout,
                        &counts[q], approx ? &approx[q] : nullptr);
        if (rc != GSIM_OK) return rc;
        seconds[q] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return GSIM_OK;
}

int gsim_db_search_each(gsim_db* db, const uint32_t* queries, uint32_t nq, uint32_t k, float cutoff, int metric,
                        float alpha, float beta, gsim_hit* hits, uint32_t* counts, uint64_t* approx)
{
    return search_host(db, queries, nq, k, cutoff, metric, alpha, beta, hits, counts, approx, true);
}

int gsim_db_search_device(gsim_db* db, const uint32_t* query, uint32_t k, float cutoff, int metric, float alpha,
                          float beta, void* d_result)
{
    int rc = check_search_args(db, query, metric);
    if (rc != GSIM_OK) return rc;
    if (!d_result) return fail(GSIM_ERR_INVALID, "d_result is NULL");
    if (db->shards.size() != 1) return fail(GSIM_ERR_STATE, "search_device needs a single-shard handle");
    if (db->fold > 1) return fail(GSIM_ERR_STATE, "search_device does not support folded tables");
    std::lock_guard<std::mutex> guard(db->search_mutex);
    Shard& s = db->shards[0];
    return enqueue_query(db, s, query, k, cutoff, metric, alpha, beta, db->row_base, d_result, false);
}

} // extern "C"
