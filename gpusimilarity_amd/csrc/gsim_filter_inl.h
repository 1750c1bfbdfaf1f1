// gsim_filter_inl.h -- the streaming top-k filter of the four-kernel pipeline's scan (BlockFilter, WaveFilter), shared by the
// kernels that feed compact_kernel / select_kernel: scan_kernel and its siblings (gsim_scan.hip) and the row-set scans
// (gsim_subset.hip).  Moved here verbatim from gsim_scan.hip.  Internal; device code only.
#pragma once

#include "gsim_device_common.h"
#include "gsim_prefilter.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

// Streaming top-k filter.
//
// Every workgroup keeps, in LDS, a histogram `hist` of the coarse bins of the rows
// it has EMITTED (written out as candidates).  From time to time a wave pushes the
// not-yet-pushed part of it into the table-wide histogram `ghist` (global memory,
// device-scope atomics), re-reads `ghist` and derives a threshold bin: the largest
// bin B with at least k counted rows at or above it.  The threshold is published
// with atomicMax (`gtau`) and every wave of every workgroup picks it up on its next
// chunk.  A row is emitted only if bin(score) >= the wave's current threshold.
//
// Why this is exact: `ghist` only ever counts distinct rows of the table that have
// really been scanned, so "k counted rows at or above B" implies that the table's
// k-th best score lies in a bin >= B; a row in a lower bin scores strictly less than
// k other rows and cannot be in the top-k.  Everything is monotone (counts and
// thresholds only grow), so there are no barriers and no ordering requirements:
// a stale (lower) threshold only emits more than necessary, a histogram read while
// others add to it only under-counts.  On a random table the number of emitted rows
// falls from N to roughly k * ln(N / k) + (#workgroups * first push).
struct BlockFilter {
    uint32_t hist[kScanBins];    // rows emitted by this workgroup, per coarse bin
    uint32_t flushed[kScanBins]; // part of hist already added to ghist
    uint32_t tau;                // workgroup's copy of the threshold bin (monotone)
    uint32_t nemit;              // candidates emitted by the workgroup so far
    uint32_t trigger;            // nemit value at which the next push / re-read happens
    uint32_t lock;               // one pusher at a time
    // Per-wave staging of emitted candidates.  Candidates go to LDS (ds_write, lgkmcnt) and
    // reach global memory in bursts of >= 64: a global store inside the streaming loop would be
    // waited for by the loop's next s_waitcnt vmcnt(0) (gfx950 has one counter for loads and
    // stores) -- measured at ~0.36 us per emitting iteration.
    u64 stage_key[kScanBlock / 64][kStage];
    uint32_t stage_cb[kScanBlock / 64][kStage];
};

// first push after this many emitted rows per workgroup (then geometrically)
constexpr uint32_t kFirstPush = 64;

// Per-wave view of the filter (members wave-uniform except `kept`).
struct WaveFilter {
    static constexpr bool kFused = false;
    __device__ __forceinline__ void checkpoint(uint32_t, int) {}
    // Narrow rows (128 ... 512 bits): a wave meets 64 ... 512 rows per load and the score (an f32 divide per row) is most of
    // the kernel -- 20 M x 128-bit rows: 149 us against the 40 us the bytes take.  Without a cutoff only rows that can reach
    // the threshold bin need a score: the division-free test of the single launch (gsim_prefilter.h, proven for rows up to
    // 512 bits), at the lower edge of the bin.  (With a cutoff every row at or above it is counted: all are scored.)
    template <int LPR> __device__ __forceinline__ void offer_counts(bool active, uint32_t row, uint32_t val, const ScanArgs& a, int lane)
    {
        if constexpr (LPR >= 1 && LPR <= 4) {
            if (!has_cutoff && k) { // (wave-uniform)
                if (tau != pk_tau) { // (wave-uniform; the threshold moves a few times per query)
                    pk_tau = tau;
                    const PrefilterConstants pk = prefilter_constants(a.metric == GSIM_METRIC_TVERSKY, a.alpha, a.beta, a.qpop,
                                                                      prefilter_level(true, static_cast<float>(tau) * (1.0f / kScanBins), 0u), true);
                    pk_ka = pk.ka;
                    pk_kb = pk.kb;
                }
                const bool maybe = active && static_cast<float>(val >> 16) >= __builtin_fmaf(pk_kb, static_cast<float>(val & 0xFFFFu), pk_ka);
                if (__ballot(maybe) == 0) return; // no row of this round can reach the threshold bin: none is scored
                active = maybe;                   // (a row the test rejects lies below the bin: not a candidate, and nothing counts it)
            }
        }
        offer_scored(*this, active, row, val, a, lane);
    }
    uint32_t pk_tau;
    float pk_ka, pk_kb;
    BlockFilter* sh;
    QueryState* st;
    u64* seg;         // this wave's private candidate segment (keys)
    uint32_t* seg_cb; // ... and the popcounts the score came from (common << 16 | popc_db)
    u64* stg_key;     // this wave's LDS staging area
    uint32_t* stg_cb;
    uint32_t k, tau, step, cursor, staged, kept;
    float cutoff;
    bool has_cutoff;

    __device__ __forceinline__ void init(BlockFilter* b, QueryState* state, u64* s, uint32_t* scb, uint32_t kk,
                                         float cut)
    {
        sh = b;
        stg_key = b->stage_key[threadIdx.x >> 6];
        stg_cb = b->stage_cb[threadIdx.x >> 6];
        staged = 0;
        st = state;
        seg = s;
        seg_cb = scb;
        k = kk;
        cutoff = cut;
        has_cutoff = cut > 0.0f; // fingerprintdb_cuda.cu:263: compaction only if cutoff > 0
        pk_tau = 0; // (no threshold yet: everything passes)
        pk_ka = 0.0f;
        pk_kb = 0.0f;
        tau = kk ? state->gtau : static_cast<uint32_t>(kScanBins); // gtau: 0, or set by sample_kernel
        step = kk / 8 > 32 ? kk / 8 : 32;
        cursor = 0;
        kept = 0;
    }

    // device-coherent read of the table-wide threshold (issued a chunk ahead of its use)
    __device__ __forceinline__ uint32_t load_gtau() const
    {
        return __hip_atomic_load(&st->gtau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // pick up a threshold raised by another wave (same workgroup: LDS; any workgroup: g)
    __device__ __forceinline__ void refresh(uint32_t g, int lane)
    {
        const uint32_t t = __hip_atomic_load(&sh->tau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        tau = t > tau ? t : tau;
        if (g > tau) { // raised by another workgroup: hand it to the other waves of this one through LDS
            tau = g;
            if (lane == 0) atomicMax(&sh->tau, g);
        }
    }

    // Push this workgroup's new counts into ghist, derive the threshold from ghist.
    __device__ __forceinline__ void push_and_rethreshold(int lane)
    {
        constexpr int PER = kScanBins / 64;
        uint32_t locked = 0;
        if (lane == 0) locked = atomicExch(&sh->lock, 1u);
        locked = __builtin_amdgcn_readfirstlane(locked);
        if (locked == 0) {
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const uint32_t b = static_cast<uint32_t>(lane * PER + i);
                const uint32_t h = __hip_atomic_load(&sh->hist[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const uint32_t fl = sh->flushed[b];
                if (b >= tau && h > fl) {
                    atomicAdd(&st->ghist[b], h - fl);
                    sh->flushed[b] = h;
                }
            }
            if (lane == 0) __hip_atomic_store(&sh->lock, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // threshold from the table-wide histogram: device-coherent (sc1) 16-byte buffer
        // loads, 4 per lane -- 1024 separate 4-byte sc1 loads cost ~20 us per push
        uint32_t h[PER];
        uint32_t s = 0;
        {
            const __amdgpu_buffer_rsrc_t rsrc =
                __builtin_amdgcn_make_buffer_rsrc(st->ghist, 0, kScanBins * 4, 0x00020000);
#pragma unroll
            for (int i = 0; i < PER / 4; i++) {
                const u32x4 v4 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * PER * 4 + i * 16, 0, /*sc1*/ 16);
                h[4 * i + 0] = v4.x;
                h[4 * i + 1] = v4.y;
                h[4 * i + 2] = v4.z;
                h[4 * i + 3] = v4.w;
                s += v4.x + v4.y + v4.z + v4.w;
            }
        }
        uint32_t bin_k, cnt;
        threshold_from_counts<PER>(h, s, k, lane, bin_k, cnt);
        if (cnt >= k) {
            if (lane == 0) {
                atomicMax(&st->gtau, bin_k);
                atomicMax(&sh->tau, bin_k);
            }
            tau = bin_k > tau ? bin_k : tau;
        }
    }

    // staged candidates -> this wave's global segment, coalesced
    __device__ __forceinline__ void flush_stage(int lane)
    {
        for (uint32_t i = lane; i < staged; i += 64) {
            seg[cursor + i] = stg_key[i];
            seg_cb[cursor + i] = stg_cb[i];
        }
        cursor += staged;
        staged = 0;
    }

    // One row per lane (or an inactive lane).
    __device__ __forceinline__ void offer(bool active, uint32_t row, float raw_score, uint32_t cb, int lane)
    {
        const float s = apply_cutoff(raw_score, cutoff);
        const bool keep = active && (!has_cutoff || s != 0.0f);
        kept += keep ? 1u : 0u;
        const uint32_t bin = coarse_bin(s);
        const bool cand = keep && bin >= tau;
        const u64 m = __ballot(cand);
        if (m != 0) {
            if (cand) {
                const uint32_t slot = staged + lane_rank(m);
                stg_key[slot] = make_key(s, row);
                stg_cb[slot] = cb;
                atomicAdd(&sh->hist[bin], 1u); // ds_add_u32
            }
            const uint32_t n = static_cast<uint32_t>(__popcll(m));
            staged += n;
            if (staged > 64) flush_stage(lane);
            uint32_t old = 0;
            if (lane == 0) old = atomicAdd(&sh->nemit, n);
            old = __builtin_amdgcn_readfirstlane(old);
            const uint32_t trig = __hip_atomic_load(&sh->trigger, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (old < trig && old + n >= trig) { // exactly one wave crosses a given trigger
                push_and_rethreshold(lane);
                if (lane == 0) {
                    // next push after 50 % more emitted rows (at least `step`): a handful of pushes per
                    // workgroup and query; the emission rate falls as the threshold rises
                    const uint32_t now = __hip_atomic_load(&sh->nemit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const uint32_t inc = now / 2 > step ? now / 2 : step;
                    __hip_atomic_store(&sh->trigger, now + inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }

    __device__ __forceinline__ void finish(uint32_t w, const ScanArgs& a, int lane)
    {
        if (staged) flush_stage(lane);
        if (lane == 0) {
            a.seg_count[w] = cursor;
            if (cursor) atomicAdd(&a.state->ncand, static_cast<u64>(cursor));
        }
        if (has_cutoff) {
            const uint32_t tot = wave_sum(kept);
            if (lane == 0 && tot) atomicAdd(&a.state->kept, static_cast<u64>(tot));
        }
    }
};

__device__ __forceinline__ void block_filter_init(BlockFilter* sh, uint32_t k, uint32_t tau0)
{
    for (int i = threadIdx.x; i < kScanBins; i += kScanBlock) {
        sh->hist[i] = 0;
        sh->flushed[i] = 0;
    }
    if (threadIdx.x == 0) {
        sh->tau = k ? tau0 : static_cast<uint32_t>(kScanBins);
        sh->nemit = 0;
        sh->trigger = k ? (k < kFirstPush ? k : kFirstPush) : 0xFFFFFFFFu;
        sh->lock = 0;
    }
    __syncthreads();
}

// After every wave of the workgroup is done: whatever has not been pushed yet goes
// into the table-wide histogram, for the bins at or above the final threshold.
// ghist is then exact for every bin >= the largest threshold any wave used, which is
// all K2 needs (see compact_kernel).
__device__ __forceinline__ void block_filter_flush(BlockFilter* sh, const ScanArgs& a)
{
    __syncthreads();
    const uint32_t tau = sh->tau;
    for (int i = threadIdx.x; i < kScanBins; i += kScanBlock) {
        const uint32_t h = sh->hist[i], fl = sh->flushed[i];
        if (static_cast<uint32_t>(i) >= tau && h > fl) atomicAdd(&a.state->ghist[i], h - fl);
    }
}

} // namespace
} // namespace gsim
