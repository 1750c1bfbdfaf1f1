// gsim_maxmin.hip -- MaxMin diversity picking (gsim_db_maxmin): one pass over the table per pick.
//
// Pass p streams the whole table against the row of pick p, through the scan's own loops (gsim_scan_inl.h: scan_rows,
// scan_rows_ragged, scan_rows_wragged -- every width streams the way gsim_db_search's scan does) with MaxMinFilter:
//   * a row's score is score_of(...) of the packed counts, NaN (0/0: two all-zero rows) counted as 0;
//   * maxsim[row] is read, and maxsim / nearest are stored only when the score is strictly greater (after the first few
//     picks that is rare: the state costs ~4 B read per row and pass);
//   * every lane keeps the smallest key (maxsim bits << 32 | row) it has met.  All scores are >= 0, so the u64 order of the
//     keys is (maxsim, row); a picked row holds +inf and never wins, nor is it ever overwritten by a score.
// Selection in the same launch: wave minimum, workgroup minimum, ONE store into the pass's partials, ONE agent-scope ticket
// add; the workgroup whose add returns last -- over all the launches of the pass -- reduces the partials and publishes
// pick p + 1 (picks, pick_scores, the +inf sentinel), then re-zeroes the ticket.  The next pass reads its query row's index
// from picks[p + 1]: no host round trip between picks.  A selector that stops (max_score, or no unpicked row left) sets the
// done word, and every later pass returns after one scalar load.
//
// gsim_maxmin_cached.hip compiles this file again with GSIM_STREAM_LOAD_DEFAULT_POLICY: default-policy table loads for
// tables whose rows and state fit the Infinity Cache, where the pass re-reads them from it.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

constexpr uint32_t kPickedBits = 0x7F800000u; // +inf: the maxsim of a picked row

struct MaxMinFilter {
    static constexpr bool kFused = false;
    float* maxsim;      // this launch's first row (r0)
    uint32_t* nearest;  // ditto, or nullptr
    uint32_t row0;      // r0: the launch's first row in the table (the keys carry table rows)
    uint32_t pick;      // position of this pass's query in picks
    u64 key;            // smallest (maxsim bits << 32 | table row) this lane has met
    uint32_t updated;   // rows whose maxsim this lane raised

    __device__ __forceinline__ void checkpoint(uint32_t, int) {}
    __device__ __forceinline__ uint32_t load_gtau() const { return 0u; }
    __device__ __forceinline__ void refresh(uint32_t, int) {}

    template <int LPR> __device__ __forceinline__ void offer_counts(bool active, uint32_t row, uint32_t val, const ScanArgs& a, int lane)
    {
        if (!active) return;
        float s = score_of(a.metric, a.alpha, a.beta, a.qpop, val & 0xFFFFu, val >> 16);
        s = s == s ? s : 0.0f; // NaN (0/0) counts as 0
        const float m = maxsim[row];
        float now = m;
        if (s > m) { // (+inf: a picked row, never raised)
            now = s;
            maxsim[row] = s;
            if (nearest) nearest[row] = pick;
            updated++;
        }
        const u64 k = (static_cast<u64>(__float_as_uint(now)) << 32) | (row0 + row);
        key = k < key ? k : key;
    }
};

__device__ __forceinline__ u64 wave_min64(u64 v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = static_cast<u64>(__shfl_xor(static_cast<long long>(v), d, 64));
        v = o < v ? o : v;
    }
    return v;
}

// LDS of one workgroup: the waves' minima and counts, the "selector" flag, and (rows of 3 ... 22 words: scan_rows_wragged)
// every wave's word area -- one object, so that nothing else is declared __shared__ beside the streaming loop's area.
template <int NLW> struct MaxMinShared {
    uint32_t words[kScanBlock / 64][NLW ? NLW * 256 : 1];
    u64 key[kScanBlock / 64];
    uint32_t upd[kScanBlock / 64];
    uint32_t last;
};

// KIND 0: scan_rows<LPR, U>; 1: scan_rows_ragged<LPR, U>; 2: scan_rows_wragged<LPR, U> (LPR = words per row); 3: generic.
template <int KIND, int LPR, int U>
__global__ __launch_bounds__(kScanBlock) void maxmin_kernel(MaxMinArgs m, ScanGeometry g, u64 r0, u64 nrows, uint32_t wg0, uint32_t p)
{
    constexpr int NLW = KIND == 2 ? (LPR % 2 ? LPR : LPR / 2) * U : 0;
    __shared__ MaxMinShared<NLW> sh;
    if (m.ctl[kMaxMinDone]) return; // picking ended in an earlier pass
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (tid >> 6));

    // the query: the row of pick p, resolved here from what the host (seeds, pick 0) or the previous pass wrote
    const uint32_t* qrow = static_cast<const uint32_t*>(m.rows) + static_cast<u64>(m.picks[p]) * m.W;
    uint32_t qp = 0;
    for (uint32_t i = static_cast<uint32_t>(lane); i < m.W; i += 64u) qp += __popc(qrow[i]);
    ScanArgs a{};
    a.rows = static_cast<const uint32_t*>(m.rows) + r0 * m.W;
    a.nrows = nrows;
    a.W = m.W;
    a.query = qrow;
    a.qpop = wave_sum(qp);
    a.metric = m.metric;
    a.alpha = m.alpha;
    a.beta = m.beta;

    MaxMinFilter f;
    f.maxsim = m.maxsim + r0;
    f.nearest = m.nearest ? m.nearest + r0 : nullptr;
    f.row0 = static_cast<uint32_t>(r0);
    f.pick = p;
    f.key = ~0ull;
    f.updated = 0;
    if constexpr (KIND == 0) {
        const u32x4 q = reinterpret_cast<const u32x4*>(qrow)[lane % LPR];
        scan_rows<LPR, U>(a, g, f, q, w, lane);
    } else if constexpr (KIND == 1) {
        scan_rows_ragged<LPR, U>(a, g, f, w, lane);
    } else if constexpr (KIND == 2) {
        scan_rows_wragged<LPR, U>(a, g, f, w, lane, sh.words[wv]);
    } else {
        scan_rows_lane(a, g, f, w, lane);
    }

    const u64 k = wave_min64(f.key);
    const uint32_t u = wave_sum(f.updated);
    if (lane == 0) {
        sh.key[wv] = k;
        sh.upd[wv] = u;
    }
    __syncthreads();
    if (tid == 0) {
        u64 kb = sh.key[0];
        uint32_t ub = sh.upd[0];
        for (int i = 1; i < kScanBlock / 64; i++) {
            kb = sh.key[i] < kb ? sh.key[i] : kb;
            ub += sh.upd[i];
        }
        if (ub) atomicAdd(reinterpret_cast<unsigned long long*>(m.ctl + kMaxMinUpdated), static_cast<u64>(ub));
        m.partials[wg0 + blockIdx.x] = kb;
    }
    if (p + 1 >= m.npicks) return; // the last pick's pass (row_score / nearest only): nothing to select

    // Last arriver (the split-K hand-off in its counter form): every wave's stores done, a workgroup barrier, one
    // agent-scope release, the ticket; the selector acquires before it reads anything another workgroup wrote.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(m.ctl + kMaxMinTicket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh.last = t == m.nwg_total - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!sh.last) return;
    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    u64 best = ~0ull;
    for (uint32_t i = static_cast<uint32_t>(tid); i < m.nwg_total; i += kScanBlock) {
        const u64 x = m.partials[i];
        best = x < best ? x : best;
    }
    best = wave_min64(best);
    __syncthreads(); // (sh.key is read again)
    if (lane == 0) sh.key[wv] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int i = 1; i < kScanBlock / 64; i++) best = sh.key[i] < best ? sh.key[i] : best;
    m.ctl[kMaxMinTicket] = 0u; // (every workgroup of this pass has added: the next pass starts from zero)
    const uint32_t j = p + 1;
    if (j < m.nseeds) { // the next pick is a seed: its score is its maxsim now
        const uint32_t r = m.picks[j];
        m.pick_scores[j] = m.maxsim[r];
        m.maxsim[r] = __uint_as_float(kPickedBits);
        m.ctl[kMaxMinPicked] = j + 1u;
        return;
    }
    const uint32_t bits = static_cast<uint32_t>(best >> 32);
    const float s = __uint_as_float(bits);
    if (bits >= kPickedBits || s > m.max_score) { // every row picked, or the best candidate is too similar: stop
        m.ctl[kMaxMinDone] = 1u;
        return;
    }
    const uint32_t r = static_cast<uint32_t>(best);
    m.picks[j] = r;
    m.pick_scores[j] = s;
    m.maxsim[r] = __uint_as_float(kPickedBits);
    m.ctl[kMaxMinPicked] = j + 1u;
}

template <int KIND, int LPR, int U>
hipError_t launch_t(const MaxMinArgs& m, const ScanGeometry& g, u64 r0, u64 nrows, uint32_t wg0, uint32_t p, hipStream_t s)
{
    hipLaunchKernelGGL((maxmin_kernel<KIND, LPR, U>), dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, m, g, r0, nrows, wg0, p);
    return hipGetLastError();
}

} // namespace

#ifdef GSIM_STREAM_LOAD_DEFAULT_POLICY
hipError_t launch_maxmin_pass_cached(const MaxMinArgs& m, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t wg0, uint32_t p,
                                     hipStream_t s)
#else
ScanGeometry maxmin_geometry(uint64_t nrows, uint32_t W, int num_cus)
{
    ScanGeometry g{};
    if (fused_word_geometry(nrows, W, num_cus, &g)) return g; // rows of 3 ... 11 or twice that many words
    g = scan_geometry(nrows, W, num_cus, 4, 8);
    if (g.lanes_per_row != 0 || g.ragged_loads != 0) return g;
    // generic: one row per lane, 64 rows per wave and trip; four waves per CU
    g = ScanGeometry{};
    g.unroll = 1;
    g.chunk_rows = 64;
    g.nchunks = (nrows + 63) / 64;
    uint64_t nw = static_cast<uint64_t>(num_cus) * 4u;
    if (nw > g.nchunks) nw = g.nchunks;
    if (nw < 1) nw = 1;
    g.nwaves = static_cast<uint32_t>((nw + 3) / 4 * 4);
    return g;
}

hipError_t launch_maxmin_pass(const MaxMinArgs& m, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t wg0, uint32_t p, hipStream_t s)
#endif
{
#define GSIM_CASE(L) \
    if (g.lanes_per_row == L && g.unroll == 8) return launch_t<0, L, 8>(m, g, r0, nrows, wg0, p, s);
    GSIM_CASE(1)
    GSIM_CASE(2)
    GSIM_CASE(4)
    GSIM_CASE(8)
    GSIM_CASE(16)
    GSIM_CASE(32)
    GSIM_CASE(64)
#undef GSIM_CASE
    if (g.lanes_per_row != 0) return hipErrorInvalidValue;
    if (g.ragged_words) {
        switch (m.W) {
        case 3: return launch_t<2, 3, 3>(m, g, r0, nrows, wg0, p, s);
        case 5: return launch_t<2, 5, 2>(m, g, r0, nrows, wg0, p, s);
        case 7: return launch_t<2, 7, 1>(m, g, r0, nrows, wg0, p, s);
        case 6: return launch_t<2, 6, 3>(m, g, r0, nrows, wg0, p, s);
        case 10: return launch_t<2, 10, 2>(m, g, r0, nrows, wg0, p, s);
        case 14: return launch_t<2, 14, 1>(m, g, r0, nrows, wg0, p, s);
        case 9: return launch_t<2, 9, 1>(m, g, r0, nrows, wg0, p, s);
        case 18: return launch_t<2, 18, 1>(m, g, r0, nrows, wg0, p, s);
        case 11: return launch_t<2, 11, 1>(m, g, r0, nrows, wg0, p, s);
        case 22: return launch_t<2, 22, 1>(m, g, r0, nrows, wg0, p, s);
        default: return hipErrorInvalidValue;
        }
    }
    switch (g.ragged_loads) {
    case 0: return launch_t<3, 0, 1>(m, g, r0, nrows, wg0, p, s);
    case 3: return launch_t<1, 3, 3>(m, g, r0, nrows, wg0, p, s);
    case 5: return launch_t<1, 5, 2>(m, g, r0, nrows, wg0, p, s);
    case 7: return launch_t<1, 7, 1>(m, g, r0, nrows, wg0, p, s);
    case 9: return launch_t<1, 9, 1>(m, g, r0, nrows, wg0, p, s);
    case 11: return launch_t<1, 11, 1>(m, g, r0, nrows, wg0, p, s);
    case 13: return launch_t<1, 13, 1>(m, g, r0, nrows, wg0, p, s);
    case 15: return launch_t<1, 15, 1>(m, g, r0, nrows, wg0, p, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace gsim
