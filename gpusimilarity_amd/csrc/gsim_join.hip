// gsim_join.hip -- threshold joins (gsim_db_join, gsim_db_join_queries), the streaming route: one pass over the table per
// left row, for calls with few left rows.  (Calls with many take the tile kernel of gsim_neighbors.hip, launch_join_tiles.)
//
// A pass streams the table against its left row through the scan's own loops (gsim_scan_inl.h: scan_rows, scan_rows_ragged,
// scan_rows_wragged, scan_rows_lane -- every width streams the way gsim_db_search's scan does) with JoinFilter:
//   * a row's score is score_of(...) of the packed counts; it is kept when score >= cutoff (NaN, 0/0, never is);
//   * kept rows go to the wave's staging area in LDS as {table row, score bits}.  Nothing kept, nothing issued: the loop
//     stays free of global traffic, and the prefetched chunk is the only thing its waits cover;
//   * the area is flushed when fewer than 64 free slots remain, and once after the loop: ONE cursor atomic for all the staged
//     rows, then the keys ((left row << 32) | table row) and scores stored, 64 per trip.  The cursor keeps counting past the
//     buffer's capacity, as the tile kernel's does: the host grows the buffer to the exact size and runs the launches that
//     overflowed once more (capi_pairs.cpp).
// The order in which waves append is not fixed; the sort by (left row, table row) behind it is what makes the output
// byte-identical from run to run -- the keys are unique.
//
// GSIM_JOIN_BY_SCORE: rocPRIM's radix sort is stable, so sorting the (left, column)-ordered pairs once more by
// (left, inverted score bits) leaves every list by (score descending, column ascending): gsim_db_search's order.  Scores are
// >= 0, so their bit patterns order as integers.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

constexpr uint32_t kJoinStage = 256; // kept rows a wave stages in LDS between two cursor atomics (an offer adds up to 64)

struct JoinFilter {
    static constexpr bool kFused = false;
    uint2* stage;    // this wave's staging area: {table row, score bits}
    uint32_t n;      // entries staged (wave-uniform)
    uint32_t row0;   // the launch's first row in the table (the keys carry table rows)
    u64 left;        // left row << 32
    float cutoff;
    u64* keys;
    float* vals;
    u64* cursor;
    u64 cap;

    __device__ __forceinline__ void checkpoint(uint32_t, int) {}
    __device__ __forceinline__ uint32_t load_gtau() const { return 0u; }
    __device__ __forceinline__ void refresh(uint32_t, int) {}

    __device__ __forceinline__ void flush(int lane)
    {
        if (n == 0) return;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(cursor, static_cast<u64>(n));
        base = (static_cast<u64>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base >> 32)))) << 32) |
               static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base & 0xFFFFFFFFull)));
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier(); // (one wave: its LDS operations execute in order)
        for (uint32_t i = static_cast<uint32_t>(lane); i < n; i += 64u) {
            const uint2 e = stage[i];
            const u64 pos = base + i;
            if (pos < cap) {
                keys[pos] = left | e.x;
                vals[pos] = __uint_as_float(e.y);
            }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier(); // the next offers overwrite the area
        n = 0;
    }

    // (called by all 64 lanes together: every streaming loop offers under wave-uniform control flow)
    template <int LPR> __device__ __forceinline__ void offer_counts(bool active, uint32_t row, uint32_t val, const ScanArgs& a, int lane)
    {
        const float s = score_of(a.metric, a.alpha, a.beta, a.qpop, val & 0xFFFFu, val >> 16);
        const bool keep = active && s >= cutoff; // (NaN: never)
        const u64 m = __ballot(keep);
        if (m == 0) return;
        if (keep) stage[n + lane_rank(m)] = make_uint2(row0 + row, __float_as_uint(s));
        n += static_cast<uint32_t>(__popcll(m));
        if (n > kJoinStage - 64u) flush(lane);
    }
};

// LDS of one workgroup: every wave's staging area and (rows of 3 ... 22 words: scan_rows_wragged) every wave's word area --
// one object, so that nothing else is declared __shared__ beside the streaming loop's area.
template <int NLW> struct JoinShared {
    uint32_t words[kScanBlock / 64][NLW ? NLW * 256 : 1];
    uint2 stage[kScanBlock / 64][kJoinStage];
};

// KIND 0: scan_rows<LPR, U>; 1: scan_rows_ragged<LPR, U>; 2: scan_rows_wragged<LPR, U> (LPR = words per row); 3: scan_rows_lane.
template <int KIND, int LPR, int U>
__global__ __launch_bounds__(kScanBlock) void join_kernel(JoinArgs j, ScanGeometry g, u64 r0, u64 nrows, uint32_t l)
{
    constexpr int NLW = KIND == 2 ? (LPR % 2 ? LPR : LPR / 2) * U : 0;
    __shared__ JoinShared<NLW> sh;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (tid >> 6));

    const uint32_t* qrow = j.left + static_cast<u64>(l) * j.W;
    uint32_t qp = 0;
    for (uint32_t i = static_cast<uint32_t>(lane); i < j.W; i += 64u) qp += __popc(qrow[i]);
    ScanArgs a{};
    a.rows = static_cast<const uint32_t*>(j.rows) + r0 * j.W;
    a.nrows = nrows;
    a.W = j.W;
    a.query = qrow;
    a.qpop = wave_sum(qp);
    a.metric = j.metric;
    a.alpha = j.alpha;
    a.beta = j.beta;

    JoinFilter f;
    f.stage = sh.stage[wv];
    f.n = 0;
    f.row0 = static_cast<uint32_t>(r0);
    f.left = static_cast<u64>(l) << 32;
    f.cutoff = j.cutoff;
    f.keys = j.keys;
    f.vals = j.vals;
    f.cursor = j.cursor;
    f.cap = j.cap;
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
    f.flush(lane);
}

template <int KIND, int LPR, int U>
hipError_t launch_t(const JoinArgs& j, const ScanGeometry& g, u64 r0, u64 nrows, uint32_t l, hipStream_t s)
{
    hipLaunchKernelGGL((join_kernel<KIND, LPR, U>), dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, j, g, r0, nrows, l);
    return hipGetLastError();
}

// the (left, column)-sorted pairs -> sort keys of the second pass, in place: key = left << 32 | ~score bits, value = column
__global__ __launch_bounds__(256) void join_score_keys_kernel(u64* __restrict__ keys, uint32_t* __restrict__ vals, u64 n)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= n) return;
    const u64 k = keys[t];
    const uint32_t bits = vals[t];
    keys[t] = (k & 0xFFFFFFFF00000000ull) | static_cast<uint32_t>(~bits);
    vals[t] = static_cast<uint32_t>(k);
}

// ... and the CSR from them (nbr_csr_kernel's scheme: every output by its own thread)
__global__ __launch_bounds__(256) void join_score_csr_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ cols, u64 n,
                                                             u64 nrows_out, uint32_t row_base, u64* __restrict__ indptr,
                                                             uint32_t* __restrict__ indices, float* __restrict__ scores)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (t <= nrows_out) {
        u64 lo = 0, hi = n;
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if ((keys[mid] >> 32) < t) lo = mid + 1;
            else hi = mid;
        }
        indptr[t] = lo;
    }
    if (t < n) {
        indices[t] = cols[t] + row_base;
        scores[t] = __uint_as_float(~static_cast<uint32_t>(keys[t]));
    }
}

} // namespace

hipError_t launch_join_pass(const JoinArgs& m, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t p, hipStream_t s)
{
#define GSIM_CASE(L) \
    if (g.lanes_per_row == L && g.unroll == 8) return launch_t<0, L, 8>(m, g, r0, nrows, p, s);
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
        case 3: return launch_t<2, 3, 3>(m, g, r0, nrows, p, s);
        case 5: return launch_t<2, 5, 2>(m, g, r0, nrows, p, s);
        case 7: return launch_t<2, 7, 1>(m, g, r0, nrows, p, s);
        case 6: return launch_t<2, 6, 3>(m, g, r0, nrows, p, s);
        case 10: return launch_t<2, 10, 2>(m, g, r0, nrows, p, s);
        case 14: return launch_t<2, 14, 1>(m, g, r0, nrows, p, s);
        case 9: return launch_t<2, 9, 1>(m, g, r0, nrows, p, s);
        case 18: return launch_t<2, 18, 1>(m, g, r0, nrows, p, s);
        case 11: return launch_t<2, 11, 1>(m, g, r0, nrows, p, s);
        case 22: return launch_t<2, 22, 1>(m, g, r0, nrows, p, s);
        default: return hipErrorInvalidValue;
        }
    }
    switch (g.ragged_loads) {
    case 0: return launch_t<3, 0, 1>(m, g, r0, nrows, p, s);
    case 3: return launch_t<1, 3, 3>(m, g, r0, nrows, p, s);
    case 5: return launch_t<1, 5, 2>(m, g, r0, nrows, p, s);
    case 7: return launch_t<1, 7, 1>(m, g, r0, nrows, p, s);
    case 9: return launch_t<1, 9, 1>(m, g, r0, nrows, p, s);
    case 11: return launch_t<1, 11, 1>(m, g, r0, nrows, p, s);
    case 13: return launch_t<1, 13, 1>(m, g, r0, nrows, p, s);
    case 15: return launch_t<1, 15, 1>(m, g, r0, nrows, p, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t join_score_sort_bytes(uint64_t n, uint32_t end_bit, size_t* bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<const u64*>(nullptr), static_cast<u64*>(nullptr),
                                     static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<size_t>(n), 0u,
                                     end_bit);
}

hipError_t launch_join_by_score(void* tmp, size_t tmp_bytes, unsigned long long* keys, float* scores, unsigned long long* keys_tmp,
                                uint32_t* cols_tmp, uint64_t n, uint32_t end_bit, uint64_t nrows_out, uint32_t row_base, uint64_t* indptr,
                                uint32_t* indices, float* scores_out, hipStream_t s)
{
    uint32_t* vals = reinterpret_cast<uint32_t*>(scores);
    if (n) {
        hipLaunchKernelGGL(join_score_keys_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<u64*>(keys),
                           vals, static_cast<u64>(n));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        size_t bytes = tmp_bytes;
        e = rocprim::radix_sort_pairs(tmp, bytes, reinterpret_cast<const u64*>(keys), reinterpret_cast<u64*>(keys_tmp),
                                      static_cast<const uint32_t*>(vals), cols_tmp, static_cast<size_t>(n), 0u, end_bit, s);
        if (e != hipSuccess) return e;
    }
    const u64 threads = n > nrows_out + 1 ? n : nrows_out + 1;
    hipLaunchKernelGGL(join_score_csr_kernel, dim3(static_cast<uint32_t>((threads + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const u64*>(keys_tmp), static_cast<const uint32_t*>(cols_tmp), static_cast<u64>(n),
                       static_cast<u64>(nrows_out), row_base, reinterpret_cast<u64*>(indptr), indices, scores_out);
    return hipGetLastError();
}

} // namespace gsim
