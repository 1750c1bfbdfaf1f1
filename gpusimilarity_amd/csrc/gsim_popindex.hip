// gsim_popindex.hip -- popcount indexes (gsim_popindex_*, gsim_db_search_bounded): the table's rows ordered by popcount, and the
// scan of a window of that order.
//
// A query with a bits set and a row with b bits set share c bits, max(0, a + b - fp_bits) <= c <= min(a, b), so the row's score is at
// most ub[b] = the largest score_of(a, b, c) over that range -- found by enumeration with the scan's own arithmetic, hence exact for
// every metric, f32 roundings included (popindex_bounds_kernel).  With the rows sorted by (popcount, row) the rows that can reach a
// score are a contiguous window of the order; the host (capi_popindex.cpp) picks the windows, this file builds the order and scans.
//   popindex_popc_kernel     one streaming pass over the table (16 B per lane, non-temporal): a 16-bit popcount per row and the
//                            histogram of the popcounts, kept in LDS and flushed once per workgroup
//   rocPRIM                  a stable radix sort of (popcount, row) over the popcount's significant bits: `order`; an exclusive scan
//                            of the histogram: `first`
//   popindex_bounds_kernel   ub[0 .. fp_bits] of one query popcount, thread b enumerating c
//   popindex_scan_kernel     slots [lo, lo + n) of the popcount-ordered COPY of the rows, streamed as scan_kernel streams the table
//                            (group-of-lanes loads, the next chunk's loads in flight while the current one is reduced: v_and +
//                            v_bcnt + group_sum, as reduce_chunk); slot i is offered to WaveFilter as row order[i], 4 bytes a row
//                            read a chunk ahead, as subset_gather_kernel reads its list.  Widths without a power-of-two number of
//                            16-byte units: one slot per lane (subset_gather_lane_kernel's arithmetic).  What it leaves is what
//                            scan_kernel leaves: the four-kernel pipeline's tail runs behind it unchanged.
// Without the copy a window is gathered through `order` by gsim_subset.hip's launch_subset_gather; the copy itself is made by
// gsim_label_sums.hip's launch_lsum_gather.
// Seeding: none, as the row-set scans: gtau starts at 0 and rises through ghist, which counts window rows only.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_filter_inl.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

// ---------------------------------------------------------------------------
// building the index
// ---------------------------------------------------------------------------

constexpr int kPopcBlock = 256;
constexpr int kPopcUnroll = 8; // 16-byte loads in flight per lane, as the scan

// the workgroup's histogram: LDS bins (nbins <= kPopcLdsBins) or, for wider rows, the global bins themselves
struct PopcBins {
    uint32_t* lds;
    uint32_t* global;
    __device__ __forceinline__ void add(uint32_t b)
    {
        if (lds) atomicAdd(&lds[b], 1u);
        else atomicAdd(&global[b], 1u);
    }
};

__device__ __forceinline__ PopcBins popc_bins_init(uint32_t* s_hist, uint32_t* hist, uint32_t nbins)
{
    const bool in_lds = nbins <= kPopcLdsBins; // (uniform over the grid)
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < nbins; i += kPopcBlock) s_hist[i] = 0;
        __syncthreads();
    }
    return PopcBins{in_lds ? s_hist : nullptr, hist};
}

__device__ __forceinline__ void popc_bins_flush(const PopcBins& bins, uint32_t nbins)
{
    if (!bins.lds) return;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nbins; i += kPopcBlock) {
        const uint32_t h = bins.lds[i];
        if (h) atomicAdd(&bins.global[i], h);
    }
}

// Rows of LPR sixteen-byte units, LPR a power of two up to 64: chunks of kPopcUnroll x 64 / LPR rows, wave w takes chunks w, w + nwaves, ...
template <int LPR>
__global__ __launch_bounds__(kPopcBlock) void popindex_popc_kernel(const u32x4* __restrict__ rows, u64 nrows, uint16_t* __restrict__ popc,
                                                                   uint32_t* __restrict__ hist, uint32_t nbins)
{
    __shared__ uint32_t s_hist[kPopcLdsBins];
    PopcBins bins = popc_bins_init(s_hist, hist, nbins);
    constexpr int RPL = 64 / LPR;
    constexpr int CH = kPopcUnroll * RPL;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, grp = lane / LPR;
    const u64 w = static_cast<u64>(blockIdx.x) * (kPopcBlock / 64) + (threadIdx.x >> 6);
    const u64 nwaves = static_cast<u64>(gridDim.x) * (kPopcBlock / 64);
    const u64 nchunks = (nrows + CH - 1) / CH;
    for (u64 c = w; c < nchunks; c += nwaves) {
        u32x4 d[kPopcUnroll];
#pragma unroll
        for (int j = 0; j < kPopcUnroll; j++) {
            const u64 row = c * CH + static_cast<u64>(j * RPL + grp);
            d[j] = row < nrows ? stream_load(rows + row * LPR + sub) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int j = 0; j < kPopcUnroll; j++) {
            const u64 row = c * CH + static_cast<u64>(j * RPL + grp);
            const uint32_t bb = group_sum<LPR>(__popc(d[j].x) + __popc(d[j].y) + __popc(d[j].z) + __popc(d[j].w));
            if (sub == 0 && row < nrows) {
                popc[row] = static_cast<uint16_t>(bb);
                bins.add(bb);
            }
        }
    }
    popc_bins_flush(bins, nbins);
}

// Every other width.  Rows of fewer than 32 words: one row per lane, word by word (scan_rows_lane's arithmetic); wider rows: one row
// per wave, the lanes striding over its words.
__global__ __launch_bounds__(kPopcBlock) void popindex_popc_generic_kernel(const uint32_t* __restrict__ rows, u64 nrows, uint32_t W,
                                                                           uint16_t* __restrict__ popc, uint32_t* __restrict__ hist, uint32_t nbins)
{
    __shared__ uint32_t s_hist[kPopcLdsBins];
    PopcBins bins = popc_bins_init(s_hist, hist, nbins);
    const int lane = threadIdx.x & 63;
    const u64 w = static_cast<u64>(blockIdx.x) * (kPopcBlock / 64) + (threadIdx.x >> 6);
    const u64 nwaves = static_cast<u64>(gridDim.x) * (kPopcBlock / 64);
    if (W < 32u) {
        for (u64 r0 = w * 64u; r0 < nrows; r0 += nwaves * 64u) {
            const u64 row = r0 + static_cast<u64>(lane);
            if (row < nrows) {
                const uint32_t* r = rows + row * W;
                uint32_t bb = 0;
                for (uint32_t i = 0; i < W; i++) bb += __popc(r[i]);
                popc[row] = static_cast<uint16_t>(bb);
                bins.add(bb);
            }
        }
    } else {
        for (u64 row = w; row < nrows; row += nwaves) {
            const uint32_t* r = rows + row * W;
            uint32_t bb = 0;
            for (uint32_t i = static_cast<uint32_t>(lane); i < W; i += 64u) bb += __popc(__builtin_nontemporal_load(r + i));
            bb = wave_sum(bb);
            if (lane == 0) {
                popc[row] = static_cast<uint16_t>(bb);
                bins.add(bb);
            }
        }
    }
    popc_bins_flush(bins, nbins);
}

template <int LPR>
hipError_t launch_popc_t(const void* rows, uint64_t nrows, uint16_t* popc, uint32_t* hist, uint32_t nbins, uint32_t blocks, hipStream_t s)
{
    hipLaunchKernelGGL((popindex_popc_kernel<LPR>), dim3(blocks), dim3(kPopcBlock), 0, s, static_cast<const u32x4*>(rows), static_cast<u64>(nrows), popc,
                       hist, nbins);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// the bound
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void popindex_bounds_kernel(uint32_t fp_bits, uint32_t qa, int metric, float alpha, float beta, float* __restrict__ ub)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b > fp_bits) return;
    const uint32_t c0 = qa + b > fp_bits ? qa + b - fp_bits : 0u;
    const uint32_t c1 = qa < b ? qa : b;
    float m = -__builtin_inff();
    for (uint32_t c = c0; c <= c1; c++) {
        float s = score_of(metric, alpha, beta, qa, b, c);
        s = s == s ? s : 0.0f; // (NaN, 0 / 0: taken as 0, as apply_cutoff takes it)
        m = s > m ? s : m;
    }
    ub[b] = m;
}

// ---------------------------------------------------------------------------
// the window scan
// ---------------------------------------------------------------------------

// reduce_chunk for the slots of a window: load j of lane (grp, sub) holds unit `sub` of slot e0 + j * RPL + grp, whose row is ix[j]
template <int LPR, int U, bool FULL, typename Filter>
__device__ __forceinline__ void window_reduce(const u32x4 (&d)[U], const uint32_t (&ix)[U], const u32x4& q, u64 e0, uint32_t n, const ScanArgs& a,
                                              Filter& f, int lane)
{
    constexpr int RPL = 64 / LPR;
    constexpr int ROUNDS = (U + LPR - 1) / LPR;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    uint32_t v[U];
#pragma unroll
    for (int j = 0; j < U; j++) {
        const uint32_t cc = __popc(d[j].x & q.x) + __popc(d[j].y & q.y) + __popc(d[j].z & q.z) + __popc(d[j].w & q.w);
        const uint32_t bb = __popc(d[j].x) + __popc(d[j].y) + __popc(d[j].z) + __popc(d[j].w);
        v[j] = group_sum<LPR>((cc << 16) + bb);
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        // lane (grp, sub) takes the slot of load j = r * LPR + sub
        uint32_t val = 0, row = 0;
#pragma unroll
        for (int jj = 0; jj < U; jj++) {
            if (jj / LPR == r) {
                val = (sub == jj % LPR) ? v[jj] : val;
                row = (sub == jj % LPR) ? ix[jj] : row;
            }
        }
        const int j = r * LPR + sub;
        const bool active = (j < U) && (FULL || e0 + static_cast<u64>(j * RPL + grp) < n);
        f.template offer_counts<LPR>(active, row, val, a, lane);
    }
}

// One wavefront over the window: chunks w, w + nwaves, ... of CH = U * 64 / LPR slots, counted from the window's first slot (`db`
// and `list` point there: any lo is a whole number of 16-byte units into the copy).  Per trip: the row numbers and the rows of the
// next chunk are issued, then the current chunk is reduced -- scan_rows with 4 more bytes a row.
template <int LPR, int U, typename Filter>
__device__ __forceinline__ void window_rows(const ScanArgs& a, const ScanGeometry& g, Filter& f, const u32x4& q, const u32x4* __restrict__ db,
                                            const uint32_t* __restrict__ list, uint32_t n, uint32_t w, int lane)
{
    constexpr int RPL = 64 / LPR;
    constexpr int CH = U * RPL;
    const int grp = lane / LPR;
    uint32_t gt = 0;
    uint32_t trip = 0;
    const uint32_t wib = w % (kScanBlock / 64);

    const u64 nfull = n / CH; // chunks with all CH slots present
    if (w < nfull) {
        const u64 last = w + (nfull - 1 - w) / g.nwaves * g.nwaves; // this wave's last full chunk
        uint32_t ixn[U];
        u32x4 nxt[U];
        {
            const uint32_t* p = list + static_cast<u64>(w) * CH + grp;
#pragma unroll
            for (int j = 0; j < U; j++) ixn[j] = p[j * RPL];
            const u32x4* pd = db + static_cast<u64>(w) * (CH * LPR) + lane;
#pragma unroll
            for (int j = 0; j < U; j++) nxt[j] = stream_load(pd + j * 64);
        }
        for (u64 c = w;; c += g.nwaves) {
            u32x4 d[U];
            uint32_t ix[U];
#pragma unroll
            for (int j = 0; j < U; j++) {
                d[j] = nxt[j];
                ix[j] = ixn[j];
            }
            // prefetch; on the final trip it re-reads the last chunk (no branch in the body)
            const u64 cn = c + g.nwaves <= last ? c + g.nwaves : last;
            const uint32_t* p = list + cn * CH + grp;
#pragma unroll
            for (int j = 0; j < U; j++) ixn[j] = p[j * RPL];
            const u32x4* pd = db + cn * (CH * LPR) + lane;
#pragma unroll
            for (int j = 0; j < U; j++) nxt[j] = stream_load(pd + j * 64);
            f.refresh(gt, lane);
            { // the threshold poll of scan_rows
                const uint32_t period = trip < 64u ? 8u : (trip < 512u ? 32u : 128u);
                if ((trip & (period - 1u)) == 0 && ((trip / period) & (kScanBlock / 64 - 1)) == wib) gt = f.load_gtau();
                trip++;
            }
            window_reduce<LPR, U, true>(d, ix, q, c * CH, n, a, f, lane);
            if (c == last) break;
        }
    }
    if (nfull * CH < n && w == nfull % g.nwaves) { // the window's partial last chunk (a window shorter than a chunk: its only one)
        const u64 e0 = nfull * CH;
        uint32_t ix[U];
        u32x4 d[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const u64 e = e0 + static_cast<u64>(j * RPL + grp);
            ix[j] = e < n ? list[e] : 0u;
            d[j] = e < n ? stream_load(db + e0 * LPR + lane + j * 64) : u32x4{0, 0, 0, 0};
        }
        f.refresh(f.load_gtau(), lane);
        window_reduce<LPR, U, false>(d, ix, q, e0, n, a, f, lane);
    }
}

template <int LPR, int U>
__global__ __launch_bounds__(kScanBlock) void popindex_scan_kernel(ScanArgs a, ScanGeometry g, const uint32_t* order, u64 lo, uint32_t n)
{
    __shared__ BlockFilter s_filter;
    if (a.gate && *a.gate == 0) return;
    const int lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (threadIdx.x >> 6));
    block_filter_init(&s_filter, a.k, a.state->gtau);
    const u32x4 q = reinterpret_cast<const u32x4*>(a.query)[lane % LPR];
    WaveFilter f;
    f.init(&s_filter, a.state, a.cand + static_cast<u64>(w) * g.seg_cap, a.cand_cb + static_cast<u64>(w) * g.seg_cap, a.k, a.cutoff);
    window_rows<LPR, U>(a, g, f, q, reinterpret_cast<const u32x4*>(a.rows) + lo * LPR, order + lo, n, w, lane);
    f.finish(w, a, lane);
    block_filter_flush(&s_filter, a);
}

// Every other width: one slot per lane, word by word, 64 slots per trip.
__global__ __launch_bounds__(kScanBlock) void popindex_scan_lane_kernel(ScanArgs a, ScanGeometry g, const uint32_t* order, u64 lo, uint32_t n)
{
    __shared__ BlockFilter s_filter;
    if (a.gate && *a.gate == 0) return;
    const int lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (threadIdx.x >> 6));
    block_filter_init(&s_filter, a.k, a.state->gtau);
    WaveFilter f;
    f.init(&s_filter, a.state, a.cand + static_cast<u64>(w) * g.seg_cap, a.cand_cb + static_cast<u64>(w) * g.seg_cap, a.k, a.cutoff);
    const uint32_t* db = static_cast<const uint32_t*>(a.rows) + lo * a.W;
    const uint32_t* list = order + lo;
    for (u64 c = w; c < g.nchunks; c += g.nwaves) {
        const u64 e = c * 64u + static_cast<uint32_t>(lane);
        const bool active = e < n;
        const uint32_t row = active ? list[e] : 0u;
        uint32_t cc = 0, bb = 0;
        if (active) {
            const uint32_t* r = db + e * a.W;
            for (uint32_t i = 0; i < a.W; i++) {
                const uint32_t x = r[i];
                cc += __popc(x & a.query[i]);
                bb += __popc(x);
            }
        }
        f.refresh((c / g.nwaves) % 8 == 0 ? f.load_gtau() : 0u, lane);
        f.template offer_counts<64>(active, row, (cc << 16) + bb, a, lane);
    }
    f.finish(w, a, lane);
    block_filter_flush(&s_filter, a);
}

template <int LPR, int U>
hipError_t launch_window_t(const ScanArgs& a, const ScanGeometry& g, const uint32_t* order, uint64_t lo, uint32_t n, hipStream_t s)
{
    hipLaunchKernelGGL((popindex_scan_kernel<LPR, U>), dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, a, g, order, static_cast<u64>(lo), n);
    return hipGetLastError();
}

} // namespace

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------

hipError_t launch_popindex_popc(const void* rows, uint64_t nrows, uint32_t W, uint16_t* popc, uint32_t* hist, int num_cus, hipStream_t s)
{
    if (nrows == 0) return hipSuccess;
    if (W == 0 || !rows || !popc || !hist) return hipErrorInvalidValue;
    const uint32_t nbins = W * 32u + 1u;
    const uint32_t lpr = (W % 4 == 0 && (W / 4 & (W / 4 - 1)) == 0 && W / 4 <= 64) ? W / 4 : 0;
    // sixteen waves per CU (no double buffer in registers: the waves side by side hide the loads), never more waves than work
    const uint64_t rows_per_wave = lpr ? static_cast<uint64_t>(kPopcUnroll) * (64 / lpr) : (W < 32 ? 64 : 1);
    const uint64_t want = ((nrows + rows_per_wave - 1) / rows_per_wave + 3) / 4;
    const uint32_t blocks = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(want, static_cast<uint64_t>(num_cus > 0 ? num_cus : 1) * 4u)));
    switch (lpr) {
    case 1: return launch_popc_t<1>(rows, nrows, popc, hist, nbins, blocks, s);
    case 2: return launch_popc_t<2>(rows, nrows, popc, hist, nbins, blocks, s);
    case 4: return launch_popc_t<4>(rows, nrows, popc, hist, nbins, blocks, s);
    case 8: return launch_popc_t<8>(rows, nrows, popc, hist, nbins, blocks, s);
    case 16: return launch_popc_t<16>(rows, nrows, popc, hist, nbins, blocks, s);
    case 32: return launch_popc_t<32>(rows, nrows, popc, hist, nbins, blocks, s);
    case 64: return launch_popc_t<64>(rows, nrows, popc, hist, nbins, blocks, s);
    default: break;
    }
    hipLaunchKernelGGL(popindex_popc_generic_kernel, dim3(blocks), dim3(kPopcBlock), 0, s, static_cast<const uint32_t*>(rows), static_cast<u64>(nrows), W,
                       popc, hist, nbins);
    return hipGetLastError();
}

hipError_t popindex_sort_bytes(uint64_t n, uint32_t end_bit, size_t* bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<const uint16_t*>(nullptr), static_cast<uint16_t*>(nullptr),
                                     rocprim::counting_iterator<uint32_t>(0u), static_cast<uint32_t*>(nullptr), static_cast<size_t>(n), 0u, end_bit);
}

hipError_t launch_popindex_sort(void* tmp, size_t tmp_bytes, const uint16_t* popc, uint16_t* popc_sorted, uint32_t* order, uint64_t n,
                                uint32_t end_bit, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    size_t bytes = tmp_bytes;
    return rocprim::radix_sort_pairs(tmp, bytes, popc, popc_sorted, rocprim::counting_iterator<uint32_t>(0u), order, static_cast<size_t>(n), 0u, end_bit,
                                     s);
}

hipError_t popindex_scan_bytes(uint64_t n, size_t* bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u,
                                   static_cast<size_t>(n), rocprim::plus<uint32_t>());
}

hipError_t launch_popindex_first(void* tmp, size_t tmp_bytes, const uint32_t* hist, uint32_t* first, uint64_t n, hipStream_t s)
{
    size_t bytes = tmp_bytes;
    return rocprim::exclusive_scan(tmp, bytes, hist, first, 0u, static_cast<size_t>(n), rocprim::plus<uint32_t>(), s);
}

hipError_t launch_popindex_bounds(uint32_t fp_bits, uint32_t qpop, int metric, float alpha, float beta, float* ub, hipStream_t s)
{
    if (!ub || qpop > fp_bits) return hipErrorInvalidValue;
    hipLaunchKernelGGL(popindex_bounds_kernel, dim3((fp_bits + 1u + 255u) / 256u), dim3(256), 0, s, fp_bits, qpop, metric, alpha, beta, ub);
    return hipGetLastError();
}

ScanGeometry popindex_scan_geometry(uint64_t n, uint32_t W, int num_cus)
{
    // the scan's own grid over a "table" of n rows: one wave per SIMD, eight loads in flight per lane and eight more prefetched
    ScanGeometry g = scan_geometry(n, W, num_cus, 4, 8);
    if (g.lanes_per_row != 0) return g;
    // a width without a power-of-two lane count: one slot per lane, 64 slots a chunk -- the grid the gather's lane kernel takes for a
    // list of n entries (the two lane kernels walk their chunks alike)
    return subset_gather_geometry(n, W, num_cus);
}

hipError_t launch_popindex_scan(const ScanArgs& a, const ScanGeometry& g, const uint32_t* order, uint64_t lo, uint32_t n, hipStream_t s)
{
    if (n == 0 || !order || !a.rows) return hipErrorInvalidValue;
#define GSIM_CASE(L) \
    if (g.lanes_per_row == L && g.unroll == 8) return launch_window_t<L, 8>(a, g, order, lo, n, s);
    GSIM_CASE(1)
    GSIM_CASE(2)
    GSIM_CASE(4)
    GSIM_CASE(8)
    GSIM_CASE(16)
    GSIM_CASE(32)
    GSIM_CASE(64)
#undef GSIM_CASE
    if (g.lanes_per_row != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(popindex_scan_lane_kernel, dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, a, g, order, static_cast<u64>(lo), n);
    return hipGetLastError();
}

} // namespace gsim
