// gsim_popindex.hip -- popcount indexes (gsim_popindex_*, gsim_db_search_bounded): the table's rows ordered by popcount, and the
// scan of a window of that order.
//
// A query with a bits set and a row with b bits set share c bits, max(0, a + b - fp_bits) <= c <= min(a, b), so the row's score is at
// most ub[b] = the largest score_of(a, b, c) over that range -- found by enumeration with the scan's own arithmetic, hence exact for
// every metric, f32 roundings included (popindex_bounds_kernel).  With the rows sorted by (popcount, row) the rows that can reach a
// score are a contiguous window of the order; the host (capi_popindex.cpp) picks the windows, this file builds the order and scans.
//   popindex_popc_kernel     one streaming pass over the table (walk_rows_x4 / walk_rows_strided, gsim_row_units.h): a 16-bit
//                            popcount per row and the histogram of the popcounts, kept in LDS and flushed once per workgroup
//   rocPRIM                  a stable radix sort of (popcount, row) over the popcount's significant bits: `order`; `first` is the
//                            exclusive scan of the histogram (launch_scan_u32)
//   popindex_bounds_kernel   ub[0 .. fp_bits] of one query popcount, thread b enumerating c
//   popindex_scan_kernel     slots [lo, lo + n) of the popcount-ordered COPY of the rows, streamed as scan_kernel streams the table
//                            (group-of-lanes loads, the next chunk's loads in flight while the current one is reduced:
//                            reduce_listed, gsim_row_units.h); slot i is offered to WaveFilter as row order[i], 4 bytes a row read a
//                            chunk ahead.  Widths without a power-of-two number of 16-byte units: one slot per lane
//                            (listed_lane_kernel<true>, gsim_row_units.h).  What it leaves is what scan_kernel leaves: the
//                            four-kernel pipeline's tail runs behind it unchanged.
// Without the copy a window is gathered through `order` by gsim_subset.hip's launch_subset_gather; the copy itself is made by
// gsim_label_sums.hip's launch_lsum_gather.
// Seeding: none, as the row-set scans: gtau starts at 0 and rises through ghist, which counts window rows only.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_filter_inl.h"
#include "gsim_row_units.h"
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

// what the pass keeps of a row: `writer` is the one lane that does it, `bb` the row's popcount
__device__ __forceinline__ void popc_keep(bool writer, u64 row, uint32_t bb, uint16_t* __restrict__ popc, PopcBins& bins)
{
    if (!writer) return;
    popc[row] = static_cast<uint16_t>(bb);
    bins.add(bb);
}

// Rows of LPR sixteen-byte units, LPR a power of two up to 64 (walk_rows_x4: chunks of kPopcUnroll x 64 / LPR rows)
template <int LPR>
__global__ __launch_bounds__(kPopcBlock) void popindex_popc_kernel(const u32x4* __restrict__ rows, u64 nrows, uint16_t* __restrict__ popc,
                                                                   uint32_t* __restrict__ hist, uint32_t nbins)
{
    __shared__ uint32_t s_hist[kPopcLdsBins];
    PopcBins bins = popc_bins_init(s_hist, hist, nbins);
    const int lane = threadIdx.x & 63;
    const u64 w = static_cast<u64>(blockIdx.x) * (kPopcBlock / 64) + (threadIdx.x >> 6);
    const u64 nwaves = static_cast<u64>(gridDim.x) * (kPopcBlock / 64);
    walk_rows_x4<LPR, kPopcUnroll>(rows, 0, nrows, w, nwaves, lane, [&](u64 row, bool in, const u32x4& d) {
        const uint32_t bb = group_sum<LPR>(__popc(d.x) + __popc(d.y) + __popc(d.z) + __popc(d.w));
        popc_keep(lane % LPR == 0 && in, row, bb, popc, bins);
    });
    popc_bins_flush(bins, nbins);
}

// G lanes per row striding over its words (walk_rows_strided), a wide row's words non-temporal
template <int G>
__device__ __forceinline__ void popc_strided(const uint32_t* __restrict__ rows, u64 nrows, uint32_t W, u64 w, u64 nwaves, int lane,
                                             uint16_t* __restrict__ popc, PopcBins& bins)
{
    walk_rows_strided<G>(rows, 0, nrows, W, w, nwaves, lane, [&](u64 row, bool in, const uint32_t* r) {
        uint32_t bb = 0;
        if (in)
            for (uint32_t i = static_cast<uint32_t>(lane % G); i < W; i += G) bb += __popc(G == 1 ? r[i] : __builtin_nontemporal_load(r + i));
        if (G == 64) bb = wave_sum(bb);
        popc_keep(lane % G == 0 && in, row, bb, popc, bins);
    });
}

// Every other width.  Rows of fewer than 32 words: one row per lane, word by word; wider rows: one row per wave.
__global__ __launch_bounds__(kPopcBlock) void popindex_popc_generic_kernel(const uint32_t* __restrict__ rows, u64 nrows, uint32_t W,
                                                                           uint16_t* __restrict__ popc, uint32_t* __restrict__ hist, uint32_t nbins)
{
    __shared__ uint32_t s_hist[kPopcLdsBins];
    PopcBins bins = popc_bins_init(s_hist, hist, nbins);
    const int lane = threadIdx.x & 63;
    const u64 w = static_cast<u64>(blockIdx.x) * (kPopcBlock / 64) + (threadIdx.x >> 6);
    const u64 nwaves = static_cast<u64>(gridDim.x) * (kPopcBlock / 64);
    if (W < 32u) popc_strided<1>(rows, nrows, W, w, nwaves, lane, popc, bins);
    else popc_strided<64>(rows, nrows, W, w, nwaves, lane, popc, bins);
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
            poll_threshold(f, gt, trip, wib, lane);
            reduce_listed<LPR, U, true>(d, ix, q, c * CH, n, a, f, lane);
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
        reduce_listed<LPR, U, false>(d, ix, q, e0, n, a, f, lane);
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
    const uint32_t lpr = pow2_lanes_per_row(W);
    // sixteen waves per CU (no double buffer in registers: the waves side by side hide the loads), never more waves than work
    const uint64_t rows_per_wave = lpr ? static_cast<uint64_t>(kPopcUnroll) * (64 / lpr) : (W < 32 ? 64 : 1);
    const uint64_t want = ((nrows + rows_per_wave - 1) / rows_per_wave + 3) / 4;
    const uint32_t blocks = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(want, static_cast<uint64_t>(num_cus > 0 ? num_cus : 1) * 4u)));
    if (lpr) return dispatch_lpr(lpr, [&](auto l) { return launch_popc_t<decltype(l)::value>(rows, nrows, popc, hist, nbins, blocks, s); });
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
    // a width without a power-of-two lane count: one slot per lane, 64 slots a chunk -- the grid of the gather of a list of n
    // entries (listed_lane_kernel serves both)
    return subset_gather_geometry(n, W, num_cus);
}

hipError_t launch_popindex_scan(const ScanArgs& a, const ScanGeometry& g, const uint32_t* order, uint64_t lo, uint32_t n, hipStream_t s)
{
    if (n == 0 || !order || !a.rows) return hipErrorInvalidValue;
    if (g.lanes_per_row != 0) {
        if (g.unroll != 8) return hipErrorInvalidValue;
        return dispatch_lpr(g.lanes_per_row, [&](auto lpr) { return launch_window_t<decltype(lpr)::value, 8>(a, g, order, lo, n, s); });
    }
    ScanArgs w = a; // the window's first slot: row 0 of the copy and entry 0 of the list, as the lane kernel counts them
    w.rows = static_cast<const uint32_t*>(a.rows) + lo * a.W;
    hipLaunchKernelGGL(listed_lane_kernel<true>, dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, w, g, order + lo, n);
    return hipGetLastError();
}

} // namespace gsim
