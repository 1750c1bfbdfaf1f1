// gsim_row_units.h -- what the kernels beside the table scan share.  Internal; gsim_scan.hip, gsim_fused.hip
// and the batch kernels do not include it: scan_rows and reduce_chunk (gsim_scan_inl.h) stay their own.
//
//   listed rows   a chunk of rows that carry their row numbers in registers -- gathered through a list (gsim_subset.hip) or the
//                 slots of a window of a reordered copy (gsim_popindex.hip) -- reduced and offered to the streaming filter
//                 (reduce_listed); the threshold poll of a wave's trips (poll_threshold: these two and group_scan_kernel); the
//                 kernel of the widths without a power-of-two number of 16-byte units, one entry per lane (listed_lane_kernel).
//   per-row walk  one streaming pass that does something with every row once -- a popcount (popindex_popc_kernel), a hash and a
//                 probe (rowhash_x4_kernel) -- as HeldRow is shaped: the walk is here, what happens to a row is the visitor's
//                 (walk_rows_x4, walk_rows_strided).
//   dispatch_lpr  the host-side dispatch over the seven power-of-two lane counts (pow2_lanes_per_row, gsim_device.h), as
//                 dispatch_wp (gsim_held_row.h) is for the padded widths.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "gsim_device_common.h"
#include "gsim_filter_inl.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

// f(std::integral_constant<int, LPR>) for rows of lpr = 1, 2, ... 64 sixteen-byte units
template <class F> hipError_t dispatch_lpr(uint32_t lpr, F&& f)
{
    switch (lpr) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------
// listed rows
// ---------------------------------------------------------------------------

// The threshold poll of scan_rows (gsim_scan_inl.h): one wave of the workgroup (`wib`: the wave's index in it) per period reads gtau
template <typename Filter> __device__ __forceinline__ void poll_threshold(Filter& f, uint32_t& gt, uint32_t& trip, uint32_t wib, int lane)
{
    f.refresh(gt, lane);
    const uint32_t period = trip < 64u ? 8u : (trip < 512u ? 32u : 128u);
    if ((trip & (period - 1u)) == 0 && ((trip / period) & (kScanBlock / 64 - 1)) == wib) gt = f.load_gtau();
    trip++;
}

// reduce_chunk for listed rows: load j of lane (grp, sub) holds unit `sub` of entry e0 + j * RPL + grp of a list of n, which is row
// ix[j] (v_and + v_bcnt + group_sum, then LPR rows a round to the filter).  FULL: every entry of the chunk exists.
template <int LPR, int U, bool FULL, typename Filter>
__device__ __forceinline__ void reduce_listed(const u32x4 (&d)[U], const uint32_t (&ix)[U], const u32x4& q, u64 e0, uint32_t n, const ScanArgs& a,
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
        // lane (grp, sub) takes the entry of load j = r * LPR + sub
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

// Every width without a power-of-two number of 16-byte units: one entry of a list of n per lane, word by word (scan_rows_lane's
// arithmetic), 64 entries per trip, offered as row list[e].  The entry's words: row list[e] of a.rows, or (SLOTS: a.rows is a
// copy in the list's order) row e.
template <bool SLOTS>
__global__ __launch_bounds__(kScanBlock) void listed_lane_kernel(ScanArgs a, ScanGeometry g, const uint32_t* list, uint32_t n)
{
    __shared__ BlockFilter s_filter;
    if (a.gate && *a.gate == 0) return;
    const int lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (threadIdx.x >> 6));
    block_filter_init(&s_filter, a.k, a.state->gtau);
    WaveFilter f;
    f.init(&s_filter, a.state, a.cand + static_cast<u64>(w) * g.seg_cap, a.cand_cb + static_cast<u64>(w) * g.seg_cap, a.k, a.cutoff);
    const uint32_t* db = static_cast<const uint32_t*>(a.rows);
    for (u64 c = w; c < g.nchunks; c += g.nwaves) {
        const u64 e = c * 64u + static_cast<uint32_t>(lane);
        const bool active = e < n;
        const uint32_t row = active ? list[e] : 0u;
        uint32_t cc = 0, bb = 0;
        if (active) {
            const uint32_t* r = db + (SLOTS ? e : static_cast<u64>(row)) * a.W;
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

// ---------------------------------------------------------------------------
// per-row walk
// ---------------------------------------------------------------------------

// Rows [r0, r1) of LPR sixteen-byte units, LPR a power of two up to 64: chunks of U x 64 / LPR rows, wave w of nwaves takes chunks w,
// w + nwaves, ...; all U loads of a chunk are issued (16 B per lane, non-temporal), then visit(row, in_range, unit) is called for
// each, by all 64 lanes: the LPR lanes of a group hold the row's units (lane % LPR), zero where the row is past r1.
template <int LPR, int U, typename Visit>
__device__ __forceinline__ void walk_rows_x4(const u32x4* __restrict__ src, u64 r0, u64 r1, u64 w, u64 nwaves, int lane, Visit&& visit)
{
    constexpr int RPL = 64 / LPR;
    constexpr int CH = U * RPL;
    const int sub = lane % LPR, grp = lane / LPR;
    const u64 nchunks = (r1 - r0 + CH - 1) / CH;
    for (u64 c = w; c < nchunks; c += nwaves) {
        const u64 first = r0 + c * CH + static_cast<u64>(grp); // the row of the lane's first load
        u32x4 d[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const u64 row = first + static_cast<u64>(j * RPL);
            d[j] = row < r1 ? stream_load(src + row * LPR + sub) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            const u64 row = first + static_cast<u64>(j * RPL);
            visit(row, row < r1, d[j]);
        }
    }
}

// Every other width, rows of W words, G lanes per row: G = 1 (rows of fewer than 32 words: 64 rows per wave trip) or G = 64 (one
// row per wave trip).  visit(row, in_range, words) is called by all 64 lanes; lane l of a group reads words[l % G], words[l % G + G], ...
// itself -- word loads: no width needs padding.
template <int G, typename Visit>
__device__ __forceinline__ void walk_rows_strided(const uint32_t* __restrict__ src, u64 r0, u64 r1, uint32_t W, u64 w, u64 nwaves, int lane,
                                                  Visit&& visit)
{
    constexpr int RPW = 64 / G;
    for (u64 b = r0 + w * RPW; b < r1; b += nwaves * RPW) {
        const u64 row = b + static_cast<u64>(lane / G);
        visit(row, row < r1, src + row * W);
    }
}

} // namespace
} // namespace gsim
