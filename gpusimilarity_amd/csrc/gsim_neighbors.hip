// gsim_neighbors.hip -- all-pairs neighbour lists above a cutoff (the similarity self-join behind gsim_db_neighbors)
// and the device half of their CSR.
//
// Tile kernel: the held-row pair count of gsim_held_row.h (the scalar-operand VALU scheme of batch_scan_kernel, gsim_batch.hip,
// with the table on both sides).
//   * a workgroup owns a tile of kNbrTile left rows x kNbrTile right rows; each of its four waves holds 64 right rows,
//     one whole (zero-padded) fingerprint per lane in VGPRs (HeldRow), and walks the tile's left rows one by one;
//   * the left row's words are wave-uniform: a (left, right) word-pair costs v_and + the accumulating v_bcnt_u32_b32;
//   * popc(left row) comes from a side array made once per call (nbr_prepare_kernel) through Handout64, popc(right row)
//     from the lane's own registers;
//   * the keep decision is exactly score_of(...) >= cutoff: the division-free band of gsim_prefilter.h
//     (valu_surely_not_kept, proven on the host by tests/cpp/prefilter_check.cpp) drops almost every pair with one
//     multiply and a compare, and every pair it lets through is scored with the reference's divide;
//   * survivors are appended as sort keys ((left row - row_begin) << 32 | right row, score) through one wave-aggregated
//     atomic cursor; the cursor keeps counting past the buffer's capacity, the host grows the buffer to the exact size
//     and runs the launches that overflowed once more (capi_neighbors.cpp).
// A full-table call runs the upper triangle only (diagonal tiles keep j > i) and appends every pair under both rows.
//
// CSR: one radix sort of the keys (rocPRIM, on the handle's stream) puts every row's list in column order, whatever
// order the tiles found the pairs in; a last kernel writes the row offsets and the column indices.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_held_row.h"
#include "gsim_prefilter.h"

namespace gsim
{
namespace
{

// popc of every row, and (pad != nullptr) the rows copied to WP words with zero words after the first W
__global__ __launch_bounds__(256) void nbr_prepare_kernel(const uint32_t* __restrict__ rows, u64 nrows, uint32_t W, uint32_t WP,
                                                          uint32_t* __restrict__ pad, uint32_t* __restrict__ pop)
{
    const u64 r = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t* src = rows + r * W;
    uint32_t p = 0;
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t x = src[w];
        p += static_cast<uint32_t>(__popc(x));
        if (pad) pad[r * WP + w] = x;
    }
    if (pad)
        for (uint32_t w = W; w < WP; w++) pad[r * WP + w] = 0u;
    pop[r] = p;
}

// JOIN (gsim_db_join*, launch_join_tiles): the left rows are a.lrows / a.lpop instead of the table's own, there is no triangle,
// and no pair is excluded -- separate instantiations, so that the self-join's stay what they are.
template <bool JOIN, class Args> __device__ __forceinline__ auto tile_tri(const Args& a)
{
    if constexpr (JOIN) return 0;
    else return a.tri;
}
template <bool JOIN, class Args> __device__ __forceinline__ const uint32_t* tile_left_rows(const Args& a)
{
    if constexpr (JOIN) return a.lrows;
    else return a.rows;
}
template <bool JOIN, class Args> __device__ __forceinline__ const uint32_t* tile_left_pop(const Args& a)
{
    if constexpr (JOIN) return a.lpop;
    else return a.pop;
}

template <int WP, bool JOIN = false, class Args = NbrArgs>
__global__ __launch_bounds__(kNbrBlock) void nbr_tile_kernel(Args a, uint32_t rt0, uint32_t ct0)
{
    const uint32_t rt = rt0 + blockIdx.y;
    const uint32_t ct = ct0 + blockIdx.x;
    if (tile_tri<JOIN>(a) && ct < rt) return; // below the diagonal: that pair was found from the other side
    const int lane = threadIdx.x & 63;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    const u64 i0 = a.row_begin + static_cast<u64>(rt) * kNbrTile;
    if (i0 >= a.row_end) return;
    const u64 iend = i0 + kNbrTile < a.row_end ? i0 + kNbrTile : a.row_end;
    // the clock this launch ran at: shader cycles (s_memtime) against the 100 MHz wall clock over one full tile
    const bool stamp = a.clk && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 j = static_cast<u64>(ct) * kNbrTile + wib * 64u + static_cast<uint32_t>(lane);
    const bool jin = j < a.nrows;

    HeldRow<WP> right; // this lane's right row
    const uint32_t b = right.load(a.rows, jin ? j : 0, jin);

    uint32_t nl = static_cast<uint32_t>(iend - i0);
    // diagonal tile (i0 == first right row of the tile): left row i0 + t pairs with some right row of this wave only if
    // t < 64 wib + 63
    if (tile_tri<JOIN>(a) && ct == rt && nl > wib * 64u + 63u) nl = wib * 64u + 63u;

    const float cut_lo = valu_cutoff_lo(a.cutoff);
    const uint32_t per = tile_tri<JOIN>(a) ? 2u : 1u;
    const const_u32x4p lrows = (const_u32x4p) (tile_left_rows<JOIN>(a)) + i0 * (WP / 4);
    // left row t against this lane's right row: keep == (score_of(...) >= cutoff), s = that score
    auto pair = [&](uint32_t t, uint32_t av, float& s) __attribute__((always_inline)) -> bool {
        const const_u32x4p qw = lrows + static_cast<u64>(t) * (WP / 4);
        const uint32_t c = right.common(qw);
        const u64 i = i0 + t;
        const bool valid = JOIN ? jin : jin && (tile_tri<JOIN>(a) ? j > i : j != i);
        const float den = score_den(a.metric, a.alpha, a.beta, av, b, c);
        const float cf = static_cast<float>(c);
        const bool maybe = valid && !valu_surely_not_kept(cut_lo, cf, den, c);
        s = 0.0f;
        if (__ballot(maybe) == 0) return false;
        s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, av, b, c)
        return maybe && s >= a.cutoff;
    };
    // Pass 1 counts: the kept pairs of the wave's tile, and which left rows have any (a bit per row in LDS).  Pass 2 only
    // when there are some: ONE cursor atomic for the whole wave-tile, then those rows again, their pairs stored.  A tile
    // whose every pair is kept costs twice the arithmetic but 1 atomic instead of 256.
    __shared__ uint32_t s_rows[kNbrBlock / 64][kNbrTile / 32];
    if (lane < kNbrTile / 32) s_rows[wib][lane] = 0u;
    Handout64 vpop; // popc of the left rows
    uint32_t cnt = 0;
    for (uint32_t t = 0; t < nl; t++) {
        if (Handout64::due(t)) vpop.fetch(tile_left_pop<JOIN>(a), i0 + t, static_cast<uint32_t>(lane), iend);
        const uint32_t av = vpop.get(t);
        float s;
        const u64 m = __ballot(pair(t, av, s));
        if (m == 0) continue;
        cnt += static_cast<uint32_t>(__popcll(m));
        if (lane == 0) s_rows[wib][t >> 5] |= 1u << (t & 31u);
    }
    if (cnt) {
        u64 base = 0;
        if (lane == 0) base = atomicAdd(a.cursor, static_cast<u64>(cnt) * per);
        base = (static_cast<u64>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base >> 32)))) << 32) |
               static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base & 0xFFFFFFFFull)));
        for (uint32_t w = 0; w < kNbrTile / 32; w++) {
            uint32_t rows = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(s_rows[wib][w])));
            while (rows) {
                const uint32_t t = w * 32u + static_cast<uint32_t>(__builtin_ctz(rows));
                rows &= rows - 1u;
                const u64 i = i0 + t;
                const uint32_t av = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(tile_left_pop<JOIN>(a)[i])));
                float s;
                const bool keep = pair(t, av, s);
                const u64 m = __ballot(keep);
                if (keep) {
                    const u64 pos = base + static_cast<u64>(lane_rank(m)) * per;
                    if (pos < a.cap) {
                        a.keys[pos] = ((i - a.row_begin) << 32) | j;
                        a.vals[pos] = s;
                    }
                    if (tile_tri<JOIN>(a) && pos + 1 < a.cap) { // the same pair under the right row (full-table calls: row_begin == 0)
                        a.keys[pos + 1] = (j << 32) | i;
                        a.vals[pos + 1] = s;
                    }
                }
                base += static_cast<u64>(__popcll(m)) * per;
            }
        }
    }
    if (stamp) stamp_end(a.clk);
}

__global__ void nbr_snap_kernel(const u64* cursor, u64* snap)
{
    *snap = *cursor;
}

// sorted keys -> indptr[0 .. nrows_out] and the indices (+ row_base), every output by its own thread: thread r writes
// indptr[r] = the first position whose row is >= r (a lower_bound over the sorted keys, <= 64 steps), thread p < n the
// index of position p -- no thread loops over a run of empty rows
__global__ __launch_bounds__(256) void nbr_csr_kernel(const u64* __restrict__ keys, u64 n, u64 nrows_out, uint32_t row_base,
                                                      u64* __restrict__ indptr, uint32_t* __restrict__ indices)
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
    if (t < n) indices[t] = static_cast<uint32_t>(keys[t]) + row_base;
}

} // namespace

uint32_t nbr_padded_words(uint32_t W)
{
    for (uint32_t wp = 4; wp <= kNbrMaxWords; wp *= 2)
        if (W <= wp) return wp;
    return 0;
}

hipError_t launch_nbr_prepare(const void* rows, uint64_t nrows, uint32_t W, uint32_t WP, uint32_t* pad, uint32_t* pop,
                              hipStream_t s)
{
    if (nrows == 0) return hipSuccess;
    hipLaunchKernelGGL(nbr_prepare_kernel, dim3(static_cast<uint32_t>((nrows + 255) / 256)), dim3(256), 0, s,
                       static_cast<const uint32_t*>(rows), static_cast<u64>(nrows), W, WP, pad, pop);
    return hipGetLastError();
}

hipError_t launch_nbr_tiles(const NbrArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s)
{
    const dim3 grid(nct, nrt), block(kNbrBlock);
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL(nbr_tile_kernel<decltype(wp)::value>, grid, block, 0, s, a, rt0, ct0);
        return hipGetLastError();
    });
}

hipError_t launch_join_tiles(const JoinTileArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s)
{
    const dim3 grid(nct, nrt), block(kNbrBlock);
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL((nbr_tile_kernel<decltype(wp)::value, true, JoinTileArgs>), grid, block, 0, s, a, rt0, ct0);
        return hipGetLastError();
    });
}

hipError_t launch_nbr_snap(const unsigned long long* cursor, unsigned long long* snap, hipStream_t s)
{
    hipLaunchKernelGGL(nbr_snap_kernel, dim3(1), dim3(1), 0, s, cursor, snap);
    return hipGetLastError();
}

hipError_t nbr_sort_bytes(uint64_t n, uint32_t end_bit, size_t* bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<const u64*>(nullptr), static_cast<u64*>(nullptr),
                                     static_cast<const float*>(nullptr), static_cast<float*>(nullptr), static_cast<size_t>(n), 0u,
                                     end_bit);
}

hipError_t launch_nbr_csr(void* tmp, size_t tmp_bytes, const unsigned long long* keys, const float* vals, unsigned long long* keys_sorted,
                          float* vals_sorted, uint64_t n, uint32_t end_bit, uint64_t nrows_out, uint32_t row_base, uint64_t* indptr,
                          uint32_t* indices, hipStream_t s)
{
    if (n) {
        size_t bytes = tmp_bytes;
        const hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, keys, keys_sorted, vals, vals_sorted, static_cast<size_t>(n), 0u,
                                                       end_bit, s);
        if (e != hipSuccess) return e;
    }
    const u64 threads = n > nrows_out + 1 ? n : nrows_out + 1;
    hipLaunchKernelGGL(nbr_csr_kernel, dim3(static_cast<uint32_t>((threads + 255) / 256)), dim3(256), 0, s,
                       static_cast<const u64*>(keys_sorted), static_cast<u64>(n), static_cast<u64>(nrows_out), row_base,
                       reinterpret_cast<u64*>(indptr), indices);
    return hipGetLastError();
}

} // namespace gsim
