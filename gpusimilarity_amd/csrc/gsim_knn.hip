// gsim_knn.hip -- exact k-nearest-neighbour lists of the table's own rows (gsim_db_knn): the fold kernel and the device half
// of its CSR.
//
// Fold kernel: the scalar-operand VALU scheme of nbr_tile_kernel (gsim_neighbors.hip) with the roles reversed.
//   * a workgroup is kKnnTile OWNER rows, the rows whose neighbours are sought: each of its four waves holds 64 of them, one
//     whole (zero-padded) fingerprint per lane in VGPRs, and all four walk the same candidate rows j of [c0, c1) in ascending
//     order;
//   * the candidate's words are wave-uniform: read through the scalar path and used as the SGPR operand of v_and_b32, so an
//     (owner, candidate) word-pair costs v_and + the accumulating v_bcnt_u32_b32; popc(candidate) comes from the side array
//     (nbr_prepare_kernel), 64 at a time, handed out with v_readlane; popc(owner) from the lane's own registers;
//   * every lane keeps its list length, its threshold tau -- the cutoff while its list is not full, the k-th best score held
//     after that -- and the band constant valu_cutoff_lo(tau) in registers.  The division-free band of gsim_prefilter.h
//     (valu_surely_not_kept) drops almost every pair with one multiply and a compare against the LANE's band; only when some
//     lane's pair gets through does the wave take the reference's divide;
//   * a lane accepts when s >= cutoff and its list is not full or s > tau.  STRICTLY greater: candidates arrive in ascending
//     j and a new entry goes behind every held entry with score >= s, so each list is in (score descending, row ascending)
//     order and a boundary tie group keeps its lowest rows -- that is the whole tie rule;
//   * the lists live in global memory, owner x k entries of {score, row} and one length per owner: they are the state that
//     carries from launch to launch.  An insertion is made by the whole wave for one accepting lane at a time: lane l holds
//     entries l and l + 64 of that owner's list, a ballot gives the position, the tail moves up by one entry with one store
//     per lane.  No per-thread array is ever indexed at run time.
// One launch folds the candidates [c0, c1) into the lists of a run of owner tiles; the pieces of the same owners go out as
// successive launches on one stream in ascending column order (capi_knn.cpp).  Stream order is the only dependency: owner
// tiles are independent, nothing waits grid-wide, nothing is merged across workgroups.  A few hundred owners against a very
// long table therefore have little parallelism (their columns are NOT split over workgroups); the launches stay bounded, but
// for such a range gsim_db_search with the rows as queries at k + 1 is faster per owner row (512 owners
// against 1 M x 1024-bit rows take 714 ms here and 31 ms there; with the whole table as owners the fold is the faster one),
// and so is gsim_knn_join.hip's fold, which does split them and returns the same lists (GSIM_KNN_EXCLUDE_SELF; section 23).
//
// CSR: an exclusive scan of the lengths (rocPRIM) gives indptr, one kernel copies the lists' entries to their places.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_held_row.h"
#include "gsim_prefilter.h"

namespace gsim
{
namespace
{

template <int WP> __global__ __launch_bounds__(kKnnBlock) void knn_fold_kernel(KnnArgs a, uint32_t ot0, u64 c0, u64 c1)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    // the wave's 64 owners: list numbers o0 .. o0 + 63 of the call, table rows row_begin + those
    const u64 o0 = (static_cast<u64>(ot0) + blockIdx.x) * kKnnTile + wib * 64u;
    const u64 nown = a.row_end - a.row_begin;
    if (o0 >= nown) return; // (wave-uniform; the kernel has no barrier)
    const bool stamp = a.clk && blockIdx.x == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 o = o0 + lane;
    const bool oin = o < nown; // a lane past the last owner is idle, but takes part in the ballots
    const uint32_t i = static_cast<uint32_t>(a.row_begin + (oin ? o : 0));

    // this lane's owner row, whole, in VGPRs (zero words beyond the row: nothing to count there)
    u32x4 r4[WP / 4];
    const u32x4* rp = reinterpret_cast<const u32x4*>(a.rows) + static_cast<u64>(i) * (WP / 4);
#pragma unroll
    for (int w = 0; w < WP / 4; w++) r4[w] = oin ? rp[w] : u32x4{0, 0, 0, 0};
    uint32_t av = 0;
#pragma unroll
    for (int w = 0; w < WP / 4; w++) av += __popc(r4[w].x) + __popc(r4[w].y) + __popc(r4[w].z) + __popc(r4[w].w);

    const uint32_t k = a.k;
    uint32_t len = oin ? a.len[o] : 0u;
    float tau = len == k ? a.lists[o * k + (k - 1)].score : a.cutoff;
    float cut_lo = valu_cutoff_lo(tau);
    uint32_t inserts = 0; // (wave-uniform)

    const const_u32x4p crows = (const_u32x4p) (a.rows);
    uint32_t vpop = 0;
    for (u64 j = c0; j < c1; j++) {
        const uint32_t t = static_cast<uint32_t>(j - c0);
        if ((t & 63u) == 0) { // popc of the next 64 candidates, one per lane (read back with v_readlane)
            const u64 jl = j + lane;
            vpop = jl < c1 ? a.pop[jl] : 0u;
        }
        const uint32_t b = readlane_u32(vpop, t & 63u);
        const const_u32x4p qw = crows + j * (WP / 4);
        uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
#pragma unroll
        for (int w = 0; w < WP / 4; w++) {
            const u32x4 q = qw[w]; // s_load: the candidate is wave-uniform
            acc0 = bcnt_acc(r4[w].x & q.x, acc0);
            acc1 = bcnt_acc(r4[w].y & q.y, acc1);
            acc2 = bcnt_acc(r4[w].z & q.z, acc2);
            acc3 = bcnt_acc(r4[w].w & q.w, acc3);
        }
        const uint32_t c = (acc0 + acc1) + (acc2 + acc3);
        // the owner is the query: a = popc(owner), b = popc(candidate)
        const float den = score_den(a.metric, a.alpha, a.beta, av, b, c);
        const float cf = static_cast<float>(c);
        const bool maybe = oin && static_cast<uint32_t>(j) != i && !valu_surely_not_kept(cut_lo, cf, den, c);
        if (__ballot(maybe) == 0) continue;
        const float s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, av, b, c)
        u64 accept = __ballot(maybe && s >= a.cutoff && (len < k || s > tau));
        if (accept == 0) continue; // (scores equal to tau end here: the wave paid a divide for nothing)
        inserts += static_cast<uint32_t>(__popcll(accept));
        // One accepting lane L at a time, the whole wave on ITS list: lane l holds entries l and l + 64 (k <= 128).
        while (accept) {
            const uint32_t L = static_cast<uint32_t>(__builtin_ctzll(accept));
            accept &= accept - 1;
            const float sL = __uint_as_float(readlane_u32(__float_as_uint(s), L));
            const uint32_t nL = readlane_u32(len, L);
            KnnEntry* list = a.lists + (o0 + L) * k;
            const uint32_t e0 = lane, e1 = lane + 64u;
            const KnnEntry h0 = e0 < nL ? list[e0] : KnnEntry{0.0f, 0u};
            const KnnEntry h1 = e1 < nL ? list[e1] : KnnEntry{0.0f, 0u};
            // behind every held entry with score >= sL (the held scores descend: those are a prefix); pos <= k - 1, because a
            // full list's last entry scores tau < sL
            const uint32_t pos = static_cast<uint32_t>(__popcll(__ballot(e0 < nL && h0.score >= sL)) + __popcll(__ballot(e1 < nL && h1.score >= sL)));
            if (e0 < nL && e0 >= pos && e0 + 1u < k) list[e0 + 1u] = h0;
            if (e1 < nL && e1 >= pos && e1 + 1u < k) list[e1 + 1u] = h1;
            if (lane == L) list[pos] = KnnEntry{sL, static_cast<uint32_t>(j)};
            const uint32_t nn = nL < k ? nL + 1u : k;
            if (nn == k) { // the list is full now: the k-th best is the new entry, or what was entry k - 2
                float last = sL;
                if (pos + 1u < k) {
                    const uint32_t e = k - 2u;
                    last = __uint_as_float(e < 64u ? readlane_u32(__float_as_uint(h0.score), e) : readlane_u32(__float_as_uint(h1.score), e - 64u));
                }
                if (lane == L) {
                    tau = last;
                    cut_lo = valu_cutoff_lo(last);
                }
            }
            if (lane == L) len = nn;
            // the next insertion into this list -- by this wave, in this launch -- reads these entries from other lanes
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    if (oin) a.len[o] = len;
    if (inserts && lane == 0) atomicAdd(a.inserts, static_cast<u64>(inserts));
    if (stamp) stamp_end(a.clk);
}

// entry (owner, slot) of the lists -> position indptr[owner] + slot of indices (+ row_base) and scores
__global__ __launch_bounds__(256) void knn_compact_kernel(const KnnEntry* __restrict__ lists, const uint32_t* __restrict__ len, const u64* __restrict__ indptr,
                                                          u64 nown, uint32_t k, uint32_t row_base, uint32_t* __restrict__ indices,
                                                          float* __restrict__ scores)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    const u64 o = t / k;
    const uint32_t e = static_cast<uint32_t>(t % k);
    if (o >= nown || e >= len[o]) return;
    const KnnEntry h = lists[t];
    indices[indptr[o] + e] = h.row + row_base;
    scores[indptr[o] + e] = h.score;
}

} // namespace

hipError_t launch_knn_fold(const KnnArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, hipStream_t s)
{
    if (not_ == 0 || c0 >= c1) return hipSuccess;
    if (a.k < 1 || a.k > GSIM_KNN_MAX_K || c1 > a.nrows || a.row_end > a.nrows) return hipErrorInvalidValue;
    const dim3 grid(not_), block(kKnnBlock);
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL(knn_fold_kernel<decltype(wp)::value>, grid, block, 0, s, a, ot0, static_cast<u64>(c0), static_cast<u64>(c1));
        return hipGetLastError();
    });
}

hipError_t knn_scan_bytes(uint64_t n, size_t* bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, static_cast<const uint32_t*>(nullptr), static_cast<u64*>(nullptr), u64{0},
                                   static_cast<size_t>(n), rocprim::plus<u64>());
}

hipError_t launch_knn_offsets(void* tmp, size_t tmp_bytes, const uint32_t* len, uint64_t n, uint64_t* indptr, hipStream_t s)
{
    size_t bytes = tmp_bytes;
    return rocprim::exclusive_scan(tmp, bytes, len, reinterpret_cast<u64*>(indptr), u64{0}, static_cast<size_t>(n), rocprim::plus<u64>(), s);
}

hipError_t launch_knn_compact(const KnnEntry* lists, const uint32_t* len, const uint64_t* indptr, uint64_t nown, uint32_t k, uint32_t row_base,
                              uint32_t* indices, float* scores, hipStream_t s)
{
    const u64 threads = nown * k;
    if (threads == 0) return hipSuccess;
    hipLaunchKernelGGL(knn_compact_kernel, dim3(static_cast<uint32_t>((threads + 255) / 256)), dim3(256), 0, s, lists, len,
                       reinterpret_cast<const u64*>(indptr), static_cast<u64>(nown), k, row_base, indices, scores);
    return hipGetLastError();
}

} // namespace gsim
