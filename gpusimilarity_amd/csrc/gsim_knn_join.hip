// gsim_knn_join.hip -- exact k-nearest-neighbour joins (gsim_db_knn_join / gsim_db_knn_queries): for every LEFT row its k nearest
// rows of the table.  The fold kernel of gsim_knn.hip with two changes, and the merge that the second one needs.
//
// Fold kernel: knn_fold_kernel's scheme, hot loop unchanged -- the owner row whole in VGPRs, the candidate's words wave-uniform
// through the scalar path as the SGPR operand of v_and_b32, popc(candidate) 64 at a time handed out with v_readlane, the per-lane
// band of gsim_prefilter.h, the divide only when some lane's pair passes, the wave-served insertion with the strict s > tau.
//   * the owners are not the table's rows: nl x WP words of their own (the left table's rows, or uploaded queries, zero-padded
//     by nbr_prepare_kernel where W != WP); the candidates and their popcounts are the table's;
//   * no pair is excluded unless the call says that owner o IS table row self0 + o (GSIM_KNN_EXCLUDE_SELF): a lane's own row
//     number is then what knn_fold_kernel's `j != i` compares with, and 2^32 - 1 -- no row of a table of fewer than 2^32 rows --
//     otherwise: the test costs the same either way;
//   * a workgroup is (owner tile, segment s): blockIdx.y cuts the table's column tiles into nseg contiguous ascending segments
//     (knn_join_seg_begin) and the workgroup folds the rows [r0, r1) of ITS segment into the partial list (owner, s).  A few
//     hundred owners against a long table thus fill the device, which gsim_db_knn's fold cannot.  Partial lists are lists like any
//     other: they carry from launch to launch, the pieces of a segment follow each other in ascending order on one stream.
// With nseg == 1 the partial lists are the final lists.
//
// Merge kernel: one thread per entry of a partial list.  Every partial list is in (score descending, row ascending) order and
// every row of segment s is below every row of segment s + 1, so in the order of the union an entry x of segment s comes behind
// exactly: the entries ahead of it in its own list, the entries of earlier segments that score >= x (an equal score there has a
// lower row), and the entries of later segments that score > x.  The last two are the lengths of prefixes of sorted lists:
// binary searches.  The sum is the entry's rank in the union; ranks are unique, and an entry is written to slot `rank` of the
// final list when rank < k.  An entry of the final first k is never lost to a partial list's own cut: an entry that a partial
// list dropped had k entries of its own segment ahead of it.  No atomics on the lists (the one there is adds to a statistic),
// no per-thread arrays, one writer per slot.  A thread stops adding as soon as its rank reaches k, so entries far down the
// union cost a segment or two.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_held_row.h"
#include "gsim_prefilter.h"

namespace gsim
{
namespace
{

template <int WP> __global__ __launch_bounds__(kKnnBlock) void knn_join_fold_kernel(KnnJoinArgs a, uint32_t ot0, u64 r0, u64 r1)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    // the wave's 64 owners: left rows o0 .. o0 + 63 of the call
    const u64 o0 = (static_cast<u64>(ot0) + blockIdx.x) * kKnnTile + wib * 64u;
    if (o0 >= a.nl) return; // (wave-uniform; the kernel has no barrier)
    // this workgroup's candidates: the rows [r0, r1) of segment blockIdx.y
    const u64 seg = blockIdx.y;
    const u64 seg0 = knn_join_seg_begin(seg, a.nseg, a.nrows), seg1 = knn_join_seg_begin(seg + 1, a.nseg, a.nrows);
    const u64 c0 = seg0 + r0;
    const u64 c1 = seg1 - seg0 < r1 ? seg1 : seg0 + r1;
    if (c0 >= c1) return; // (a shorter segment that is done)
    const bool stamp = a.clk && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0; // (segment 0 is never done before another)
    if (stamp) stamp_begin(a.clk);
    const u64 o = o0 + lane;
    const bool oin = o < a.nl; // a lane past the last owner is idle, but takes part in the ballots
    // the table row that IS this owner, where the call says so; else no row's number
    const uint32_t i = oin && a.self0 != ~0ull ? static_cast<uint32_t>(a.self0 + o) : 0xFFFFFFFFu;

    // this lane's owner row, whole, in VGPRs (zero words beyond the row: nothing to count there)
    u32x4 r4[WP / 4];
    const u32x4* rp = reinterpret_cast<const u32x4*>(a.lrows) + (oin ? o : 0) * (WP / 4);
#pragma unroll
    for (int w = 0; w < WP / 4; w++) r4[w] = oin ? rp[w] : u32x4{0, 0, 0, 0};
    uint32_t av = 0;
#pragma unroll
    for (int w = 0; w < WP / 4; w++) av += __popc(r4[w].x) + __popc(r4[w].y) + __popc(r4[w].z) + __popc(r4[w].w);

    const uint32_t k = a.k;
    const u64 l0 = o0 * a.nseg + seg;                 // list number of the wave's first owner; the next owner's is nseg further
    const u64 lo = l0 + static_cast<u64>(lane) * a.nseg; // this lane's
    uint32_t len = oin ? a.len[lo] : 0u;
    float tau = len == k ? a.lists[lo * k + (k - 1)].score : a.cutoff;
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
            KnnEntry* list = a.lists + (l0 + static_cast<u64>(L) * a.nseg) * k;
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
    if (oin) a.len[lo] = len;
    if (inserts && lane == 0) atomicAdd(a.inserts, static_cast<u64>(inserts));
    if (stamp) stamp_end(a.clk);
}

// entries of list[0 .. n) (scores descending) that score >= x (or_equal) or > x
__device__ __forceinline__ uint32_t knn_join_ahead(const KnnEntry* __restrict__ list, uint32_t n, float x, bool or_equal)
{
    uint32_t lo = 0, hi = n; // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const float s = list[mid].score;
        if (or_equal ? s >= x : s > x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// thread (owner blockIdx.x, entry t = blockIdx.y * 256 + threadIdx.x of its nseg x k partial slots)
__global__ __launch_bounds__(256) void knn_join_merge_kernel(const KnnEntry* __restrict__ lists, const uint32_t* __restrict__ len, uint32_t nseg,
                                                             uint32_t k, KnnEntry* __restrict__ out, uint32_t* __restrict__ out_len,
                                                             unsigned long long* __restrict__ held)
{
    const u64 o = blockIdx.x;
    const uint32_t* olen = len + o * nseg;
    const KnnEntry* olists = lists + o * nseg * k;
    const uint32_t t = blockIdx.y * 256u + threadIdx.x;
    if (t == 0) { // the final length: everything held, up to k (and the call's count of entries held before the merge)
        u64 total = 0;
        for (uint32_t s = 0; s < nseg; s++) total += olen[s];
        out_len[o] = total < k ? static_cast<uint32_t>(total) : k;
        if (total) atomicAdd(held, total);
    }
    const uint32_t seg = t / k, e = t % k;
    if (seg >= nseg || e >= olen[seg]) return;
    const KnnEntry x = olists[static_cast<u64>(seg) * k + e];
    uint32_t rank = e;
    for (uint32_t s = 0; s < nseg && rank < k; s++)
        if (s != seg) rank += knn_join_ahead(olists + static_cast<u64>(s) * k, olen[s], x.score, s < seg);
    if (rank < k) out[o * k + rank] = x;
}

} // namespace

hipError_t launch_knn_join_fold(const KnnJoinArgs& a, uint32_t ot0, uint32_t not_, uint64_t r0, uint64_t r1, hipStream_t s)
{
    if (not_ == 0 || r0 >= r1) return hipSuccess;
    const u64 nct = (a.nrows + kKnnColTile - 1) / kKnnColTile;
    if (a.k < 1 || a.k > GSIM_KNN_MAX_K || a.nseg < 1 || a.nseg > kKnnJoinMaxSegments || a.nseg > nct || a.nrows > 0xFFFFFFFFull ||
        (static_cast<u64>(ot0) + not_ - 1) * kKnnTile >= a.nl || (a.self0 != ~0ull && a.self0 + a.nl > a.nrows))
        return hipErrorInvalidValue;
    const dim3 grid(not_, a.nseg), block(kKnnBlock);
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL(knn_join_fold_kernel<decltype(wp)::value>, grid, block, 0, s, a, ot0, static_cast<u64>(r0), static_cast<u64>(r1));
        return hipGetLastError();
    });
}

hipError_t launch_knn_join_merge(const KnnEntry* lists, const uint32_t* len, uint64_t nl, uint32_t nseg, uint32_t k, KnnEntry* out,
                                 uint32_t* out_len, unsigned long long* held, hipStream_t s)
{
    if (nl == 0) return hipSuccess;
    if (k < 1 || k > GSIM_KNN_MAX_K || nseg < 1 || nseg > kKnnJoinMaxSegments || nl > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid(static_cast<uint32_t>(nl), (nseg * k + 255u) / 256u), block(256);
    hipLaunchKernelGGL(knn_join_merge_kernel, grid, block, 0, s, lists, len, nseg, k, out, out_len, held);
    return hipGetLastError();
}

} // namespace gsim
