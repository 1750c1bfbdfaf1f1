// gsim_mst.hip -- the exact single-linkage dendrogram behind gsim_db_mst: the maximum-similarity spanning forest of the graph
// "score >= cutoff", built by Boruvka rounds.  The rule is stated in include/gpusim_hip.h; the host side is capi_mst.cpp.
//
// ORDER E on the pairs a < b: (score descending, a ascending, b ascending).  It is total, so the forest Kruskal builds in that
// order is unique, and it is the forest Boruvka builds when every component takes its E-first outgoing edge.  A round is
//   1. the fold (mst_fold_kernel): every owner row's E-first edge to a row OUTSIDE its own component;
//   2. O(N) bookkeeping (launch_mst_round): every component's E-first held edge, the edges appended, the components merged.
//
// Fold kernel: knn_fold_kernel's scheme (gsim_knn.hip) with the list replaced by two registers per lane.
//   * a workgroup is kKnnTile owners, 64 to a wave, one whole (zero-padded) fingerprint per lane in VGPRs; the owners come
//     through the round's index list: lane o holds table row own[o];
//   * the candidate rows j of the workgroup's piece of [c0, c1) are walked in ascending order by all four waves: their words
//     come through the scalar path as the SGPR operand of v_and_b32; popc(candidate) AND the candidate's component id come from
//     side arrays, 64 at a time, handed out with v_readlane; the owner's component id sits in a register;
//   * a pair is dead when comp[j] == comp[i] (that covers j == i).  That test comes first: where no lane of the wave has a
//     live pair -- the wave's owners and the candidate all belong to one component, the common case once a giant component
//     has formed -- the candidate's words are not even read.  Then the division-free band of gsim_prefilter.h
//     (valu_surely_not_kept) against the LANE's tau: the cutoff until the lane holds an edge, the held score afterwards.  Only
//     when some lane's pair gets through does the wave take the reference's divide;
//   * what a lane holds is ONE 64-bit word, key(s, j) = (bits of s << 32) | ~j, 0 for nothing.  Scores are non-negative floats,
//     so their bit patterns order as the scores do: a larger key is a larger score or, at the same score, a smaller partner.  A
//     lane accepts when s >= cutoff and key(s, j) > the held key.  Within one walk in ascending j that is exactly "nothing held,
//     or s > tau, STRICTLY": an equal score at a later j has the smaller key;
//   * WHY THE LARGEST KEY IS THE ROW'S E-FIRST FOREIGN EDGE.  Fix the row i.  Its edge to p is the pair (min(i, p), max(i, p)).
//     Among partners of equal score: a partner p < i gives a = p < i, a partner p > i gives a = i, so any p < i comes before any
//     p > i in E; two partners below i are ordered by a = p; two partners above i share a = i and are ordered by b = p.  In
//     every case the smaller p wins: (score descending, partner ascending) for a fixed row is order E, and that is the key;
//   * the state that carries from launch to launch is best[i], 8 bytes per row: a lane starts from the word it finds and
//     publishes with one 64-bit atomicMax if it holds something better at the end.  max over a total order commutes, so
//     the pieces of a row's candidates may run in any order and side by side (blockIdx.y cuts [c0, c1) into pieces: a round
//     with a few hundred owners still fills the device) and the result is the same word.  A stale or half-way value read at the
//     start is a key some piece really found for this row in this round: it can only prune pairs that lose to it anyway.
// No per-thread array is indexed at run time, no scratch, no LDS, no barrier, no grid-wide wait, no spin-wait: stream order is
// the only dependency.
//
// Bookkeeping, one thread per row or per component id, comp[i] = id of i's component (a row of it; flat at round start):
//   * pick: atomicMax(cscore[comp[i]], score bits) over the rows holding an edge, then atomicMin(ckey[comp[i]], a << 32 | b)
//     among the rows holding that score: the component's E-first outgoing edge (min and max commute: deterministic);
//   * hook: component c with an edge to component d sets parent[c] = d.  The only cycles such choices can make under a total
//     order are pairs c <-> d that chose the SAME edge; there the smaller id stays a root, and only it appends the edge.  Every
//     other choice appends its edge.  Appends take a slot with an atomic add: the slots' order is not reproducible, the SET of
//     edges is, and the final sort makes the bytes so;
//   * flatten: parent[x] = root(x) as comp_flatten_kernel does (other threads' stores only put an ancestor in the place of
//     an ancestor), then comp[i] = parent[comp[i]];
//   * the next round's owners: a row's held edge is still its E-first foreign edge if its partner is still foreign, because
//     candidates only ever disappear.  So only the rows whose partner has joined their own component scan again (flag, rocPRIM
//     select of the row numbers, best[] of the selected reset); a row that scanned and holds nothing has no foreign edge >= cutoff
//     and never scans again.
// Final: a stable rocPRIM radix sort by b, then by (~score bits << 32 | a), puts the edges in order E.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_held_row.h"
#include "gsim_prefilter.h"

namespace gsim
{
namespace
{

template <int WP> __global__ __launch_bounds__(kKnnBlock) void mst_fold_kernel(MstArgs a, uint32_t ot0, u64 c0, u64 c1, u64 per)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    const u64 o0 = (static_cast<u64>(ot0) + blockIdx.x) * kKnnTile + wib * 64u;
    if (o0 >= a.nown) return; // (wave-uniform; the kernel has no barrier)
    // this workgroup's piece of the candidates
    const u64 p0 = c0 + static_cast<u64>(blockIdx.y) * per;
    if (p0 >= c1) return;
    const u64 p1 = p0 + per < c1 ? p0 + per : c1;
    const bool stamp = a.clk && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 o = o0 + lane;
    const bool oin = o < a.nown; // a lane past the last owner is idle, but takes part in the ballots
    const uint32_t i = oin ? a.own[o] : 0u;

    // this lane's owner row, whole, in VGPRs (zero words beyond the row: nothing to count there)
    u32x4 r4[WP / 4];
    const u32x4* rp = reinterpret_cast<const u32x4*>(a.rows) + static_cast<u64>(i) * (WP / 4);
#pragma unroll
    for (int w = 0; w < WP / 4; w++) r4[w] = oin ? rp[w] : u32x4{0, 0, 0, 0};
    uint32_t av = 0;
#pragma unroll
    for (int w = 0; w < WP / 4; w++) av += __popc(r4[w].x) + __popc(r4[w].y) + __popc(r4[w].z) + __popc(r4[w].w);

    const uint32_t ci = a.comp[i];
    const u64 found = oin ? __hip_atomic_load(a.best + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    u64 held = found;
    float cut_lo = valu_cutoff_lo(held ? __uint_as_float(static_cast<uint32_t>(held >> 32)) : a.cutoff);

    const const_u32x4p crows = (const_u32x4p) (a.rows);
    uint32_t vpop = 0, vcomp = 0;
    for (u64 j = p0; j < p1; j++) {
        const uint32_t t = static_cast<uint32_t>(j - p0);
        if ((t & 63u) == 0) { // popc and component of the next 64 candidates, one per lane (read back with v_readlane)
            const u64 jl = j + lane;
            vpop = jl < p1 ? a.pop[jl] : 0u;
            vcomp = jl < p1 ? a.comp[jl] : 0u;
        }
        const uint32_t cj = readlane_u32(vcomp, t & 63u);
        const bool live = oin && cj != ci;
        if (__ballot(live) == 0) continue; // the wave's owners and the candidate are one component
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
        const bool maybe = live && !valu_surely_not_kept(cut_lo, cf, den, c);
        if (__ballot(maybe) == 0) continue;
        const float s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, av, b, c)
        const u64 key = (static_cast<u64>(__float_as_uint(s)) << 32) | static_cast<uint32_t>(~static_cast<uint32_t>(j));
        if (maybe && s >= a.cutoff && key > held) { // (NaN is never >= cutoff)
            held = key;
            cut_lo = valu_cutoff_lo(s);
        }
    }
    if (held != found) atomicMax(a.best + i, held);
    if (stamp) stamp_end(a.clk);
}

__global__ __launch_bounds__(256) void mst_init_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x < kMstCtlWords) m.ctl[x] = 0;
    if (x >= m.nrows) return;
    m.comp[x] = m.parent[x] = m.own[x] = static_cast<uint32_t>(x);
    m.best[x] = kMstNone;
}

__global__ __launch_bounds__(256) void mst_reset_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= m.nrows) return;
    m.cscore[x] = 0u;
    m.ckey[x] = ~0ull;
}

__global__ __launch_bounds__(256) void mst_pick_score_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= m.nrows) return;
    const u64 k = m.best[x];
    if (k != kMstNone) atomicMax(m.cscore + m.comp[x], static_cast<uint32_t>(k >> 32));
}

__global__ __launch_bounds__(256) void mst_pick_edge_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= m.nrows) return;
    const u64 k = m.best[x];
    if (k == kMstNone) return;
    const uint32_t c = m.comp[x];
    if (static_cast<uint32_t>(k >> 32) != m.cscore[c]) return;
    const uint32_t i = static_cast<uint32_t>(x), p = ~static_cast<uint32_t>(k);
    const uint32_t lo = i < p ? i : p, hi = i < p ? p : i;
    atomicMin(m.ckey + c, (static_cast<u64>(lo) << 32) | hi);
}

// one thread per component id c that is a root holding an edge: hook, append (head comment)
__global__ __launch_bounds__(256) void mst_hook_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= m.nrows) return;
    const uint32_t c = static_cast<uint32_t>(x);
    const u64 e = m.ckey[c];
    if (m.comp[c] != c || e == ~0ull) return;
    const uint32_t ea = static_cast<uint32_t>(e >> 32), eb = static_cast<uint32_t>(e);
    const uint32_t d = m.comp[ea] == c ? m.comp[eb] : m.comp[ea]; // the component at the other end
    const bool mutual = m.ckey[d] == e;
    if (!(mutual && c < d)) m.parent[c] = d;
    if (!(mutual && c > d)) {
        const u64 slot = atomicAdd(m.ctl + kMstCtlEdges, 1ull);
        if (slot < m.cap) { // (a forest has at most nrows - 1 edges; the host checks the count)
            m.ekey[slot] = (static_cast<u64>(~m.cscore[c]) << 32) | ea;
            m.eb[slot] = eb;
        }
    }
}

__global__ __launch_bounds__(256) void mst_flatten_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= m.nrows) return;
    uint32_t r = static_cast<uint32_t>(x);
    for (;;) {
        const uint32_t p = __hip_atomic_load(m.parent + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == r) break;
        r = p;
    }
    if (r != x) __hip_atomic_store(m.parent + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void mst_relabel_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x < m.nrows) m.comp[x] = m.parent[m.comp[x]];
}

// a row scans again when the partner it holds has joined its own component
__global__ __launch_bounds__(256) void mst_flag_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= m.nrows) return;
    const u64 k = m.best[x];
    const bool again = k != kMstNone && m.comp[~static_cast<uint32_t>(k)] == m.comp[x];
    m.flag[x] = again ? 1u : 0u;
    if (again) m.best[x] = kMstNone;
}

__global__ __launch_bounds__(256) void mst_count_roots_kernel(MstState m)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    const u64 roots = __ballot(x < m.nrows && m.comp[x] == x);
    if (roots && (threadIdx.x & 63u) == 0) atomicAdd(m.ctl + kMstCtlRoots, static_cast<u64>(__popcll(roots)));
}

struct MstEdgeOut {
    uint32_t a, b;
    float score;
};

__global__ __launch_bounds__(256) void mst_emit_kernel(const u64* __restrict__ ekey, const uint32_t* __restrict__ eb, u64 n, uint32_t row_base,
                                                       MstEdgeOut* __restrict__ out)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= n) return;
    const u64 k = ekey[x];
    out[x] = MstEdgeOut{static_cast<uint32_t>(k) + row_base, eb[x] + row_base, __uint_as_float(~static_cast<uint32_t>(k >> 32))};
}

dim3 rows_grid(u64 n) { return dim3(static_cast<uint32_t>((n + 255) / 256)); }

} // namespace

static_assert(sizeof(MstEdgeOut) == sizeof(gsim_mst_edge), "the device writes gsim_mst_edge");

hipError_t launch_mst_fold(const MstArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t nchunk, hipStream_t s)
{
    if (not_ == 0 || c0 >= c1) return hipSuccess;
    if (c1 > a.nrows || a.nown > a.nrows || nchunk < 1 || nchunk > 65535u) return hipErrorInvalidValue;
    const u64 per = ((c1 - c0 + nchunk - 1) / nchunk + 63u) / 64u * 64u;
    const dim3 grid(not_, nchunk), block(kKnnBlock);
    const u64 b0 = c0, b1 = c1;
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL(mst_fold_kernel<decltype(wp)::value>, grid, block, 0, s, a, ot0, b0, b1, per);
        return hipGetLastError();
    });
}

hipError_t launch_mst_init(const MstState& m, hipStream_t s)
{
    hipLaunchKernelGGL(mst_init_kernel, rows_grid(m.nrows > kMstCtlWords ? m.nrows : kMstCtlWords), dim3(256), 0, s, m);
    return hipGetLastError();
}

hipError_t mst_select_bytes(uint64_t nrows, size_t* bytes)
{
    *bytes = 0;
    return rocprim::select(nullptr, *bytes, rocprim::counting_iterator<uint32_t>(0), static_cast<const uint32_t*>(nullptr),
                           static_cast<uint32_t*>(nullptr), static_cast<unsigned long long*>(nullptr), static_cast<size_t>(nrows));
}

hipError_t launch_mst_round(const MstState& m, void* tmp, size_t tmp_bytes, hipStream_t s)
{
    if (m.nrows == 0) return hipSuccess;
    const dim3 grid = rows_grid(m.nrows), block(256);
    hipLaunchKernelGGL(mst_reset_kernel, grid, block, 0, s, m);
    hipLaunchKernelGGL(mst_pick_score_kernel, grid, block, 0, s, m);
    hipLaunchKernelGGL(mst_pick_edge_kernel, grid, block, 0, s, m);
    hipLaunchKernelGGL(mst_hook_kernel, grid, block, 0, s, m);
    hipLaunchKernelGGL(mst_flatten_kernel, grid, block, 0, s, m);
    hipLaunchKernelGGL(mst_relabel_kernel, grid, block, 0, s, m);
    hipLaunchKernelGGL(mst_flag_kernel, grid, block, 0, s, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = tmp_bytes;
    return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint32_t>(0), static_cast<const uint32_t*>(m.flag), m.own,
                           m.ctl + kMstCtlOwners, static_cast<size_t>(m.nrows), s);
}

hipError_t launch_mst_count_roots(const MstState& m, hipStream_t s)
{
    if (m.nrows == 0) return hipSuccess;
    hipLaunchKernelGGL(mst_count_roots_kernel, rows_grid(m.nrows), dim3(256), 0, s, m);
    return hipGetLastError();
}

hipError_t mst_sort_bytes(uint64_t n, size_t* bytes)
{
    size_t by_b = 0, by_key = 0;
    *bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, by_b, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                             static_cast<const u64*>(nullptr), static_cast<u64*>(nullptr), static_cast<size_t>(n), 0, 32);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, by_key, static_cast<const u64*>(nullptr), static_cast<u64*>(nullptr),
                                  static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<size_t>(n), 0, 64);
    *bytes = by_b > by_key ? by_b : by_key;
    return e;
}

hipError_t launch_mst_sort(const MstState& m, uint64_t n, void* tmp, size_t tmp_bytes, unsigned long long* ekey2, uint32_t* eb2,
                           uint32_t row_base, void* edges, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (n > m.cap) return hipErrorInvalidValue;
    // stable, least significant key first: by b, then by (score descending, a)
    size_t bytes = tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, static_cast<const uint32_t*>(m.eb), eb2, reinterpret_cast<const u64*>(m.ekey),
                                             reinterpret_cast<u64*>(ekey2), static_cast<size_t>(n), 0, 32, s);
    if (e != hipSuccess) return e;
    bytes = tmp_bytes;
    e = rocprim::radix_sort_pairs(tmp, bytes, reinterpret_cast<const u64*>(ekey2), reinterpret_cast<u64*>(m.ekey), static_cast<const uint32_t*>(eb2),
                                  m.eb, static_cast<size_t>(n), 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mst_emit_kernel, rows_grid(n), dim3(256), 0, s, reinterpret_cast<const u64*>(m.ekey), static_cast<const uint32_t*>(m.eb),
                       static_cast<u64>(n), row_base, static_cast<MstEdgeOut*>(edges));
    return hipGetLastError();
}

} // namespace gsim
