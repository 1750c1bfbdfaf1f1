// gsim_dbscan.hip -- DBSCAN density clustering behind gsim_db_dbscan: two passes over the pairs of the upper triangle, neither of
// which stores any of the graph "score >= cutoff".  The rule is stated in include/gpusim_hip.h; the host side is capi_dbscan.cpp.
//
// Both passes are comp_tile_kernel's tile (gsim_components.hip): a workgroup owns kNbrTile x kNbrTile rows, each lane of its four
// waves holds one right row (HeldRow), the left rows are the wave-uniform side and come through the scalar path, Handout64 hands out
// their popcounts, the division-free band of gsim_prefilter.h runs against the cutoff and the one divide only where a lane may be
// kept.  A pair (i, j), j > i, is kept when score(i, j) >= cutoff.
//
// DEGREE PASS (dbscan_count_kernel).  A kept pair adds one to degree[i] and to degree[j].  The right row's count lives in a VGPR and
// is added once per lane at the end of the tile; the left row's is popc(ballot of the kept lanes), accumulated in the wave's lane
// t & 63 and flushed at every 64-row refresh and at the end.  Integer adds commute: degree[] does not depend on the order of the
// tiles or on how the pass is cut into launches.
//
// LINK PASS (dbscan_link_kernel).  core(x) = degree[x] + 1 >= min_pts is read from the finished degrees: 64 at a time for the left
// rows (a second Handout64), once into a register for the lane's right row.  A kept pair with
//   * both rows core is united in ONE forest over all N rows, by the forest protocol of gsim_components.hip unchanged
//     (gsim_forest.h): the hook atomicCAS(&parent[hi], hi, lo), lo < hi, is the kernel's only write to `parent`, every load of
//     `parent` is an agent-scope relaxed load, the kernel shortens no paths, and launch_comp_flatten runs after every launch.  The
//     root cache is comp_tile_kernel's with one level.  A non-core row is never united, so it stays a root of its own;
//   * exactly one row core publishes key(score, core row) = (bits of score << 32) | ~core row to best[the non-core row] with a
//     64-bit atomicMax: gsim_mst.hip's key, larger for a larger score and, among equal scores, for the smaller row.  Max over a total
//     order commutes, so best[x] ends as the key of x's anchor whatever the order.  Where the non-core row is the lane's own right row
//     the lane keeps the largest key in a register and publishes once per tile; where it is the left row the wave takes the largest
//     key of its lanes and one lane publishes.  0 is "no core neighbour": a kept score is >= cutoff > 0, so a real key is not 0;
//   * neither row core does nothing.
// THE SKIP: where the left row is not a core and no lane of the wave holds a core, no pair of that left row can matter, and the wave
// goes to the next left row before it reads this one's words.  It changes no output (DbscanArgs::skip = 0 turns it off, for timing).
//
// WHY EVERY LOOP TERMINATES: as in gsim_components.hip (5).  Nothing waits for another wave: a climb only moves to smaller rows, a
// failed compare-and-swap means that another hook of that root succeeded, and there are at most N - 1 hooks.  The atomicMax and the
// integer adds are single instructions.  No spin-waits, no locks, no grid-wide waits, no LDS: stream order is the only dependency
// between launches, and between the passes.
//
// LABELS (launch_dbscan_label), on the flattened forest: flag the CORE roots (a non-core row is a root too, but no cluster), number
// them by an exclusive scan -- clusters in ascending order of their smallest core row -- and then, one thread per row: a core takes
// its root's number and is its own anchor; a non-core row with best[x] != 0 is a border row, takes the number of its anchor's root
// and is added to that cluster's size with an integer atomic; any other row is noise.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_forest.h"
#include "gsim_held_row.h"
#include "gsim_prefilter.h"

namespace gsim
{
namespace
{

__device__ __forceinline__ u64 wave_max64(u64 x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}

__device__ __forceinline__ u64 wave_sum64(u64 x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__device__ __forceinline__ u64 anchor_key(float s, uint32_t core_row)
{
    return (static_cast<u64>(__float_as_uint(s)) << 32) | static_cast<uint32_t>(~core_row);
}

template <int WP> __global__ __launch_bounds__(kNbrBlock) void dbscan_count_kernel(DbscanArgs a, uint32_t rt0, uint32_t ct0)
{
    const uint32_t rt = rt0 + blockIdx.y;
    const uint32_t ct = ct0 + blockIdx.x;
    if (ct < rt) return; // below the diagonal: that pair is found from the other side
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    const u64 i0 = static_cast<u64>(rt) * kNbrTile;
    if (i0 >= a.nrows) return;
    const u64 iend = i0 + kNbrTile < a.nrows ? i0 + kNbrTile : a.nrows;
    const bool stamp = a.clk && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 j = static_cast<u64>(ct) * kNbrTile + wib * 64u + lane;
    const bool jin = j < a.nrows;

    HeldRow<WP> right; // this lane's right row
    const uint32_t b = right.load(a.rows, jin ? j : 0, jin);

    uint32_t nl = static_cast<uint32_t>(iend - i0);
    // diagonal tile: left row i0 + t pairs with some right row of this wave only if t < 64 wib + 63
    if (ct == rt && nl > wib * 64u + 63u) nl = wib * 64u + 63u;

    const float cut_lo = valu_cutoff_lo(a.cutoff);
    const const_u32x4p lrows = (const_u32x4p) (a.rows) + i0 * (WP / 4);
    Handout64 vpop;  // popc of the left rows
    uint32_t dj = 0; // kept pairs of this lane's right row
    uint32_t dl = 0; // ... of left row (t & ~63) + lane
    uint32_t kept = 0;
    for (uint32_t t = 0; t < nl; t++) {
        if (Handout64::due(t)) {
            if (dl) atomicAdd(a.degree + i0 + (t - 64u) + lane, dl); // (dl != 0 only from t = 64 on)
            dl = 0;
            vpop.fetch(a.pop, i0 + t, lane, iend);
        }
        const uint32_t av = vpop.get(t);
        const const_u32x4p qw = lrows + static_cast<u64>(t) * (WP / 4);
        const uint32_t c = right.common(qw);
        const u64 i = i0 + t;
        const bool valid = jin && j > i;
        const float den = score_den(a.metric, a.alpha, a.beta, av, b, c);
        const float cf = static_cast<float>(c);
        const bool maybe = valid && !valu_surely_not_kept(cut_lo, cf, den, c);
        if (__ballot(maybe) == 0) continue;
        const float s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, av, b, c)
        const bool keep = maybe && s >= a.cutoff;
        const u64 m = __ballot(keep);
        if (m == 0) continue;
        const uint32_t n = static_cast<uint32_t>(__popcll(m));
        kept += n;
        if (keep) dj++;
        if (lane == (t & 63u)) dl += n;
    }
    if (dl) atomicAdd(a.degree + i0 + ((nl - 1u) & ~63u) + lane, dl); // (dl != 0: a left row of the last 64, so nl >= 1)
    if (dj) atomicAdd(a.degree + j, dj);
    if (kept && lane == 0) atomicAdd(a.counters + kDbscanKept, static_cast<u64>(kept));
    if (stamp) stamp_end(a.clk);
}

template <int WP> __global__ __launch_bounds__(kNbrBlock) void dbscan_link_kernel(DbscanArgs a, uint32_t rt0, uint32_t ct0)
{
    const uint32_t rt = rt0 + blockIdx.y;
    const uint32_t ct = ct0 + blockIdx.x;
    if (ct < rt) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    const u64 i0 = static_cast<u64>(rt) * kNbrTile;
    if (i0 >= a.nrows) return;
    const u64 iend = i0 + kNbrTile < a.nrows ? i0 + kNbrTile : a.nrows;
    const bool stamp = a.clk && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 j = static_cast<u64>(ct) * kNbrTile + wib * 64u + lane;
    const bool jin = j < a.nrows;

    HeldRow<WP> right;
    const uint32_t b = right.load(a.rows, jin ? j : 0, jin);

    uint32_t nl = static_cast<uint32_t>(iend - i0);
    if (ct == rt && nl > wib * 64u + 63u) nl = wib * 64u + 63u;

    // is the right row a core?  (degree < N < 2^32: the sum does not wrap)
    const bool cj = jin && a.degree[j] + 1u >= a.min_pts;
    const bool any_right = __ballot(cj) != 0;
    // the root cache: rj a member of the right row's component, vroot one of left row (t & ~63) + lane's (cores only)
    uint32_t rj = static_cast<uint32_t>(j), vroot = 0;
    if (cj) rj = parent_load(a.parent + j);
    u64 held = 0; // the best key(score, core left row) of a non-core right row

    const float cut_lo = valu_cutoff_lo(a.cutoff);
    const const_u32x4p lrows = (const_u32x4p) (a.rows) + i0 * (WP / 4);
    Handout64 vpop, vdeg; // popc and degree of the left rows
    uint32_t hooks = 0, lost = 0;
    for (uint32_t t = 0; t < nl; t++) {
        if (Handout64::due(t)) {
            vpop.fetch(a.pop, i0 + t, lane, iend);
            vdeg.fetch(a.degree, i0 + t, lane, iend);
            const u64 il = i0 + t + lane;
            vroot = il < iend ? parent_load(a.parent + il) : 0u;
        }
        const bool li = vdeg.get(t) + 1u >= a.min_pts; // is the left row a core?  (wave-uniform)
        if (a.skip && !li && !any_right) continue;     // no pair of this left row and this wave's right rows has a core
        const uint32_t av = vpop.get(t);
        const const_u32x4p qw = lrows + static_cast<u64>(t) * (WP / 4);
        const uint32_t c = right.common(qw);
        const u64 i = i0 + t;
        const bool valid = jin && j > i && (li || cj);
        const float den = score_den(a.metric, a.alpha, a.beta, av, b, c);
        const float cf = static_cast<float>(c);
        const bool maybe = valid && !valu_surely_not_kept(cut_lo, cf, den, c);
        if (__ballot(maybe) == 0) continue;
        const float s = __fdiv_rn(cf, den);
        const bool keep = maybe && s >= a.cutoff;
        if (__ballot(keep) == 0) continue;
        if (!li) { // the kept lanes hold cores: the left row takes the best of them
            const u64 key = wave_max64(keep ? anchor_key(s, static_cast<uint32_t>(j)) : 0ull);
            if (lane == 0) atomicMax(a.best + i, key);
            continue;
        }
        if (keep && !cj) { // a non-core right row next to a core left row
            const u64 key = anchor_key(s, static_cast<uint32_t>(i));
            held = key > held ? key : held;
        }
        const bool kl = keep && cj; // both cores: one component
        if (__ballot(kl) == 0) continue;
        uint32_t ri = readlane_u32(vroot, t & 63u);
        u64 need = __ballot(kl && rj != ri);
        if (need == 0) continue;
        // until every kept lane holds the left row's root, as comp_tile_kernel does: where they all hold ONE other value one lane
        // unites for all of them; else every lane unites for itself and the wave takes the smallest root
        while (need) {
            const int src = __builtin_ctzll(need);
            const uint32_t rb = readlane_u32(rj, static_cast<uint32_t>(src));
            const bool mine = kl && rj != ri;
            if ((need & ~__ballot(mine && rj == rb)) == 0) {
                uint32_t r = 0;
                if (lane == static_cast<uint32_t>(src)) r = comp_unite(a.parent, ri, rb, hooks, lost);
                ri = readlane_u32(r, static_cast<uint32_t>(src));
                if (mine) rj = ri;
            } else {
                if (mine) rj = comp_unite(a.parent, ri, rj, hooks, lost);
                ri = wave_min(mine ? rj : ri);
            }
            need = __ballot(kl && rj != ri);
        }
        if (lane == (t & 63u)) vroot = ri;
    }
    if (held) atomicMax(a.best + j, held); // (held != 0: a kept pair, so j is a row)
    const u64 any = __ballot(hooks | lost);
    if (any) {
        hooks = wave_sum(hooks);
        lost = wave_sum(lost);
        if (lane == 0) {
            if (hooks) atomicAdd(a.counters + kDbscanUnions, static_cast<u64>(hooks));
            if (lost) atomicAdd(a.counters + kDbscanCasFailed, static_cast<u64>(lost));
        }
    }
    if (stamp) stamp_end(a.clk);
}

// the clusters' roots: the cores that are roots of the flattened forest
__global__ __launch_bounds__(256) void dbscan_flag_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ degree,
                                                          uint32_t min_pts, u64 nrows, uint32_t* __restrict__ flag)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x < nrows) flag[x] = (parent[x] == x && degree[x] + 1u >= min_pts) ? 1u : 0u;
}

// num = the exclusive scan of the flags.  One thread per row (head comment, LABELS); sizes zeroed before
__global__ __launch_bounds__(256) void dbscan_label_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ num,
                                                           const uint32_t* __restrict__ flag, const uint32_t* __restrict__ degree,
                                                           const u64* __restrict__ best, uint32_t min_pts, u64 nrows, uint32_t row_base,
                                                           uint32_t* __restrict__ label_of, uint32_t* __restrict__ anchor,
                                                           uint32_t* __restrict__ first_row, uint32_t* __restrict__ sizes,
                                                           uint32_t* __restrict__ nclusters, unsigned long long* __restrict__ counters)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    const bool in = x < nrows;
    bool core = false, border = false;
    uint32_t deg = 0;
    if (in) {
        deg = degree[x];
        core = deg + 1u >= min_pts;
        const u64 k = core ? 0ull : best[x];
        border = k != 0;
        uint32_t label = GSIM_DBSCAN_NOISE, anc = GSIM_DBSCAN_NOISE;
        if (core || border) {
            const uint32_t arow = core ? static_cast<uint32_t>(x) : ~static_cast<uint32_t>(k);
            const uint32_t r = parent[arow];
            label = num[r];
            anc = arow + row_base;
            if (core && r == x && first_row) first_row[label] = anc;
            if (sizes) atomicAdd(sizes + label, 1u);
        }
        label_of[x] = label;
        if (anchor) anchor[x] = anc;
        if (x == nrows - 1) *nclusters = num[x] + flag[x];
    }
    // the census, one add per wave and counter
    const u64 mc = __ballot(core), mb = __ballot(border), mi = __ballot(in);
    const u64 dsum = wave_sum64(deg);
    if ((threadIdx.x & 63u) == 0 && mi) {
        if (mc) atomicAdd(counters + kDbscanCores, static_cast<u64>(__popcll(mc)));
        if (mb) atomicAdd(counters + kDbscanBorders, static_cast<u64>(__popcll(mb)));
        if (mi & ~(mc | mb)) atomicAdd(counters + kDbscanNoise, static_cast<u64>(__popcll(mi & ~(mc | mb))));
        if (dsum) atomicAdd(counters + kDbscanDegreeSum, dsum);
    }
}

} // namespace

hipError_t launch_dbscan_count(const DbscanArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s)
{
    const dim3 grid(nct, nrt), block(kNbrBlock);
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL(dbscan_count_kernel<decltype(wp)::value>, grid, block, 0, s, a, rt0, ct0);
        return hipGetLastError();
    });
}

hipError_t launch_dbscan_link(const DbscanArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s)
{
    const dim3 grid(nct, nrt), block(kNbrBlock);
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL(dbscan_link_kernel<decltype(wp)::value>, grid, block, 0, s, a, rt0, ct0);
        return hipGetLastError();
    });
}

hipError_t launch_dbscan_label(void* tmp, size_t tmp_bytes, const DbscanArgs& a, uint32_t row_base, uint32_t* flag, uint32_t* num,
                               uint32_t* label_of, uint32_t* anchor, uint32_t* first_row, uint32_t* sizes, uint32_t* nclusters, hipStream_t s)
{
    if (a.nrows == 0) return hipSuccess;
    const dim3 grid(static_cast<uint32_t>((a.nrows + 255) / 256)), block(256);
    hipLaunchKernelGGL(dbscan_flag_kernel, grid, block, 0, s, static_cast<const uint32_t*>(a.parent), static_cast<const uint32_t*>(a.degree),
                       a.min_pts, static_cast<u64>(a.nrows), flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan_u32(tmp, tmp_bytes, flag, num, a.nrows, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dbscan_label_kernel, grid, block, 0, s, static_cast<const uint32_t*>(a.parent), static_cast<const uint32_t*>(num),
                       static_cast<const uint32_t*>(flag), static_cast<const uint32_t*>(a.degree), reinterpret_cast<const u64*>(a.best), a.min_pts,
                       static_cast<u64>(a.nrows), row_base, label_of, anchor, first_row, sizes, nclusters, a.counters);
    return hipGetLastError();
}

} // namespace gsim
