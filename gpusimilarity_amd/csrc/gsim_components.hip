// gsim_components.hip -- single-linkage clustering (the connected components of the threshold graph "score >= cutoff") behind
// gsim_db_components: the pair scoring of gsim_neighbors.hip's tile kernel, every kept pair fed to a union-find forest in device
// memory instead of being stored, one forest per cutoff level.  Nothing of the graph is ever written.
//
// Tile kernel (comp_tile_kernel<WP, L>): the held-row pair count of gsim_held_row.h in nbr_tile_kernel's upper-triangle layout -- a
// workgroup owns kNbrTile x kNbrTile rows, each lane of its four waves holds one right row, the left rows are the uniform side, the
// division-free band of gsim_prefilter.h runs against cutoffs[0] (the loosest level) and the divide only where a lane may be kept.  ONE pass per
// tile: no counting pass, no cursor, no pair stores.  A kept pair (i, j), j > i, with score s unites i and j in forest l for every
// level l with s >= cutoffs[l].
//
// THE FOREST PROTOCOL.  parent_l is forest l: N words.
//   1. parent_l[x] <= x, always; comp_init_kernel sets parent_l[x] = x before the first launch.  A root is an x with
//      parent_l[x] == x.
//   2. The tile kernel writes `parent` in ONE place: the hook atomicCAS(&parent[hi], hi, lo) with lo < hi, both roots as the
//      hooking lane last saw them (each by an agent-scope load of its own parent word right before).  So only a root is ever
//      hooked, and it is hooked once.  ALL path shortening is in comp_flatten_kernel, which runs between launches and after the
//      last one and stores parent[x] = root(x) -- an ancestor of x.  The tile kernel shortens nothing.
//   3. A value read from parent[x] may be stale (a compute unit's L1 is never refreshed by another one's writes).  Whatever was
//      once stored in parent[x] is a member of x's component for the rest of the call, so "the same node reached from i and from
//      j => same component" holds with any mix of stale and fresh values, and so does uniting any member of i's component with any
//      member of j's.  A stale "x is a root" is caught by the CAS, which is performed in L2.
//   4. After a failed CAS the climb continues from the value the CAS returned, not from a reload.  Every load of `parent` in the
//      tile kernel -- the cached hints included -- is an agent-scope relaxed atomic load: served by L2, so no lane climbs a stale
//      line twice.
//   5. Nothing waits for another wave.  A climb only moves to smaller rows; a failed CAS means another hook of that root
//      succeeded, and there are at most N - 1 hooks per level: every loop terminates whatever the other waves do.  No spin-waits,
//      no locks, no grid-wide waits.
//   6. After the last launch every pair of the level's graph has been united, so each component is one tree; a tree's root is
//      its smallest row because of 1.  root(x) = the smallest row of x's component, whatever the order of the unions: the
//      outputs are byte-identical from run to run and do not depend on how the pass is cut into launches.
//
// THE ROOT CACHE keeps dense data from turning into memory traffic.  Per level, each lane keeps a member of its right row's
// component -- the last root it knows (L VGPRs, read from parent_l[j] at the start of the tile), and each wave keeps one for
// each of the next 64 left rows (L VGPRs, a lane per left row, refreshed from parent_l every 64 left rows and read back with
// v_readlane: wave-uniform).  A kept pair whose two cached values are equal costs nothing beyond its score.  Otherwise the wave
// unites until every kept lane holds the left row's root -- where the lanes that differ all hold ONE value, one lane unites for all
// of them; else every lane unites for itself and the wave takes the smallest root -- and both caches take the result.  Cached
// values need only be members of the right component (3), so nothing ever invalidates them.  On a table of identical rows all lanes
// soon hold the component's root and so does every refreshed hint: whole wave-tiles touch no memory beyond the refresh.
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

__global__ __launch_bounds__(256) void comp_init_kernel(uint32_t* __restrict__ parent, u64 nrows, u64 total)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (t < total) parent[t] = static_cast<uint32_t>(t % nrows);
}

template <int WP, int L> __global__ __launch_bounds__(kNbrBlock) void comp_tile_kernel(CompArgs a, uint32_t rt0, uint32_t ct0)
{
    const uint32_t rt = rt0 + blockIdx.y;
    const uint32_t ct = ct0 + blockIdx.x;
    if (ct < rt) return; // below the diagonal: that pair is found from the other side
    const int lane = threadIdx.x & 63;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    const u64 i0 = static_cast<u64>(rt) * kNbrTile;
    if (i0 >= a.nrows) return;
    const u64 iend = i0 + kNbrTile < a.nrows ? i0 + kNbrTile : a.nrows;
    // the clock this launch ran at: shader cycles (s_memtime) against the 100 MHz wall clock over one full tile
    const bool stamp = a.clk && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 j = static_cast<u64>(ct) * kNbrTile + wib * 64u + static_cast<uint32_t>(lane);
    const bool jin = j < a.nrows;

    HeldRow<WP> right; // this lane's right row
    const uint32_t b = right.load(a.rows, jin ? j : 0, jin);

    uint32_t nl = static_cast<uint32_t>(iend - i0);
    // diagonal tile: left row i0 + t pairs with some right row of this wave only if t < 64 wib + 63
    if (ct == rt && nl > wib * 64u + 63u) nl = wib * 64u + 63u;

    // the root cache: rj[l] a member of the right row's component, vroot[l] one of left row (t & ~63) + lane's
    uint32_t rj[L], vroot[L];
#pragma unroll
    for (int l = 0; l < L; l++) {
        rj[l] = static_cast<uint32_t>(j);
        vroot[l] = 0;
        if (l < static_cast<int>(a.nlevels) && jin) rj[l] = parent_load(a.parent + static_cast<u64>(l) * a.nrows + j);
    }

    const float cut0 = a.cutoffs[0];
    const float cut_lo = valu_cutoff_lo(cut0);
    const const_u32x4p lrows = (const_u32x4p) (a.rows) + i0 * (WP / 4);
    Handout64 vpop; // popc of the left rows
    uint32_t kept = 0, hooks = 0, lost = 0;
    for (uint32_t t = 0; t < nl; t++) {
        if (Handout64::due(t)) { // ... and their cached roots, one per lane too
            vpop.fetch(a.pop, i0 + t, static_cast<uint32_t>(lane), iend);
            const u64 il = i0 + t + static_cast<uint32_t>(lane);
#pragma unroll
            for (int l = 0; l < L; l++)
                if (l < static_cast<int>(a.nlevels)) vroot[l] = il < iend ? parent_load(a.parent + static_cast<u64>(l) * a.nrows + il) : 0u;
        }
        const uint32_t av = vpop.get(t);
        // left row t against this lane's right row: keep == (score_of(...) >= cutoffs[0]), s = that score
        const const_u32x4p qw = lrows + static_cast<u64>(t) * (WP / 4);
        const uint32_t c = right.common(qw);
        const u64 i = i0 + t;
        const bool valid = jin && j > i;
        const float den = score_den(a.metric, a.alpha, a.beta, av, b, c);
        const float cf = static_cast<float>(c);
        const bool maybe = valid && !valu_surely_not_kept(cut_lo, cf, den, c);
        if (__ballot(maybe) == 0) continue;
        const float s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, av, b, c)
        const bool keep = maybe && s >= cut0;
        const u64 m = __ballot(keep);
        if (m == 0) continue;
        kept += static_cast<uint32_t>(__popcll(m));
#pragma unroll
        for (int l = 0; l < L; l++) {
            if (l >= static_cast<int>(a.nlevels)) break;
            const bool kl = keep && s >= a.cutoffs[l];
            if (__ballot(kl) == 0) break; // (the cutoffs ascend: no lane is kept at a later level either)
            uint32_t ri = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(vroot[l]), static_cast<int>(t & 63u)));
            u64 need = __ballot(kl && rj[l] != ri);
            if (need == 0) continue;
            uint32_t* parent = a.parent + static_cast<u64>(l) * a.nrows;
            // until every kept lane holds the left row's root.  Where they all hold ONE other value (dense data after the first
            // left row) one lane unites for all of them; else every lane unites for itself and the wave takes the smallest root
            while (need) {
                const int src = __builtin_ctzll(need);
                const uint32_t rb = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(rj[l]), src));
                const bool mine = kl && rj[l] != ri;
                if ((need & ~__ballot(mine && rj[l] == rb)) == 0) {
                    uint32_t r = 0;
                    if (lane == src) r = comp_unite(parent, ri, rb, hooks, lost);
                    ri = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(r), src));
                    if (mine) rj[l] = ri;
                } else {
                    if (mine) rj[l] = comp_unite(parent, ri, rj[l], hooks, lost);
                    ri = wave_min(mine ? rj[l] : ri);
                }
                need = __ballot(kl && rj[l] != ri);
            }
            if (static_cast<uint32_t>(lane) == (t & 63u)) vroot[l] = ri;
        }
    }
    // one atomic add per wave-tile and counter (integer adds commute)
    if (kept && lane == 0) atomicAdd(a.counters + 0, static_cast<u64>(kept));
    const u64 any = __ballot(hooks | lost);
    if (any) {
        hooks = wave_sum(hooks);
        lost = wave_sum(lost);
        if (lane == 0) {
            if (hooks) atomicAdd(a.counters + 1, static_cast<u64>(hooks));
            if (lost) atomicAdd(a.counters + 2, static_cast<u64>(lost));
        }
    }
    if (stamp) stamp_end(a.clk);
}

// parent_l[x] = root(x), one thread per (level, row): every thread climbs to its root (other threads' stores only ever put an
// ancestor in the place of an ancestor) and stores it
__global__ __launch_bounds__(256) void comp_flatten_kernel(uint32_t* __restrict__ parent, u64 nrows, u64 total)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= total) return;
    uint32_t* forest = parent + (t / nrows) * nrows;
    const uint32_t x = static_cast<uint32_t>(t % nrows);
    uint32_t r = x;
    for (;;) {
        const uint32_t p = parent_load(forest + r);
        if (p == r) break;
        r = p;
    }
    if (r != x) __hip_atomic_store(forest + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// labelling of one flattened forest: flag the roots ...
__global__ __launch_bounds__(256) void comp_flag_kernel(const uint32_t* __restrict__ parent, u64 nrows, uint32_t* __restrict__ flag)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x < nrows) flag[x] = parent[x] == x ? 1u : 0u;
}

// ... and, num = the exclusive scan of the flags (a root's number: components in ascending order of their smallest row):
// component_of by gather, first_row by scatter, sizes by integer atomic adds (zeroed before), the count from the last row
__global__ __launch_bounds__(256) void comp_label_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ num, u64 nrows,
                                                         uint32_t row_base, uint32_t* __restrict__ component_of,
                                                         uint32_t* __restrict__ first_row, uint32_t* __restrict__ sizes,
                                                         uint32_t* __restrict__ ncomponents)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (x >= nrows) return;
    const uint32_t r = parent[x];
    const uint32_t c = num[r];
    component_of[x] = c;
    if (r == x && first_row) first_row[c] = static_cast<uint32_t>(x) + row_base;
    if (sizes) atomicAdd(sizes + c, 1u);
    if (x == nrows - 1) *ncomponents = num[x] + (r == x ? 1u : 0u);
}

template <int WP> hipError_t launch_tiles_wp(const CompArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s)
{
    const dim3 grid(nct, nrt), block(kNbrBlock);
    if (a.nlevels <= 1) hipLaunchKernelGGL((comp_tile_kernel<WP, 1>), grid, block, 0, s, a, rt0, ct0);
    else if (a.nlevels <= 2) hipLaunchKernelGGL((comp_tile_kernel<WP, 2>), grid, block, 0, s, a, rt0, ct0);
    else if (a.nlevels <= 4) hipLaunchKernelGGL((comp_tile_kernel<WP, 4>), grid, block, 0, s, a, rt0, ct0);
    else hipLaunchKernelGGL((comp_tile_kernel<WP, 8>), grid, block, 0, s, a, rt0, ct0);
    return hipGetLastError();
}

} // namespace

hipError_t launch_comp_init(uint32_t* parent, uint64_t nrows, uint32_t nlevels, hipStream_t s)
{
    const u64 total = static_cast<u64>(nrows) * nlevels;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(comp_init_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, parent, static_cast<u64>(nrows), total);
    return hipGetLastError();
}

hipError_t launch_comp_tiles(const CompArgs& a, uint32_t rt0, uint32_t nrt, uint32_t ct0, uint32_t nct, hipStream_t s)
{
    if (a.nlevels < 1 || a.nlevels > kCompMaxLevels) return hipErrorInvalidValue;
    return dispatch_wp(a.WP, [&](auto wp) { return launch_tiles_wp<decltype(wp)::value>(a, rt0, nrt, ct0, nct, s); });
}

hipError_t launch_comp_flatten(uint32_t* parent, uint64_t nrows, uint32_t nlevels, hipStream_t s)
{
    const u64 total = static_cast<u64>(nrows) * nlevels;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(comp_flatten_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, parent, static_cast<u64>(nrows), total);
    return hipGetLastError();
}

hipError_t launch_comp_label(void* tmp, size_t tmp_bytes, const uint32_t* parent, uint64_t nrows, uint32_t row_base, uint32_t* flag,
                             uint32_t* num, uint32_t* component_of, uint32_t* first_row, uint32_t* sizes, uint32_t* ncomponents,
                             hipStream_t s)
{
    if (nrows == 0) return hipSuccess;
    const dim3 grid(static_cast<uint32_t>((nrows + 255) / 256)), block(256);
    hipLaunchKernelGGL(comp_flag_kernel, grid, block, 0, s, parent, static_cast<u64>(nrows), flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan_u32(tmp, tmp_bytes, flag, num, nrows, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(comp_label_kernel, grid, block, 0, s, parent, static_cast<const uint32_t*>(num), static_cast<u64>(nrows), row_base,
                       component_of, first_row, sizes, ncomponents);
    return hipGetLastError();
}

} // namespace gsim
