// gsim_mreach.hip -- the fold kernel of the mutual-reachability forest behind gsim_db_mreach_mst / gsim_db_hdbscan, and the tail of
// the core pass behind gsim_db_core_scores.  The rule is stated in include/gpusim_hip.h; the host side is capi_hdbscan.cpp.  The
// rounds' bookkeeping, the owner list and the final sort are gsim_mst.hip's, unchanged: only the value of a pair differs.
//
// The value of a pair is m(i, j) = min(score(i, j), core[i], core[j]), where core[] is a side array of N floats (the score of the
// row's (min_pts - 1)-th nearest neighbour, or 0.0f for a row that has fewer: such a row has no edge at all).  ORDER E on the
// pairs a < b is (m descending, a ascending, b ascending).
//
// Fold kernel: mst_fold_kernel's scheme (gsim_mst.hip) with one more side array.
//   * a workgroup is kKnnTile owners, 64 to a wave, one whole fingerprint per lane in VGPRs, through the round's index list; the
//     candidates j of the workgroup's piece of [c0, c1) are walked in ascending order; their words come through the scalar path;
//     popc(j), comp[j] AND core[j] of the next 64 candidates are read one per lane and handed out with v_readlane; the owner's
//     component id and core score sit in registers;
//   * cap = min(core[i], core[j]), as bit patterns (non-negative floats order as their bits do).  A pair is dead when
//     comp[j] == comp[i], or cap < cutoff (one of the two rows is not dense at any level of this call: that covers the idle lanes,
//     whose core is 0), or key(cap, j) <= the held key: m <= cap, so key(cap, j) is the best key the pair can have, and it loses
//     to what the lane holds whatever its score is.  That is "cap below the held value", and also "cap equal to it at a partner
//     beyond the held one" -- the state of a dense row once it holds an edge at its own core score: every later candidate whose
//     core is no smaller is capped at exactly that value.  All of that is known before the candidate's words are read, and where
//     no lane of the wave has a live pair they are not read;
//   * then the division-free band of gsim_prefilter.h against the LANE's tau: the cutoff until the lane holds an edge, the held
//     value afterwards.  m <= score, so a pair whose score is surely below tau has m below the held value: the band prunes nothing
//     that could win;
//   * a lane holds ONE 64-bit word, key(m, j) = (bits of m << 32) | ~j, 0 for nothing, and accepts when score >= cutoff and
//     key(m, j) > the held key (cap >= cutoff is part of `live`, so m >= cutoff);
//   * WHY THE LARGEST KEY IS STILL THE ROW'S E-FIRST FOREIGN EDGE.  gsim_mst.hip's argument uses two facts only: the pair's value is
//     symmetric -- m(i, j) = m(j, i) bit for bit, because the score is and min commutes -- so both ends see the same value for the
//     edge; and for a fixed row i the key orders (value descending, partner ascending).  Among partners of equal value a partner
//     p < i gives a = p < i and a partner p > i gives a = i, two partners below i are ordered by a = p, two above by b = p: the
//     smaller p is earlier in E in every case.  Nothing in it asks where the value comes from;
//   * WHY THE OWNER LIST STAYS VALID.  core[] is fixed before the first round, so m(i, j) does not change between rounds: a row's
//     held edge stays its E-first foreign edge for as long as its partner is foreign, because candidates only ever disappear.  A
//     row that scanned and holds nothing has no foreign pair with m >= cutoff and never scans again -- the rows with core 0 among
//     them, after the first scan, in which every one of their pairs dies before a word is read;
//   * best[i] carries from launch to launch exactly as in gsim_mst.hip: one 64-bit atomicMax at the end, max over a total order
//     commutes, a stale value read at the start is a key some piece really found and only prunes what loses to it.
// No per-thread array is indexed at run time, no scratch, no LDS, no barrier, no grid-wide wait, no spin-wait.
// (Not built: a wave-uniform early EXIT from the walk once every lane holds a key whose value equals its own core score.  The
// dead-pair test above already retires every pair such a lane still meets, one ballot per candidate -- DESIGN.md section 28.)
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

template <int WP> __global__ __launch_bounds__(kKnnBlock) void mreach_fold_kernel(MreachArgs ma, uint32_t ot0, u64 c0, u64 c1, u64 per)
{
    const MstArgs& a = ma.mst;
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
    const uint32_t ki = oin ? __float_as_uint(ma.core[i]) : 0u; // (an idle lane is not dense: all its pairs are dead)
    const uint32_t kcut = __float_as_uint(a.cutoff);
    const u64 found = oin ? __hip_atomic_load(a.best + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    u64 held = found;
    float cut_lo = valu_cutoff_lo(held ? __uint_as_float(static_cast<uint32_t>(held >> 32)) : a.cutoff);

    const const_u32x4p crows = (const_u32x4p) (a.rows);
    uint32_t vpop = 0, vcomp = 0, vcore = 0;
    for (u64 j = p0; j < p1; j++) {
        const uint32_t t = static_cast<uint32_t>(j - p0);
        if ((t & 63u) == 0) { // popc, component and core score of the next 64 candidates, one per lane (read back with v_readlane)
            const u64 jl = j + lane;
            vpop = jl < p1 ? a.pop[jl] : 0u;
            vcomp = jl < p1 ? a.comp[jl] : 0u;
            vcore = jl < p1 ? __float_as_uint(ma.core[jl]) : 0u;
        }
        const uint32_t cj = readlane_u32(vcomp, t & 63u);
        const uint32_t kj = readlane_u32(vcore, t & 63u);
        const uint32_t cap = ki < kj ? ki : kj;
        const u64 top = (static_cast<u64>(cap) << 32) | static_cast<uint32_t>(~static_cast<uint32_t>(j)); // the pair's best possible key
        const bool live = cj != ci && cap >= kcut && top > held;
        if (__ballot(live) == 0) continue; // one component, or not dense, or capped at or below what every lane holds
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
        const uint32_t sb = __float_as_uint(s);
        const uint32_t mb = sb < cap ? sb : cap; // (used only where s >= cutoff > 0: both are bit patterns of positive floats)
        const u64 key = (static_cast<u64>(mb) << 32) | static_cast<uint32_t>(~static_cast<uint32_t>(j));
        if (maybe && s >= a.cutoff && key > held) { // (NaN is never >= cutoff)
            held = key;
            cut_lo = valu_cutoff_lo(__uint_as_float(mb));
        }
    }
    if (held != found) atomicMax(a.best + i, held);
    if (stamp) stamp_end(a.clk);
}

__global__ __launch_bounds__(256) void mreach_core_kernel(const KnnEntry* __restrict__ lists, const uint32_t* __restrict__ len, u64 n, uint32_t k,
                                                          float cutoff, float* __restrict__ core, u64* __restrict__ dense)
{
    const u64 x = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    float v = 0.0f;
    if (x < n) {
        v = k == 0 ? 1.0f : (len[x] == k ? lists[x * k + (k - 1)].score : 0.0f);
        core[x] = v;
    }
    const u64 d = __ballot(x < n && v >= cutoff);
    if (d && (threadIdx.x & 63u) == 0) atomicAdd(dense, static_cast<u64>(__popcll(d)));
}

} // namespace

hipError_t launch_mreach_fold(const MreachArgs& ma, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t nchunk, hipStream_t s)
{
    const MstArgs& a = ma.mst;
    if (not_ == 0 || c0 >= c1) return hipSuccess;
    if (c1 > a.nrows || a.nown > a.nrows || nchunk < 1 || nchunk > 65535u || !ma.core) return hipErrorInvalidValue;
    const u64 per = ((c1 - c0 + nchunk - 1) / nchunk + 63u) / 64u * 64u;
    const dim3 grid(not_, nchunk), block(kKnnBlock);
    const u64 b0 = c0, b1 = c1;
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL(mreach_fold_kernel<decltype(wp)::value>, grid, block, 0, s, ma, ot0, b0, b1, per);
        return hipGetLastError();
    });
}

hipError_t launch_mreach_core(const KnnEntry* lists, const uint32_t* len, uint64_t nrows, uint32_t k, float cutoff, float* core,
                              unsigned long long* dense, hipStream_t s)
{
    if (nrows == 0) return hipSuccess;
    if (!core || !dense || (k && (!lists || !len))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mreach_core_kernel, dim3(static_cast<uint32_t>((nrows + 255) / 256)), dim3(256), 0, s, lists, len, static_cast<u64>(nrows), k,
                       cutoff, core, reinterpret_cast<u64*>(dense));
    return hipGetLastError();
}

} // namespace gsim
