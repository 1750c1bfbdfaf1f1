// gsim_label_sums.hip -- quantised score sums grouped by label (gsim_db_label_sums): for every labelled row the sum of its scores
// against its own cluster and the other cluster of the greatest mean -- what silhouettes and exact medoids are made of.  The rule is
// stated in include/gpusim_hip.h; DESIGN.md section 29 has the kernel's metadata, the launch cutting and the measurements.
//
// The host hands over the labelled rows in LABEL ORDER: a zero-padded copy sorted by (label, row), their popcounts, the label of
// every sorted position and the nlabels + 1 segment starts.  Owners and candidates are positions of that copy.
//
// Fold kernel (lsum_fold_kernel): the scalar-operand VALU scheme of knn_fold_kernel (gsim_knn.hip) with the list replaced by a sum.
//   * a workgroup is kLsumTile OWNERS in sorted order: each of its four waves holds 64 of them, one whole row per lane in VGPRs
//     (HeldRow), and walks the wave-uniform candidates j in ascending order: the candidate's words come through the scalar path and
//     are the SGPR operand of v_and_b32, popc(candidate) comes from the side array, 64 at a time (Handout64);
//   * EVERY pair takes the reference's divide -- nothing is dropped, so there is no band in front of it -- and becomes
//     q = (uint32) floor(s * 2^31): an exact scaling, a truncating conversion.  c == 0 gives 0 (0 / 0 included), the owner's own
//     position adds 0.  A lane adds q to its 64-bit running sum: integers, so no order of addition can change a sum;
//   * candidates arrive in ascending label order, so the walk is a scalar loop over SEGMENTS around the candidate loop: the label
//     and the end of the current segment are wave-uniform, the inner loop carries no label test.  Where a segment truly ends, every
//     lane folds its running sum: into own_q if the label is its own, otherwise into its best-so-far when the mean is STRICTLY
//     greater -- run * best_n > best_q * n, compared as exact 96-bit products -- or when it is the first other label.  Ascending
//     labels make that the lowest-label tie rule;
//   * {run_q, own_q, best_q, best_label} per owner (LsumState, 32 bytes) lives in global memory and carries from launch to launch: a
//     launch's candidate range may end in the middle of a segment, the fold happens only at the segment's end.  As in gsim_db_knn,
//     stream order is the only dependency: nothing waits grid-wide, columns are not split over workgroups, so a short range against
//     nothing else has little parallelism;
//   * OWN_ONLY: a wave's 64 owners span a contiguous run of labels l_lo .. l_hi, so the wave walks [first[l_lo], first[l_hi + 1])
//     only (cut to the launch's range), and a lane keeps only the segment of its own label: sum of n_l^2 pairs instead of n^2.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_held_row.h"

namespace gsim
{
namespace
{

// out[p] = the table row list[p], zero-padded to WP words
__global__ __launch_bounds__(256) void lsum_gather_kernel(const uint32_t* __restrict__ rows, uint32_t W, uint32_t WP, const uint32_t* __restrict__ list, u64 n,
                                                          uint32_t* __restrict__ out)
{
    const u64 total = n * WP;
    for (u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x; t < total; t += static_cast<u64>(gridDim.x) * 256u) {
        const u64 p = t / WP;
        const uint32_t w = static_cast<uint32_t>(t - p * WP);
        out[t] = w < W ? rows[static_cast<u64>(list[p]) * W + w] : 0u;
    }
}

__global__ __launch_bounds__(256) void lsum_init_kernel(LsumState* state, u64 n)
{
    const u64 p = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (p < n) state[p] = LsumState{0, 0, 0, GSIM_LABEL_NONE, 0};
}

template <int WP, bool OWN_ONLY> __global__ __launch_bounds__(kLsumBlock) void lsum_fold_kernel(LsumArgs a, uint32_t ot0, u64 c0, u64 c1)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    // the wave's 64 owners: sorted positions o0 .. o0 + 63
    const u64 o0 = (static_cast<u64>(ot0) + blockIdx.x) * kLsumTile + wib * 64u;
    if (o0 >= a.n) return; // (wave-uniform; the kernel has no barrier)
    u64 j0 = c0, j1 = c1;
    if constexpr (OWN_ONLY) { // the segments of the wave's own labels, cut to the launch
        const u64 olast = o0 + 63u < a.n ? o0 + 63u : a.n - 1u;
        const u64 lo = a.first[a.keys[o0]], hi = a.first[a.keys[olast] + 1u];
        j0 = lo > c0 ? lo : c0;
        j1 = hi < c1 ? hi : c1;
        if (j0 >= j1) return;
    }
    const bool stamp = a.clk && blockIdx.x == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 o = o0 + lane;
    const bool oin = o < a.n; // a lane past the last owner holds a zero row: every q it sees is 0, and it stores nothing
    const u64 oc = oin ? o : a.n - 1u;
    const uint32_t self = oin ? static_cast<uint32_t>(o) : 0xFFFFFFFFu; // (n < 2^32)
    const uint32_t mine = a.keys[oc];

    HeldRow<WP> held;
    const uint32_t av = held.load(a.rows, oc, oin);

    LsumState st = a.state[oc];
    u64 run = st.run_q, own = st.own_q, best = st.best_q;
    uint32_t best_label = st.best_label;
    uint32_t best_n = 1u; // rows of best_label
    if constexpr (!OWN_ONLY) {
        if (best_label != GSIM_LABEL_NONE) best_n = a.first[best_label + 1u] - a.first[best_label];
    }

    const const_u32x4p crows = (const_u32x4p) (a.rows);
    Handout64 pops;
    u64 j = j0;
    while (j < j1) { // one trip per segment
        const uint32_t l = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a.keys[j]))); // (wave-uniform, as j)
        const u64 send = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a.first[l + 1u])));
        const u64 e = send < j1 ? send : j1;
        for (; j < e; j++) {
            const uint32_t t = static_cast<uint32_t>(j - j0);
            if (Handout64::due(t)) pops.fetch(a.pop, j, lane, j1);
            const uint32_t b = pops.get(t);
            const uint32_t c = held.common(crows + j * (WP / 4));
            // the owner is the query: a = popc(owner), b = popc(candidate)
            const float den = score_den(a.metric, a.alpha, a.beta, av, b, c);
            const float s = __fdiv_rn(static_cast<float>(c), den); // == score_of(metric, alpha, beta, av, b, c) where c > 0
            const uint32_t q = __float2uint_rz(s * 2147483648.0f);
            run += c != 0u && static_cast<uint32_t>(j) != self ? q : 0u;
        }
        if (e == send) { // the segment ends here: fold
            if (l == mine) {
                own = run;
            } else if constexpr (!OWN_ONLY) {
                const uint32_t nl = static_cast<uint32_t>(send - a.first[l]);
                const bool greater = static_cast<unsigned __int128>(run) * best_n > static_cast<unsigned __int128>(best) * nl;
                if (best_label == GSIM_LABEL_NONE || greater) {
                    best = run;
                    best_label = l;
                    best_n = nl;
                }
            }
            run = 0;
        }
    }
    if (oin) a.state[o] = LsumState{run, own, best, best_label, 0};
    if (stamp) stamp_end(a.clk);
}

__global__ __launch_bounds__(256) void lsum_scatter_kernel(const LsumState* __restrict__ state, const uint32_t* __restrict__ list, u64 n, uint32_t row0,
                                                           u64* __restrict__ own_q, uint32_t* __restrict__ other_label, u64* __restrict__ other_q)
{
    const u64 p = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (p >= n) return;
    const LsumState st = state[p];
    const uint32_t i = list[p] - row0;
    own_q[i] = st.own_q;
    if (other_label) {
        other_label[i] = st.best_label;
        other_q[i] = st.best_q;
    }
}

template <bool OWN_ONLY> hipError_t launch_fold_t(const LsumArgs& a, uint32_t ot0, uint32_t not_, u64 c0, u64 c1, hipStream_t s)
{
    const dim3 grid(not_), block(kLsumBlock);
    return dispatch_wp(a.WP, [&](auto wp) {
        hipLaunchKernelGGL((lsum_fold_kernel<decltype(wp)::value, OWN_ONLY>), grid, block, 0, s, a, ot0, c0, c1);
        return hipGetLastError();
    });
}

} // namespace

hipError_t launch_lsum_gather(const uint32_t* rows, uint32_t W, uint32_t WP, const uint32_t* list, uint64_t n, uint32_t* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (W == 0 || W > WP || !rows || !list || !out) return hipErrorInvalidValue;
    const u64 blocks = (n * WP + 255) / 256;
    hipLaunchKernelGGL(lsum_gather_kernel, dim3(static_cast<uint32_t>(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, rows, W, WP, list,
                       static_cast<u64>(n), out);
    return hipGetLastError();
}

hipError_t launch_lsum_init(LsumState* state, uint64_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lsum_init_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, state, static_cast<u64>(n));
    return hipGetLastError();
}

hipError_t launch_lsum_fold(const LsumArgs& a, bool own_only, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, hipStream_t s)
{
    if (not_ == 0 || c0 >= c1) return hipSuccess;
    if (c1 > a.n || a.n > 0xFFFFFFFFull || (static_cast<u64>(ot0) + not_ - 1) * kLsumTile >= a.n || !a.rows || !a.pop || !a.keys || !a.first || !a.state)
        return hipErrorInvalidValue;
    return own_only ? launch_fold_t<true>(a, ot0, not_, c0, c1, s) : launch_fold_t<false>(a, ot0, not_, c0, c1, s);
}

hipError_t launch_lsum_scatter(const LsumState* state, const uint32_t* list, uint64_t n, uint32_t row0, unsigned long long* own_q, uint32_t* other_label,
                               unsigned long long* other_q, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFFull || !own_q || (other_label != nullptr) != (other_q != nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lsum_scatter_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, state, list, static_cast<u64>(n), row0, own_q,
                       other_label, other_q);
    return hipGetLastError();
}

} // namespace gsim
