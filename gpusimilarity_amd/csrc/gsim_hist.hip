// gsim_hist.hip -- similarity histograms and hit counts (gsim_db_histogram, gsim_db_histogram_queries): for every left row the
// number of table rows whose score falls between each pair of edges.  Two kernels, one result; the output is integer, so
// neither the route nor the order in which workgroups add their counts can change it.
//
// The bin of a score: bin(s) = the number of edges e with s >= e, in f32 (NaN and 0.0: bin 0).  hist_bin finds it from a
// coarse table of kHistCoarse cells -- cell t = floor(s x 256), an exact scaling, holds the number of edges <= t / 256, a
// lower bound of bin(s) because t / 256 <= s -- and walks up the true edges from there.  That IS the comparison against
// every edge, started where it cannot fail any more: same counts as a binary search, one LDS read and (with fewer edges than
// cells) one or two compares.
//
// Streaming route (hist_kernel): one pass over the table per left row through the scan's own loops (gsim_scan_inl.h, as
// join_kernel: every width streams the way gsim_db_search's scan does) with HistFilter:
//   * a row's score is score_of(...) of the packed counts, binned;
//   * the wave adds into ITS histogram in LDS.  Score distributions are concentrated -- most of a wave's 64 rows share one or
//     two bins -- so the add is peeled: take the first lane's bin, ballot the lanes that share it, ONE lane adds the ballot's
//     popcount, repeat with the lanes that are left.  (hist_naive_add: one LDS atomic per lane instead, for timing.)
//   * nothing is issued to global memory inside the loop; the wave flushes its non-zero counters once behind it, 64
//     consecutive uint64 counters per atomic instruction.
//
// Owner-tile route (hist_tile_kernel): the scalar-operand scheme of knn_fold_kernel (gsim_knn.hip) with the fold replaced by
// a counter increment.
//   * a workgroup is kHistTile OWNER (left) rows: each of its four waves holds 64 of them, one whole zero-padded fingerprint
//     per lane in VGPRs; the candidate table rows are wave-uniform, read through the scalar path and used as the SGPR operand
//     of v_and_b32; popc(candidate) comes from nbr_prepare_kernel's array, 64 at a time, handed out with v_readlane;
//   * the grid is owner tiles x column chunks: unlike k-NN lists, counts add in any order, so a few hundred owners against a
//     very long table still fill the device;
//   * every lane counts into its own owner's bins in LDS -- the addresses of a wave's 64 lanes are distinct by construction,
//     stride hist_tile_stride() words, odd, so that the lanes of a bank group that hit the same bin hit 32 different banks.
//     A chunk is at most kHistMaxChunk < 2^16 candidates, so no counter of a workgroup can pass 65 535 and two share a word:
//     the add is ds_add_u32 of 1 << 16 (bin & 1) at word bin >> 1.  At 128 edges that is 65 words per owner, 66.5 KB per
//     workgroup, two workgroups per CU;
//   * bin 0 never reaches LDS in the loop: the lane counts it in a register.  A pair that valu_surely_not_kept(
//     valu_cutoff_lo(edges[0]), ...) rejects is in bin 0 by the prefilter's proof (tests/cpp/prefilter_check.cpp, cutoffs in
//     (0, 1]; with edges[0] > 1 the band is off and only c == 0 short-cuts), and a wave whose 64 pairs are all rejected skips
//     the divide;
//   * a workgroup flushes once: every wave adds the non-zero counters of its 64 owners to the uint64 device counters.
//
// Totals: hist_total_kernel sums the rows of the counter matrix per bin.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_held_row.h"
#include "gsim_prefilter.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

// bin(s); edges / coarse in LDS
__device__ __forceinline__ uint32_t hist_bin(float s, const float* edges, const uint8_t* coarse, uint32_t nedges)
{
    // (NaN > 0 is false: cell 0, which holds 0 because edges[0] > 0, and no edge is <= NaN)
    const uint32_t t = s > 0.0f ? static_cast<uint32_t>(fminf(s * static_cast<float>(kHistCoarse), static_cast<float>(kHistCoarse - 1))) : 0u;
    uint32_t b = coarse[t];
    while (b < nedges && s >= edges[b]) b++;
    return b;
}

// the workgroup's copy of the edges and the coarse table (blockDim.x == 256 == kHistCoarse); the caller synchronises
__device__ __forceinline__ void load_bins(const HistBins& bins, float* edges, uint8_t* coarse, uint32_t tid)
{
    if (tid < bins.nedges) edges[tid] = bins.edges[tid];
    coarse[tid] = bins.coarse[tid];
}

// ---- streaming route ---------------------------------------------------------------------------------------------------------

struct HistFilter {
    static constexpr bool kFused = false;
    uint32_t* cnt;         // this wave's nedges + 1 counters in LDS (a launch is fewer than 2^32 rows)
    const float* edges;    // the workgroup's copies in LDS
    const uint8_t* coarse;
    uint32_t nedges;
    uint32_t self;         // the excluded row, counted from the launch's first; 0xFFFFFFFF: none
    int naive;

    __device__ __forceinline__ void checkpoint(uint32_t, int) {}
    __device__ __forceinline__ uint32_t load_gtau() const { return 0u; }
    __device__ __forceinline__ void refresh(uint32_t, int) {}

    // (called by all 64 lanes together: every streaming loop offers under wave-uniform control flow)
    template <int LPR> __device__ __forceinline__ void offer_counts(bool active, uint32_t row, uint32_t val, const ScanArgs& a, int lane)
    {
        const float s = score_of(a.metric, a.alpha, a.beta, a.qpop, val & 0xFFFFu, val >> 16);
        const bool on = active && row != self;
        const uint32_t bin = hist_bin(s, edges, coarse, nedges);
        if (naive) {
            if (on) atomicAdd(&cnt[bin], 1u);
            return;
        }
        u64 m = __ballot(on);
        while (m) { // one trip per distinct bin among the wave's rows
            const uint32_t L = static_cast<uint32_t>(__builtin_ctzll(m));
            const uint32_t bL = readlane_u32(bin, L);
            const u64 same = __ballot(on && bin == bL);
            if (static_cast<uint32_t>(lane) == L) cnt[bL] += static_cast<uint32_t>(__popcll(same)); // (one wave: its LDS operations execute in order)
            m &= ~same;
        }
    }
};

constexpr uint32_t kHistCounters = GSIM_HIST_MAX_EDGES + 1;

// LDS of one workgroup: one object, as JoinShared
template <int NLW> struct HistShared {
    uint32_t words[kScanBlock / 64][NLW ? NLW * 256 : 1];
    uint32_t cnt[kScanBlock / 64][kHistCounters];
    float edges[GSIM_HIST_MAX_EDGES];
    uint8_t coarse[kHistCoarse];
};

// KIND 0: scan_rows<LPR, U>; 1: scan_rows_ragged<LPR, U>; 2: scan_rows_wragged<LPR, U> (LPR = words per row); 3: scan_rows_lane.
template <int KIND, int LPR, int U>
__global__ __launch_bounds__(kScanBlock) void hist_kernel(HistStreamArgs h, ScanGeometry g, u64 r0, u64 nrows, uint32_t l)
{
    constexpr int NLW = KIND == 2 ? (LPR % 2 ? LPR : LPR / 2) * U : 0;
    __shared__ HistShared<NLW> sh;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (tid >> 6));
    const uint32_t nb = h.bins.nedges + 1u;

    load_bins(h.bins, sh.edges, sh.coarse, static_cast<uint32_t>(tid));
    for (uint32_t i = static_cast<uint32_t>(lane); i < nb; i += 64u) sh.cnt[wv][i] = 0u;
    __syncthreads();

    const uint32_t* qrow = h.left + static_cast<u64>(l) * h.W;
    uint32_t qp = 0;
    for (uint32_t i = static_cast<uint32_t>(lane); i < h.W; i += 64u) qp += __popc(qrow[i]);
    ScanArgs a{};
    a.rows = static_cast<const uint32_t*>(h.rows) + r0 * h.W;
    a.nrows = nrows;
    a.W = h.W;
    a.query = qrow;
    a.qpop = wave_sum(qp);
    a.metric = h.metric;
    a.alpha = h.alpha;
    a.beta = h.beta;

    HistFilter f;
    f.cnt = sh.cnt[wv];
    f.edges = sh.edges;
    f.coarse = sh.coarse;
    f.nedges = h.bins.nedges;
    const u64 self = h.self0 + l; // (left row l is table row self0 + l)
    f.self = h.self0 != ~0ull && self >= r0 && self - r0 < nrows ? static_cast<uint32_t>(self - r0) : 0xFFFFFFFFu;
    f.naive = h.naive;
    if constexpr (KIND == 0) {
        const u32x4 q = reinterpret_cast<const u32x4*>(qrow)[lane % LPR];
        scan_rows<LPR, U>(a, g, f, q, w, lane);
    } else if constexpr (KIND == 1) {
        scan_rows_ragged<LPR, U>(a, g, f, w, lane);
    } else if constexpr (KIND == 2) {
        scan_rows_wragged<LPR, U>(a, g, f, w, lane, sh.words[wv]);
    } else {
        scan_rows_lane(a, g, f, w, lane);
    }
    // the wave's counters -> the left row's device counters
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    u64* out = h.hist + static_cast<u64>(l) * nb;
    for (uint32_t i = static_cast<uint32_t>(lane); i < nb; i += 64u) {
        const uint32_t v = sh.cnt[wv][i];
        if (v) atomicAdd(&out[i], static_cast<u64>(v));
    }
}

template <int KIND, int LPR, int U>
hipError_t launch_t(const HistStreamArgs& h, const ScanGeometry& g, u64 r0, u64 nrows, uint32_t l, hipStream_t s)
{
    hipLaunchKernelGGL((hist_kernel<KIND, LPR, U>), dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, h, g, r0, nrows, l);
    return hipGetLastError();
}

// ---- owner-tile route --------------------------------------------------------------------------------------------------------

constexpr uint32_t kHistLdsHead = GSIM_HIST_MAX_EDGES + kHistCoarse / 4; // words in front of the counters: edges, coarse table

template <int WP>
__global__ __launch_bounds__(kHistBlock) void hist_tile_kernel(HistTileArgs a, uint32_t ot0, u64 c0, u64 c1, uint32_t chunk)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t hist_lds[];
    float* edges = reinterpret_cast<float*>(hist_lds);
    uint8_t* coarse = reinterpret_cast<uint8_t*>(hist_lds + GSIM_HIST_MAX_EDGES);
    uint32_t* cnt = hist_lds + kHistLdsHead;
    const uint32_t nedges = a.bins.nedges;
    const uint32_t nb = nedges + 1u;
    const uint32_t stride = ((nedges + 2u) / 2u) | 1u; // == hist_tile_stride(nedges)

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
    load_bins(a.bins, edges, coarse, threadIdx.x);
    for (uint32_t i = threadIdx.x; i < kHistTile * stride; i += kHistBlock) cnt[i] = 0u;
    __syncthreads();

    // the wave's 64 owners: left rows o0 .. o0 + 63
    const u64 o0 = (static_cast<u64>(ot0) + blockIdx.x) * kHistTile + wib * 64u;
    if (o0 >= a.nl) return; // (wave-uniform; no barrier behind this point)
    const bool stamp = a.clk && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
    if (stamp) stamp_begin(a.clk);
    const u64 o = o0 + lane;
    const bool oin = o < a.nl; // a lane past the last owner is idle, but takes part in the ballots
    const u64 self = a.self0 != ~0ull && oin ? a.self0 + o : ~0ull;

    // this lane's owner row, whole, in VGPRs (zero words beyond the row: nothing to count there)
    u32x4 r4[WP / 4];
    const u32x4* rp = reinterpret_cast<const u32x4*>(a.lrows) + (oin ? o : 0) * (WP / 4);
#pragma unroll
    for (int w = 0; w < WP / 4; w++) r4[w] = oin ? rp[w] : u32x4{0, 0, 0, 0};
    uint32_t av = 0;
#pragma unroll
    for (int w = 0; w < WP / 4; w++) av += __popc(r4[w].x) + __popc(r4[w].y) + __popc(r4[w].z) + __popc(r4[w].w);

    uint32_t* mine = cnt + (wib * 64u + lane) * stride; // this owner's counters
    const float cut_lo = a.bins.cut_lo;
    uint32_t n0 = 0; // pairs in bin 0

    const u64 j0 = c0 + static_cast<u64>(blockIdx.y) * chunk;
    const u64 j1 = j0 + chunk < c1 ? j0 + chunk : c1; // (at most kHistMaxChunk candidates: no 16-bit counter can wrap)
    const const_u32x4p crows = (const_u32x4p) (a.rows);
    uint32_t vpop = 0;
    for (u64 j = j0; j < j1; j++) {
        const uint32_t t = static_cast<uint32_t>(j - j0);
        if ((t & 63u) == 0) { // popc of the next 64 candidates, one per lane (read back with v_readlane)
            const u64 jl = j + lane;
            vpop = jl < j1 ? a.pop[jl] : 0u;
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
        const bool counted = oin && j != self;
        const bool above = counted && !valu_surely_not_kept(cut_lo, cf, den, c); // false: bin 0 without the divide
        n0 += counted && !above;
        if (__ballot(above) == 0) continue;
        const float s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, av, b, c)
        const uint32_t bin = hist_bin(s, edges, coarse, nedges);
        n0 += above && bin == 0u;
        if (above && bin != 0u) atomicAdd(&mine[bin >> 1], 1u << ((bin & 1u) * 16u));
    }
    if (n0) atomicAdd(&mine[0], n0); // (n0 <= chunk < 2^16, and nothing else has touched bin 0's half)

    // the wave's 64 owners x nb counters -> the device counters, 64 consecutive ones per instruction
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier(); // (one wave: its LDS operations execute in order)
    const uint32_t* wcnt = cnt + wib * 64u * stride;
    const u64 nown = a.nl - o0 < 64u ? a.nl - o0 : 64u;
    u64* out = a.hist + o0 * nb;
    for (uint32_t i = lane; i < static_cast<uint32_t>(nown) * nb; i += 64u) {
        const uint32_t ow = i / nb, bin = i - ow * nb;
        const uint32_t v = (wcnt[ow * stride + (bin >> 1)] >> ((bin & 1u) * 16u)) & 0xFFFFu;
        if (v) atomicAdd(&out[i], static_cast<u64>(v));
    }
    if (stamp) stamp_end(a.clk);
}

template <int WP>
hipError_t launch_tiles_t(const HistTileArgs& a, uint32_t ot0, uint32_t not_, u64 c0, u64 c1, uint32_t chunk, hipStream_t s)
{
    const size_t lds = hist_tile_lds_bytes(GSIM_HIST_MAX_EDGES);
    static DynLdsOnce once;
    const hipError_t e = once.ensure(reinterpret_cast<const void*>(hist_tile_kernel<WP>), lds);
    if (e != hipSuccess) return e;
    const u64 nchunks = (c1 - c0 + chunk - 1) / chunk;
    if (nchunks > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hist_tile_kernel<WP>, dim3(not_, static_cast<uint32_t>(nchunks)), dim3(kHistBlock), hist_tile_lds_bytes(a.bins.nedges), s, a,
                       ot0, c0, c1, chunk);
    return hipGetLastError();
}

// ---- totals ------------------------------------------------------------------------------------------------------------------

// total[b] += the counters e of the flattened matrix with e % nb == b; every workgroup sums in LDS first
__global__ __launch_bounds__(256) void hist_total_kernel(const u64* __restrict__ hist, u64 n, uint32_t nb, u64* __restrict__ total)
{
    __shared__ u64 acc[kHistCounters];
    for (uint32_t i = threadIdx.x; i < nb; i += 256u) acc[i] = 0;
    __syncthreads();
    const u64 step = static_cast<u64>(gridDim.x) * 256u;
    const uint32_t bstep = static_cast<uint32_t>(step % nb);
    u64 e = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    uint32_t b = static_cast<uint32_t>(e % nb);
    for (; e < n; e += step) {
        const u64 v = hist[e];
        if (v) atomicAdd(&acc[b], v);
        b += bstep;
        b = b >= nb ? b - nb : b;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += 256u)
        if (acc[i]) atomicAdd(&total[i], acc[i]);
}

} // namespace

uint32_t hist_tile_stride(uint32_t nedges)
{
    return ((nedges + 2u) / 2u) | 1u;
}

size_t hist_tile_lds_bytes(uint32_t nedges)
{
    return (static_cast<size_t>(kHistLdsHead) + static_cast<size_t>(kHistTile) * hist_tile_stride(nedges)) * 4u;
}

hipError_t launch_hist_tiles(const HistTileArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t chunk, hipStream_t s)
{
    if (not_ == 0 || c0 >= c1) return hipSuccess;
    if (a.bins.nedges < 1 || a.bins.nedges > GSIM_HIST_MAX_EDGES || c1 > a.nrows || chunk == 0 || chunk > kHistMaxChunk || chunk % kHistColTile ||
        (static_cast<u64>(ot0) + not_ - 1) * kHistTile >= a.nl)
        return hipErrorInvalidValue;
    // (launch_tiles_t<WP> keeps its own DynLdsOnce: the dynamic-LDS attribute is set once per instantiation)
    return dispatch_wp(a.WP, [&](auto wp) { return launch_tiles_t<decltype(wp)::value>(a, ot0, not_, c0, c1, chunk, s); });
}

hipError_t launch_hist_pass(const HistStreamArgs& m, const ScanGeometry& g, uint64_t r0, uint64_t nrows, uint32_t p, hipStream_t s)
{
    if (m.bins.nedges < 1 || m.bins.nedges > GSIM_HIST_MAX_EDGES) return hipErrorInvalidValue;
#define GSIM_CASE(L) \
    if (g.lanes_per_row == L && g.unroll == 8) return launch_t<0, L, 8>(m, g, r0, nrows, p, s);
    GSIM_CASE(1)
    GSIM_CASE(2)
    GSIM_CASE(4)
    GSIM_CASE(8)
    GSIM_CASE(16)
    GSIM_CASE(32)
    GSIM_CASE(64)
#undef GSIM_CASE
    if (g.lanes_per_row != 0) return hipErrorInvalidValue;
    if (g.ragged_words) {
        switch (m.W) {
        case 3: return launch_t<2, 3, 3>(m, g, r0, nrows, p, s);
        case 5: return launch_t<2, 5, 2>(m, g, r0, nrows, p, s);
        case 7: return launch_t<2, 7, 1>(m, g, r0, nrows, p, s);
        case 6: return launch_t<2, 6, 3>(m, g, r0, nrows, p, s);
        case 10: return launch_t<2, 10, 2>(m, g, r0, nrows, p, s);
        case 14: return launch_t<2, 14, 1>(m, g, r0, nrows, p, s);
        case 9: return launch_t<2, 9, 1>(m, g, r0, nrows, p, s);
        case 18: return launch_t<2, 18, 1>(m, g, r0, nrows, p, s);
        case 11: return launch_t<2, 11, 1>(m, g, r0, nrows, p, s);
        case 22: return launch_t<2, 22, 1>(m, g, r0, nrows, p, s);
        default: return hipErrorInvalidValue;
        }
    }
    switch (g.ragged_loads) {
    case 0: return launch_t<3, 0, 1>(m, g, r0, nrows, p, s);
    case 3: return launch_t<1, 3, 3>(m, g, r0, nrows, p, s);
    case 5: return launch_t<1, 5, 2>(m, g, r0, nrows, p, s);
    case 7: return launch_t<1, 7, 1>(m, g, r0, nrows, p, s);
    case 9: return launch_t<1, 9, 1>(m, g, r0, nrows, p, s);
    case 11: return launch_t<1, 11, 1>(m, g, r0, nrows, p, s);
    case 13: return launch_t<1, 13, 1>(m, g, r0, nrows, p, s);
    case 15: return launch_t<1, 15, 1>(m, g, r0, nrows, p, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_hist_total(const unsigned long long* hist, uint64_t nl, uint32_t nbins, unsigned long long* total, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(total, 0, static_cast<size_t>(nbins) * 8, s);
    if (e != hipSuccess || nl == 0) return e;
    const u64 n = nl * nbins;
    const u64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(hist_total_kernel, dim3(static_cast<uint32_t>(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, hist, n, nbins, total);
    return hipGetLastError();
}

} // namespace gsim
