// gsim_group.hip -- group queries (gsim_db_search_group): exact top-k of the table by the MAX, MIN or MEAN of a row's scores
// against a SET of M queries, in one pass over the table.  The rule is stated in include/gpusim_hip.h.
//
// The layout is the multi-query scan's (gsim_batch.hip): every lane holds RPL whole rows in registers, the row's popcount is
// taken once, and the M queries are wave-uniform -- read through a constant-address-space pointer, so their words arrive by
// scalar loads and are the SGPR operand of v_and_b32 (2 VALU instructions per word pair).  Per query: the inner product, the
// score with the scan's own arithmetic (score_of; NaN -> 0), and the mode's reduction in registers:
//   MAX / MIN   a strict compare, so `which` is the lowest query that attains the extreme;
//   MEAN        acc = fadd_rn(acc, s) in query order 0 ... M-1, then fdiv_rn(acc, (float) M) -- the order is part of the rule.
// After the last query a row is ONE f32 in [0, 1]: it is offered once to the four-kernel pipeline's streaming filter
// (WaveFilter::offer, gsim_filter_inl.h) with cb = which << 16 | popc(row), and the kernel ends as the row-set scans do
// (finish + block_filter_flush) -- compact_kernel and the select kernels follow unchanged.
// Seeding: none (gtau starts at 0): sample_kernel's seed is a bound for single-query scores only.
//
// Launch cutting: M inner products per row make a pass over a large table long, so a pass is cut into launches over
// consecutive chunk ranges (GSIM_GROUP_LAUNCH_PAIRS row x query pairs each).  Chunk c belongs to wave c % nwaves in every
// launch, so a wave's candidate segment continues where its predecessor stopped: it starts at seg_count[w] and adds only its
// own increment to QueryState::ncand / kept; ghist and gtau live in QueryState and carry over by themselves.
//
// `which` behind the tail: the select kernel's usual path writes the hit's cb verbatim; its heavy-tie path and the large-k
// sort rebuild {common, popc_db} from ScanArgs::query_dev instead, which for a group is not `which`.  Those blocks carry
// header flag 1, and group_which_kernel recomputes the field for them from the M queries (the same arithmetic, so the same
// extreme and the same lowest index).
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_filter_inl.h"
#include "gsim_row_units.h"

namespace gsim
{
namespace
{

typedef const __attribute__((address_space(4))) uint32_t* ConstWords; // constant address space: wave-uniform reads are scalar loads
typedef int s8 __attribute__((ext_vector_type(8)));                   // an 8-dword SGPR tuple

// NaN (0 / 0) counts as 0.0: what gsim_db_search returns at cutoff 0 (apply_cutoff: a NaN compares false)
__device__ __forceinline__ float pair_score(int metric, float alpha, float beta, uint32_t qa, uint32_t bb, uint32_t cc)
{
    return apply_cutoff(score_of(metric, alpha, beta, qa, bb, cc), 0.0f);
}

// The mode's reduction over the queries, one instance per row held by the lane.
template <int MODE> struct GroupAcc {
    float g;
    uint32_t which;
    __device__ __forceinline__ void init()
    {
        g = MODE == GSIM_GROUP_MAX ? -1.0f : (MODE == GSIM_GROUP_MIN ? 2.0f : 0.0f); // (every pair score lies in [0, 1])
        which = 0;
    }
    __device__ __forceinline__ void add(float s, uint32_t q)
    {
        if constexpr (MODE == GSIM_GROUP_MEAN) {
            g = __fadd_rn(g, s);
        } else {
            const bool better = MODE == GSIM_GROUP_MAX ? s > g : s < g; // strict: the lowest query that attains it stays
            g = better ? s : g;
            which = better ? q : which;
        }
    }
    __device__ __forceinline__ float result(uint32_t nq) const { return MODE == GSIM_GROUP_MEAN ? __fdiv_rn(g, static_cast<float>(nq)) : g; }
};

// the first chunk of wave w at or after c0 (chunk c belongs to wave c % nwaves in every launch of the pass)
__device__ __forceinline__ u64 first_chunk(u64 c0, uint32_t w, uint32_t nwaves)
{
    const uint32_t r = static_cast<uint32_t>(c0 % nwaves);
    return c0 + (w >= r ? w - r : w + nwaves - r);
}

// WORDS != 0: rows of WORDS words (a multiple of 4) held in registers, RPL rows per lane, MANUAL: the query words in 8-word blocks
// double-buffered by hand (WORDS % 16 == 0; two 8-dword tuples -- with batch_scan_kernel's 16-dword ones the filter's wave-uniform
// state no longer fits the scalar registers and the compiler spills some).  WORDS == 0: any width, one row per lane, word by word (the row is read again
// for every query -- from the cache; correct, not fast).
template <int WORDS, int RPL, int MODE, bool MANUAL>
__global__ __launch_bounds__(kScanBlock) void group_scan_kernel(ScanArgs a, ScanGeometry g, GroupArgs ga)
{
    __shared__ BlockFilter s_filter;
    const int lane = threadIdx.x & 63;
    const uint32_t wib = threadIdx.x >> 6;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (threadIdx.x >> 6));
    block_filter_init(&s_filter, a.k, a.state->gtau);
    // this wave's segment continues behind what the pass's earlier launches left
    const uint32_t start = ga.first ? 0u : static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a.seg_count[w])));
    WaveFilter f;
    f.init(&s_filter, a.state, a.cand + static_cast<u64>(w) * g.seg_cap + start, a.cand_cb + static_cast<u64>(w) * g.seg_cap + start, a.k, a.cutoff);
    const uint32_t nq = ga.nq;
    const ConstWords qbase = (ConstWords) ga.queries;
    uint32_t gt = 0, trip = 0;

    if constexpr (WORDS != 0) {
        static_assert(!MANUAL || WORDS % 16 == 0, "the hand-scheduled loads alternate two 8-word buffers");
        constexpr int CHR = 64 * RPL;
        constexpr int NB = WORDS / 8;
        const u32x4* __restrict__ db = reinterpret_cast<const u32x4*>(a.rows);
        for (u64 c = first_chunk(ga.c0, w, g.nwaves); c < ga.c1; c += g.nwaves) {
            u32x4 r4[RPL][WORDS / 4];
            uint32_t bb[RPL];
            bool active[RPL];
            u64 rowi[RPL];
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                rowi[r] = c * CHR + r * 64 + lane;
                active[r] = rowi[r] < a.nrows;
                const u32x4* p = db + rowi[r] * (WORDS / 4);
#pragma unroll
                for (int j = 0; j < WORDS / 4; j++) r4[r][j] = active[r] ? p[j] : u32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                bb[r] = 0;
#pragma unroll
                for (int j = 0; j < WORDS / 4; j++) bb[r] += __popc(r4[r][j].x) + __popc(r4[r][j].y) + __popc(r4[r][j].z) + __popc(r4[r][j].w);
            }
            poll_threshold(f, gt, trip, wib, lane);

            GroupAcc<MODE> acc[RPL];
#pragma unroll
            for (int r = 0; r < RPL; r++) acc[r].init();
            s8 qA, qB;
            if constexpr (MANUAL) asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=s"(qA) : "s"(qbase));
            for (uint32_t q0 = 0; q0 < nq; q0 += 64) {
                // the popcounts of 64 queries in a VGPR (lane i: query q0 + i), read with v_readlane: a vector load, so that
                // nothing but the query words counts on lgkmcnt inside the loop
                const uint32_t vqpop = q0 + lane < nq ? ga.qpop[q0 + lane] : 0u;
                const uint32_t qn = nq - q0 < 64u ? nq - q0 : 64u;
                for (uint32_t qq = 0; qq < qn; qq++) {
                    const uint32_t q = q0 + qq;
                    const ConstWords qw = qbase + static_cast<size_t>(q) * WORDS;
                    uint32_t cnt[RPL][4];
#pragma unroll
                    for (int r = 0; r < RPL; r++) cnt[r][0] = cnt[r][1] = cnt[r][2] = cnt[r][3] = 0;
                    if constexpr (MANUAL) {
                        // as batch_scan_kernel: the next block (or the next query's first) is in flight while this one is
                        // reduced; scalar loads return out of order, hence lgkmcnt(0) before a buffer is used.
                        // The compiler does not know that qA / qB are in flight between the load and the wait (qA also from one
                        // query, and one chunk, to the next): this is right only while it neither copies nor spills the two tuples
                        // there.  After ANY change to this loop, or to what is live across it, read the ISA again: both tuples in
                        // fixed SGPR ranges, no s_mov of them before the wait, SGPR spills 0 (DESIGN.md section 13 has the figures).
#pragma unroll
                        for (int blk = 0; blk < NB; blk++) {
                            s8& cur = (blk & 1) ? qB : qA; // NB is even: block 0 of every query is qA
                            s8& nxt = (blk & 1) ? qA : qB;
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            __builtin_amdgcn_sched_barrier(0);
                            if (blk + 1 < NB) {
                                asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(nxt) : "s"(qw), "n"((blk + 1) * 32));
                            } else if (q + 1 < nq) {
                                asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(nxt) : "s"(qw), "n"(WORDS * 4));
                            }
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int j = 0; j < 2; j++) {
#pragma unroll
                                for (int r = 0; r < RPL; r++) {
                                    const u32x4 x = r4[r][blk * 2 + j];
                                    cnt[r][0] = bcnt_acc(x.x & static_cast<uint32_t>(cur[4 * j + 0]), cnt[r][0]);
                                    cnt[r][1] = bcnt_acc(x.y & static_cast<uint32_t>(cur[4 * j + 1]), cnt[r][1]);
                                    cnt[r][2] = bcnt_acc(x.z & static_cast<uint32_t>(cur[4 * j + 2]), cnt[r][2]);
                                    cnt[r][3] = bcnt_acc(x.w & static_cast<uint32_t>(cur[4 * j + 3]), cnt[r][3]);
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < WORDS / 4; j++) {
                            const uint32_t q0w = qw[4 * j + 0], q1w = qw[4 * j + 1], q2w = qw[4 * j + 2], q3w = qw[4 * j + 3];
#pragma unroll
                            for (int r = 0; r < RPL; r++) {
                                cnt[r][0] = bcnt_acc(r4[r][j].x & q0w, cnt[r][0]);
                                cnt[r][1] = bcnt_acc(r4[r][j].y & q1w, cnt[r][1]);
                                cnt[r][2] = bcnt_acc(r4[r][j].z & q2w, cnt[r][2]);
                                cnt[r][3] = bcnt_acc(r4[r][j].w & q3w, cnt[r][3]);
                            }
                        }
                    }
                    const uint32_t qa = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(vqpop), static_cast<int>(qq)));
#pragma unroll
                    for (int r = 0; r < RPL; r++) {
                        const uint32_t cc = (cnt[r][0] + cnt[r][1]) + (cnt[r][2] + cnt[r][3]);
                        acc[r].add(pair_score(a.metric, a.alpha, a.beta, qa, bb[r], cc), q);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RPL; r++)
                f.offer(active[r], static_cast<uint32_t>(rowi[r]), acc[r].result(nq), (acc[r].which << 16) + bb[r], lane);
        }
    } else {
        const uint32_t* __restrict__ db = static_cast<const uint32_t*>(a.rows);
        const uint32_t W = a.W;
        for (u64 c = first_chunk(ga.c0, w, g.nwaves); c < ga.c1; c += g.nwaves) {
            const u64 rowi = c * 64u + static_cast<uint32_t>(lane);
            const bool active = rowi < a.nrows;
            const uint32_t* r = db + (active ? rowi : 0) * W;
            uint32_t bb = 0;
            if (active)
                for (uint32_t i = 0; i < W; i++) bb += __popc(r[i]);
            poll_threshold(f, gt, trip, wib, lane);
            GroupAcc<MODE> acc;
            acc.init();
            for (uint32_t q = 0; q < nq; q++) {
                const ConstWords qw = qbase + static_cast<size_t>(q) * W;
                uint32_t cc = 0;
                if (active)
                    for (uint32_t i = 0; i < W; i++) cc += __popc(r[i] & qw[i]);
                acc.add(pair_score(a.metric, a.alpha, a.beta, ga.qpop[q], bb, cc), q);
            }
            f.offer(active, static_cast<uint32_t>(rowi), acc.result(nq), (acc.which << 16) + bb, lane);
        }
    }
    f.finish(w, a, lane); // (seg_count[w] = this launch's candidates, ncand / kept += this launch's)
    if (lane == 0 && start) a.seg_count[w] = start + f.cursor; // ... the segment's cursor counts the earlier launches' too
    block_filter_flush(&s_filter, a);
}

// Hits [h0, h1) of a result block whose header carries flag 1 (the tail rebuilt the hits' 16-bit fields from the rows): `which`
// again, from the M queries.  One hit per thread.
__global__ __launch_bounds__(256) void group_which_kernel(ScanArgs a, GroupArgs ga, uint32_t row_base, void* block, uint32_t h0, uint32_t h1)
{
    const gsim_result_header* hdr = static_cast<const gsim_result_header*>(block);
    if ((hdr->flags & 1u) == 0) return;
    const uint32_t n = hdr->count < h1 ? hdr->count : h1;
    const uint32_t i = h0 + blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    gsim_group_hit* hit = reinterpret_cast<gsim_group_hit*>(const_cast<gsim_result_header*>(hdr) + 1) + i;
    uint32_t which = 0;
    if (ga.mode != GSIM_GROUP_MEAN) {
        const uint32_t* r = static_cast<const uint32_t*>(a.rows) + static_cast<u64>(hit->row - row_base) * a.W;
        const uint32_t bb = hit->popc_db;
        const bool is_max = ga.mode == GSIM_GROUP_MAX;
        float best = is_max ? -1.0f : 2.0f;
        for (uint32_t q = 0; q < ga.nq; q++) {
            const uint32_t* qw = ga.queries + static_cast<size_t>(q) * a.W;
            uint32_t cc = 0;
            for (uint32_t j = 0; j < a.W; j++) cc += __popc(r[j] & qw[j]);
            const float s = pair_score(a.metric, a.alpha, a.beta, ga.qpop[q], bb, cc);
            const bool better = is_max ? s > best : s < best;
            best = better ? s : best;
            which = better ? q : which;
        }
    }
    hit->which = static_cast<uint16_t>(which);
}

template <int WORDS, int RPL, bool MANUAL> hipError_t launch_group_t(const ScanArgs& a, const ScanGeometry& g, const GroupArgs& ga, hipStream_t s)
{
    const dim3 grid(g.nwaves / (kScanBlock / 64)), block(kScanBlock);
    switch (ga.mode) {
    case GSIM_GROUP_MAX: hipLaunchKernelGGL((group_scan_kernel<WORDS, RPL, GSIM_GROUP_MAX, MANUAL>), grid, block, 0, s, a, g, ga); break;
    case GSIM_GROUP_MIN: hipLaunchKernelGGL((group_scan_kernel<WORDS, RPL, GSIM_GROUP_MIN, MANUAL>), grid, block, 0, s, a, g, ga); break;
    case GSIM_GROUP_MEAN: hipLaunchKernelGGL((group_scan_kernel<WORDS, RPL, GSIM_GROUP_MEAN, MANUAL>), grid, block, 0, s, a, g, ga); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// rows per lane of the specialised widths (launch_batch_scan's), 1 for the word loop
uint32_t group_rpl(uint32_t W)
{
    return W == 4 || W == 8 || W == 16 ? 4u : (W == 32 ? 2u : 1u);
}

} // namespace

ScanGeometry group_geometry(uint64_t nrows, uint32_t W, int num_cus)
{
    ScanGeometry g{};
    g.unroll = 1;
    g.chunk_rows = 64u * group_rpl(W);
    g.nchunks = (nrows + g.chunk_rows - 1) / g.chunk_rows;
    // twelve waves per CU (three per SIMD, the multi-query scan's): the loop is VALU-bound, and the other waves of a SIMD fill the
    // issue slots one of them leaves while it waits for query words or offers its rows
    uint64_t nw = static_cast<uint64_t>(num_cus) * 12u;
    if (nw > g.nchunks) nw = g.nchunks;
    if (nw < 1) nw = 1;
    g.nwaves = static_cast<uint32_t>((nw + 3) / 4 * 4);
    const uint64_t per = (g.nchunks + g.nwaves - 1) / g.nwaves; // every row of a wave's share may be a candidate
    g.seg_cap = static_cast<uint32_t>((per ? per : 1) * g.chunk_rows);
    return g;
}

hipError_t launch_group_scan(const ScanArgs& a, const ScanGeometry& g, const GroupArgs& ga, hipStream_t s)
{
    switch (a.W) {
    case 4: return launch_group_t<4, 4, false>(a, g, ga, s);
    case 8: return launch_group_t<8, 4, false>(a, g, ga, s);
    case 16: return launch_group_t<16, 4, true>(a, g, ga, s);
    case 32: return launch_group_t<32, 2, true>(a, g, ga, s);
    case 64: return launch_group_t<64, 1, true>(a, g, ga, s);
    default: return launch_group_t<0, 1, false>(a, g, ga, s);
    }
}

hipError_t launch_group_which(const ScanArgs& a, const GroupArgs& ga, uint32_t row_base, void* block, uint32_t h0, uint32_t h1, hipStream_t s)
{
    if (h1 <= h0) return hipSuccess;
    hipLaunchKernelGGL(group_which_kernel, dim3((h1 - h0 + 255u) / 256u), dim3(256), 0, s, a, ga, row_base, block, h0, h1);
    return hipGetLastError();
}

} // namespace gsim
