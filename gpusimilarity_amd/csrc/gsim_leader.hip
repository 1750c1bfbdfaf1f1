// gsim_leader.hip -- leader (sphere-exclusion) clustering (gsim_db_leader).  The rule is stated in include/gpusim_hip.h.
//
// The call keeps an ACTIVE LIST: the unassigned non-seed rows, ascending.  A round takes the first B entries as candidates and
//   1. resolves them among themselves: leader_cover_kernel scores the candidate pairs (i < j) with the scan's arithmetic and leaves
//      one bit per pair, "i would cover j"; leader_resolve_kernel -- one workgroup, its first wave -- walks the candidates in order
//      under a mask of this round's leaders (candidate j is a leader unless an earlier leader of the round covers it; the earliest
//      such leader gets it; nobody becomes a leader past the cap), then all its threads append the new leaders, copy their rows and
//      popcounts into the dense round buffer and write the candidates' leader_of / row_score;
//   2. passes over the rest of the list (leader_pass_kernel, cut into launches): every lane gathers RPL whole rows by list entry
//      into registers and tests them against the round's leaders IN ORDER -- wave-uniform, read through a constant-address-space
//      pointer: scalar loads, the SGPR operand of v_and_b32, as group_scan_kernel -- and records the first leader that covers a row.
//      The decision is score_of(...) >= cutoff exactly: valu_surely_not_kept (gsim_prefilter.h) comes first, the divide runs only
//      for the pairs it lets through.  A lane whose rows are all covered stops contributing, and the wave leaves the leader loop
//      when a ballot says nobody is left.  Stores (gfx950 has one in-order vmcnt) come after the chunk's leader loop;
//   3. compacts the list in order (rocPRIM select under "leader_of[row] is still none") into the other list buffer.
// Seed rounds are rounds whose leaders are given: no resolve.  By induction every row on the list has been compared with every
// leader made so far, the candidates are the lowest unassigned rows, and the pass takes the round's leaders in order: the result is
// the sequential walk's whatever B is and however a pass is cut into launches.  Nothing waits across workgroups.
#include "gsim_device.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_prefilter.h"

namespace gsim
{
namespace
{

typedef const __attribute__((address_space(4))) uint32_t* ConstWords; // constant address space: wave-uniform reads are scalar loads
typedef int s8 __attribute__((ext_vector_type(8)));                   // an 8-dword SGPR tuple

template <bool NT> __device__ __forceinline__ u32x4 row_load(const u32x4* p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// Does the leader (popcount qa) cover the row (popcount bb, cc bits in common)?  Exactly score_of(...) >= cutoff; NaN never does.
__device__ __forceinline__ bool covers(const LeaderArgs& a, float cut_lo, uint32_t qa, uint32_t bb, uint32_t cc, float& s)
{
    const float den = score_den(a.metric, a.alpha, a.beta, qa, bb, cc);
    const float cf = static_cast<float>(static_cast<int>(cc));
    if (valu_surely_not_kept(cut_lo, cf, den, cc)) return false;
    s = __fdiv_rn(cf, den); // (== score_of(...) bit for bit: gsim_device_common.h)
    return s >= a.cutoff;
}

// WORDS != 0: rows of WORDS words (a multiple of 4) held in registers, RPL rows per lane; MANUAL: the leaders' words in 8-word
// blocks double-buffered by hand (WORDS % 16 == 0), as group_scan_kernel -- see the warning there: after ANY change to the leader
// loop read the ISA again (both tuples in fixed SGPR ranges, no s_mov of them before the wait, SGPR spills 0; DESIGN.md
// section 14).  WORDS == 0: any width, one row per lane, word by word.  NT: non-temporal row loads.
// Chunk c of the launch (64 * RPL list entries from e0 on) belongs to wave c % nwaves.
template <int WORDS, int RPL, bool MANUAL, bool NT>
__global__ __launch_bounds__(kScanBlock) void leader_pass_kernel(LeaderArgs a, const uint32_t* __restrict__ list, u64 e0, u64 e1, uint32_t nwaves)
{
    const int lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (threadIdx.x >> 6));
    const uint32_t nl = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a.ctl[kLdrRoundNl])));
    const uint32_t pos0 = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(a.ctl[kLdrRoundPos])));
    const ConstWords qbase = (ConstWords) a.round_fp;
    const float cut_lo = valu_cutoff_lo(a.cutoff);
    u64 pairs = 0;        // wave-uniform: leader x row scores this wave's rows needed
    uint32_t covered = 0; // ... and the rows it found a leader for
    if (nl == 0) return;

    if constexpr (WORDS != 0) {
        static_assert(!MANUAL || WORDS % 16 == 0, "the hand-scheduled loads alternate two 8-word buffers");
        constexpr int CHR = 64 * RPL;
        constexpr int NB = WORDS / 8;
        const u32x4* __restrict__ db = reinterpret_cast<const u32x4*>(a.rows);
        const u64 nchunks = (e1 - e0 + CHR - 1) / CHR;
        uint32_t idxn[RPL];
        bool actn[RPL];
#pragma unroll
        for (int r = 0; r < RPL; r++) {
            const u64 e = e0 + static_cast<u64>(w) * CHR + r * 64 + lane;
            actn[r] = w < nchunks && e < e1;
            idxn[r] = actn[r] ? list[e] : 0u;
        }
        for (u64 c = w; c < nchunks; c += nwaves) {
            u32x4 r4[RPL][WORDS / 4];
            uint32_t bb[RPL], idx[RPL];
            bool active[RPL];
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                idx[r] = idxn[r];
                active[r] = actn[r];
                const u32x4* p = db + static_cast<u64>(idx[r]) * (WORDS / 4);
#pragma unroll
                for (int j = 0; j < WORDS / 4; j++) r4[r][j] = active[r] ? row_load<NT>(p + j) : u32x4{0, 0, 0, 0};
            }
            // the next chunk's list entries, behind this chunk's rows on the one in-order vmcnt: they land under the leader loop
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                const u64 e = e0 + (c + nwaves) * CHR + r * 64 + lane;
                actn[r] = c + nwaves < nchunks && e < e1;
                idxn[r] = actn[r] ? list[e] : 0u;
            }
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                bb[r] = 0;
#pragma unroll
                for (int j = 0; j < WORDS / 4; j++) bb[r] += __popc(r4[r][j].x) + __popc(r4[r][j].y) + __popc(r4[r][j].z) + __popc(r4[r][j].w);
            }

            bool alive[RPL];
            uint32_t covq[RPL];
            float covs[RPL];
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                alive[r] = active[r];
                covq[r] = 0;
                covs[r] = 0.0f;
            }
            s8 qA, qB;
            if constexpr (MANUAL) asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=s"(qA) : "s"(qbase));
            bool go = true;
            for (uint32_t q0 = 0; go && q0 < nl; q0 += 64) {
                // the popcounts of 64 leaders in a VGPR (lane i: leader q0 + i), read with v_readlane (as group_scan_kernel)
                const uint32_t vqpop = q0 + lane < nl ? a.round_pop[q0 + lane] : 0u;
                const uint32_t qn = nl - q0 < 64u ? nl - q0 : 64u;
                for (uint32_t qq = 0; qq < qn; qq++) {
                    const uint32_t q = q0 + qq;
                    const ConstWords qw = qbase + static_cast<size_t>(q) * WORDS;
                    uint32_t cnt[RPL][4];
#pragma unroll
                    for (int r = 0; r < RPL; r++) cnt[r][0] = cnt[r][1] = cnt[r][2] = cnt[r][3] = 0;
                    if constexpr (MANUAL) {
                        // the next block (or the next leader's first) is in flight while this one is reduced; scalar loads return
                        // out of order, hence lgkmcnt(0) before a buffer is used
#pragma unroll
                        for (int blk = 0; blk < NB; blk++) {
                            s8& cur = (blk & 1) ? qB : qA; // NB is even: block 0 of every leader is qA
                            s8& nxt = (blk & 1) ? qA : qB;
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            __builtin_amdgcn_sched_barrier(0);
                            if (blk + 1 < NB) {
                                asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(nxt) : "s"(qw), "n"((blk + 1) * 32));
                            } else if (q + 1 < nl) {
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
                    bool any = false;
#pragma unroll
                    for (int r = 0; r < RPL; r++) {
                        const uint32_t cc = (cnt[r][0] + cnt[r][1]) + (cnt[r][2] + cnt[r][3]);
                        float s = 0.0f;
                        if (alive[r] && covers(a, cut_lo, qa, bb[r], cc, s)) {
                            alive[r] = false;
                            covq[r] = q;
                            covs[r] = s;
                        }
                        any = any || alive[r];
                    }
                    if (__ballot(any) == 0) { // nobody left: the wave leaves the leader loop
                        go = false;
                        break;
                    }
                }
            }
            // (an early exit leaves the next leader's first block in flight: it has to land before its registers mean anything else)
            if constexpr (MANUAL) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            uint32_t tested = 0, got = 0;
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                if (active[r] && !alive[r]) {
                    a.leader_of[idx[r]] = pos0 + covq[r];
                    if (a.row_score) a.row_score[idx[r]] = covs[r];
                    tested += covq[r] + 1u;
                    got++;
                } else if (active[r]) {
                    tested += nl;
                }
            }
            pairs += wave_sum(tested);
            covered += wave_sum(got);
        }
    } else {
        const uint32_t* __restrict__ db = static_cast<const uint32_t*>(a.rows);
        const ConstWords qpop = (ConstWords) a.round_pop;
        const uint32_t W = a.W;
        const u64 nchunks = (e1 - e0 + 63) / 64;
        for (u64 c = w; c < nchunks; c += nwaves) {
            const u64 e = e0 + c * 64u + static_cast<uint32_t>(lane);
            const bool active = e < e1;
            const uint32_t idx = active ? list[e] : 0u;
            const uint32_t* r = db + static_cast<u64>(idx) * W;
            uint32_t bb = 0;
            if (active)
                for (uint32_t i = 0; i < W; i++) bb += __popc(r[i]);
            bool alive = active;
            uint32_t covq = 0;
            float covs = 0.0f;
            for (uint32_t q = 0; q < nl; q++) {
                const ConstWords qw = qbase + static_cast<size_t>(q) * W;
                if (alive) {
                    uint32_t cc = 0;
                    for (uint32_t i = 0; i < W; i++) cc += __popc(r[i] & qw[i]);
                    float s = 0.0f;
                    if (covers(a, cut_lo, qpop[q], bb, cc, s)) {
                        alive = false;
                        covq = q;
                        covs = s;
                    }
                }
                if (__ballot(alive) == 0) break;
            }
            uint32_t tested = 0, got = 0;
            if (active && !alive) {
                a.leader_of[idx] = pos0 + covq;
                if (a.row_score) a.row_score[idx] = covs;
                tested = covq + 1u;
                got = 1;
            } else if (active) {
                tested = nl;
            }
            pairs += wave_sum(tested);
            covered += wave_sum(got);
        }
    }
    if (lane == 0) {
        if (pairs) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl + kLdrPairs), pairs);
        if (covered) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctl + kLdrAssigned), static_cast<u64>(covered));
    }
}

// inner product and popcounts of two rows, word by word
__device__ __forceinline__ void pair_counts(const uint32_t* x, const uint32_t* y, uint32_t W, uint32_t& px, uint32_t& py, uint32_t& cc)
{
    px = py = cc = 0;
    for (uint32_t i = 0; i < W; i++) {
        const uint32_t u = x[i], v = y[i];
        px += __popc(u);
        py += __popc(v);
        cc += __popc(u & v);
    }
}

// One wave per (candidate j, 64 earlier candidates): bit i % 64 of cover[j * nwords + i / 64] = "score(candidate i, candidate j) >=
// cutoff", for i < j only.  Words past j / 64 are not written (and not read).
__global__ __launch_bounds__(256) void leader_cover_kernel(LeaderArgs a, const uint32_t* __restrict__ list, uint32_t nc, uint32_t nwords)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t j = wid / nwords, wd = wid % nwords;
    if (j >= nc || wd * 64u > j) return;
    const uint32_t i = wd * 64u + static_cast<uint32_t>(lane);
    const bool valid = i < j;
    const uint32_t* rows = static_cast<const uint32_t*>(a.rows);
    const uint32_t* rj = rows + static_cast<u64>(list[j]) * a.W;
    const uint32_t* ri = rows + static_cast<u64>(list[valid ? i : j]) * a.W;
    uint32_t pa, pb, cc;
    pair_counts(ri, rj, a.W, pa, pb, cc);
    const float s = score_of(a.metric, a.alpha, a.beta, pa, pb, cc); // (the leader is the query: a = its popcount)
    const u64 m = __ballot(valid && s >= a.cutoff);
    if (lane == 0) a.cover[static_cast<u64>(j) * nwords + wd] = m;
}

// One workgroup.  Wave 0 walks the candidates in order (lane l keeps word l of the mask of this round's leaders), then every thread
// takes candidates: leaders are appended and copied into the round buffer, covered candidates get their leader and score.
__global__ __launch_bounds__(256) void leader_resolve_kernel(LeaderArgs a, const uint32_t* __restrict__ list, uint32_t nc, uint32_t nwords)
{
    __shared__ uint32_t s_by[kLeaderMaxRound];   // candidate -> the candidate that leads it (itself: a leader), or none
    __shared__ uint16_t s_ord[kLeaderMaxRound];  // candidate (a leader) -> its position among the round's leaders
    __shared__ uint16_t s_cand[kLeaderMaxRound]; // ... and back
    __shared__ uint32_t s_nl, s_assigned;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const uint32_t pos0 = a.ctl[kLdrLeaders];
    if (tid < 64) {
        u64 mask = 0;
        uint32_t nl = 0;
        const uint32_t room = a.max_leaders - pos0; // (>= 1: the host ends the call at the cap)
        for (uint32_t j0 = 0; j0 < nc; j0 += 8) {
            u64 cw[8];
#pragma unroll
            for (uint32_t t = 0; t < 8; t++) {
                const uint32_t j = j0 + t;
                cw[t] = j < nc && static_cast<uint32_t>(lane) <= (j >> 6) ? a.cover[static_cast<u64>(j) * nwords + lane] : 0ull;
            }
#pragma unroll
            for (uint32_t t = 0; t < 8; t++) {
                const uint32_t j = j0 + t;
                if (j >= nc) break;
                const u64 hit = cw[t] & mask;
                const u64 lanes = __ballot(hit != 0);
                uint32_t by = GSIM_LEADER_NONE;
                bool leads = false;
                if (lanes) {
                    const int l = __ffsll(static_cast<long long>(lanes)) - 1;
                    const uint32_t lo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(hit)), l, 64));
                    const uint32_t hi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(hit >> 32)), l, 64));
                    by = static_cast<uint32_t>(l) * 64u + (lo ? static_cast<uint32_t>(__ffs(static_cast<int>(lo))) - 1u : 32u + static_cast<uint32_t>(__ffs(static_cast<int>(hi))) - 1u);
                } else if (nl < room) {
                    leads = true;
                    by = j;
                    if (static_cast<uint32_t>(lane) == (j >> 6)) mask |= 1ull << (j & 63u);
                }
                if (lane == 0) {
                    s_by[j] = by;
                    if (leads) {
                        s_ord[j] = static_cast<uint16_t>(nl);
                        s_cand[nl] = static_cast<uint16_t>(j);
                    }
                }
                if (leads) nl++;
            }
        }
        if (lane == 0) {
            s_nl = nl;
            s_assigned = 0;
        }
    }
    __syncthreads();
    const uint32_t nl = s_nl;
    const uint32_t* rows = static_cast<const uint32_t*>(a.rows);
    uint32_t mine = 0;
    for (uint32_t j = static_cast<uint32_t>(tid); j < nc; j += 256u) {
        const uint32_t by = s_by[j];
        if (by == GSIM_LEADER_NONE) continue; // past the cap and not covered: stays unassigned
        const uint32_t row = list[j];
        const uint32_t* rj = rows + static_cast<u64>(row) * a.W;
        mine++;
        if (by == j) {
            const uint32_t q = s_ord[j];
            uint32_t pop = 0;
            for (uint32_t i = 0; i < a.W; i++) pop += __popc(rj[i]);
            a.round_pop[q] = pop;
            a.leaders[pos0 + q] = row;
            a.leader_of[row] = pos0 + q;
            if (a.row_score) a.row_score[row] = 1.0f;
        } else {
            a.leader_of[row] = pos0 + s_ord[by];
            if (a.row_score) {
                uint32_t pa, pb, cc;
                pair_counts(rows + static_cast<u64>(list[by]) * a.W, rj, a.W, pa, pb, cc);
                a.row_score[row] = score_of(a.metric, a.alpha, a.beta, pa, pb, cc);
            }
        }
    }
    for (uint32_t t = static_cast<uint32_t>(tid); t < nl * a.W; t += 256u) {
        const uint32_t q = t / a.W, i = t % a.W;
        a.round_fp[t] = rows[static_cast<u64>(list[s_cand[q]]) * a.W + i];
    }
    if (mine) atomicAdd(&s_assigned, mine);
    __syncthreads();
    if (tid == 0) {
        a.ctl[kLdrRoundNl] = nl;
        a.ctl[kLdrRoundPos] = pos0;
        a.ctl[kLdrLeaders] = pos0 + nl;
        // the pairs scored for the walk: candidate i < candidate j
        *reinterpret_cast<unsigned long long*>(a.ctl + kLdrPairs) += static_cast<u64>(nc) * (nc - 1u) / 2u;
        *reinterpret_cast<unsigned long long*>(a.ctl + kLdrAssigned) += s_assigned;
    }
}

// A seed round: leaders[pos0 .. pos0 + nc) into the round buffer
__global__ __launch_bounds__(256) void leader_seed_round_kernel(LeaderArgs a, uint32_t pos0, uint32_t nc)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t* rows = static_cast<const uint32_t*>(a.rows);
    for (uint32_t q = tid; q < nc; q += 256u) {
        const uint32_t* r = rows + static_cast<u64>(a.leaders[pos0 + q]) * a.W;
        uint32_t pop = 0;
        for (uint32_t i = 0; i < a.W; i++) pop += __popc(r[i]);
        a.round_pop[q] = pop;
    }
    for (uint32_t t = tid; t < nc * a.W; t += 256u) {
        const uint32_t q = t / a.W, i = t % a.W;
        a.round_fp[t] = rows[static_cast<u64>(a.leaders[pos0 + q]) * a.W + i];
    }
    if (tid == 0) {
        a.ctl[kLdrRoundNl] = nc;
        a.ctl[kLdrRoundPos] = pos0;
        a.ctl[kLdrLeaders] = pos0 + nc;
    }
}

// the seeds are leaders from the start: leader_of / row_score of leaders[0 .. nseeds)
__global__ __launch_bounds__(256) void leader_seed_mark_kernel(LeaderArgs a, uint32_t nseeds)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nseeds) return;
    const uint32_t row = a.leaders[j];
    a.leader_of[row] = j;
    if (a.row_score) a.row_score[row] = 1.0f;
}

struct Unassigned {
    const uint32_t* leader_of;
    __device__ bool operator()(const uint32_t& row) const { return leader_of[row] == GSIM_LEADER_NONE; }
};

template <int WORDS, int RPL, bool MANUAL>
hipError_t launch_pass_t(const LeaderArgs& a, const uint32_t* list, u64 e0, u64 e1, int num_cus, bool nt, hipStream_t s)
{
    const u64 nchunks = (e1 - e0 + 64u * RPL - 1) / (64u * RPL);
    // twelve waves per CU, as the group scan: the loop is VALU-bound
    u64 nw = static_cast<u64>(num_cus) * 12u;
    if (nw > nchunks) nw = nchunks;
    const uint32_t nwaves = static_cast<uint32_t>((nw + 3) / 4 * 4);
    const dim3 grid(nwaves / (kScanBlock / 64)), block(kScanBlock);
    if constexpr (WORDS != 0) {
        if (nt) hipLaunchKernelGGL((leader_pass_kernel<WORDS, RPL, MANUAL, true>), grid, block, 0, s, a, list, e0, e1, nwaves);
        else hipLaunchKernelGGL((leader_pass_kernel<WORDS, RPL, MANUAL, false>), grid, block, 0, s, a, list, e0, e1, nwaves);
    } else {
        hipLaunchKernelGGL((leader_pass_kernel<0, 1, false, false>), grid, block, 0, s, a, list, e0, e1, nwaves);
    }
    return hipGetLastError();
}

} // namespace

uint32_t leader_chunk_rows(uint32_t W)
{
    return 64u * (W == 4 || W == 8 || W == 16 ? 4u : (W == 32 ? 2u : 1u));
}

hipError_t launch_leader_pass(const LeaderArgs& a, const uint32_t* list, uint64_t e0, uint64_t e1, int num_cus, bool nt, hipStream_t s)
{
    if (e1 <= e0) return hipSuccess;
    switch (a.W) {
    case 4: return launch_pass_t<4, 4, false>(a, list, e0, e1, num_cus, nt, s);
    case 8: return launch_pass_t<8, 4, false>(a, list, e0, e1, num_cus, nt, s);
    case 16: return launch_pass_t<16, 4, true>(a, list, e0, e1, num_cus, nt, s);
    case 32: return launch_pass_t<32, 2, true>(a, list, e0, e1, num_cus, nt, s);
    case 64: return launch_pass_t<64, 1, true>(a, list, e0, e1, num_cus, nt, s);
    default: return launch_pass_t<0, 1, false>(a, list, e0, e1, num_cus, nt, s);
    }
}

hipError_t launch_leader_resolve(const LeaderArgs& a, const uint32_t* list, uint32_t nc, hipStream_t s)
{
    if (nc == 0 || nc > kLeaderMaxRound) return hipErrorInvalidValue;
    const uint32_t nwords = (nc + 63u) / 64u;
    const uint32_t waves = nc * nwords;
    hipLaunchKernelGGL(leader_cover_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, s, a, list, nc, nwords);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(leader_resolve_kernel, dim3(1), dim3(256), 0, s, a, list, nc, nwords);
    return hipGetLastError();
}

hipError_t launch_leader_seed_round(const LeaderArgs& a, uint32_t pos0, uint32_t nc, hipStream_t s)
{
    if (nc == 0 || nc > kLeaderMaxRound) return hipErrorInvalidValue;
    hipLaunchKernelGGL(leader_seed_round_kernel, dim3(1), dim3(256), 0, s, a, pos0, nc);
    return hipGetLastError();
}

hipError_t leader_select_bytes(uint64_t n, size_t* bytes)
{
    size_t b0 = 0, b1 = 0;
    hipError_t e = rocprim::select(nullptr, b0, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                   static_cast<size_t>(n), Unassigned{nullptr});
    if (e != hipSuccess) return e;
    e = rocprim::select(nullptr, b1, rocprim::counting_iterator<uint32_t>(0u), static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                        static_cast<size_t>(n), Unassigned{nullptr});
    *bytes = b0 > b1 ? b0 : b1;
    return e;
}

hipError_t launch_leader_first_list(const LeaderArgs& a, void* tmp, size_t tmp_bytes, uint64_t nrows, uint32_t nseeds, uint32_t* list_out, hipStream_t s)
{
    if (nseeds) {
        hipLaunchKernelGGL(leader_seed_mark_kernel, dim3((nseeds + 255u) / 256u), dim3(256), 0, s, a, nseeds);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return rocprim::select(tmp, tmp_bytes, rocprim::counting_iterator<uint32_t>(0u), list_out, a.ctl + kLdrActive, static_cast<size_t>(nrows),
                           Unassigned{a.leader_of}, s);
}

hipError_t launch_leader_compact(const LeaderArgs& a, void* tmp, size_t tmp_bytes, const uint32_t* list_in, uint64_t n, uint32_t* list_out, hipStream_t s)
{
    return rocprim::select(tmp, tmp_bytes, list_in, list_out, a.ctl + kLdrActive, static_cast<size_t>(n), Unassigned{a.leader_of}, s);
}

} // namespace gsim
