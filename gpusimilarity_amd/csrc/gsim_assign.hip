// gsim_assign.hip -- nearest-centre assignment (gsim_db_assign, the assign step of gsim_db_kmeans): for every table row of a
// range the centre with the greatest score and that score.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 21
// has the route and the measurements.
//
// The contraction is gsim_scores.hip's, unchanged: CENTRES are the A operand, TABLE rows the B operand along the lanes, four
// v_mfma_scale_f32_32x32x64_f8f6f4 per 256-bit group and 32 x 32 tile (gsim_mfma_fp4.h), 128 centres x 128 rows per workgroup
// and pass, staged through LDS with the same swizzle and the same one-barrier-per-step double buffer.  What differs:
//
//   * a workgroup keeps ONE block of 128 table rows and loops over all the centre blocks itself.  Its rows are staged again
//     for every centre block -- 128 rows are at most 64 KB and come from L2 after the first pass -- so the table is read from
//     memory once and a centre block's pass is exactly the scores kernel's block, operands included; nothing of a row block
//     meets another workgroup, so there are no global atomics;
//   * the epilogue keeps instead of storing.  Accumulator register r of a tile is centre (r & 3) + 8 (r >> 2) + 4 h of the
//     tile against the lane's OWN table row: the arg-max over a lane's 32 registers of a row is register-local.  Per pair the
//     scores kernel's epilogue (score_den, one correctly rounded divide, the >= 0 select), then the 64-bit key
//     (score bits << 32) | ~centre: non-negative floats order as their bit patterns, so the greatest key is the greatest f32
//     score and, among equal scores, the lowest centre.  A centre past m (the last block's clamped loads) gets key 0, below
//     every real key.  The comparison is on the ROUNDED score, as the rule demands: no cross-multiplied shortcut;
//   * at the end one __shfl_xor(., 32) joins the lane halves (the other 16 centres of every tile), LDS joins the two waves
//     that share table rows (wr = 0, 1), and 128 threads store label and score: 8 bytes a row;
//   * the centres' popcounts of a block sit in LDS in two buffers by block parity: a wave that has gone on to the next block
//     writes the other buffer while a slower wave still reads this one in its epilogue; the barriers of the next block's
//     steps separate block b from b + 2.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_mfma_fp4.h"

namespace gsim
{
namespace
{

constexpr int kAssignStageGroups = 4;                      // as the scores kernel: 256-bit groups of every row staged per step
constexpr int kAssignStageChunks = 2 * kAssignStageGroups; // 16-byte chunks per row and step: one 128-byte LDS line
constexpr int kAssignPasses = 2 * kScoresTile * kAssignStageChunks / kScoresBlock;

struct AssignShared {
    u32x4 rows[2][2 * kScoresTile * kAssignStageChunks]; // [buffer][line = side * 128 + row][chunk, swizzled]
    uint32_t cpop[2][kScoresTile];                       // popc of a centre block, by the block's parity
    uint32_t rpop[kScoresTile];                          // popc of the workgroup's table rows
    unsigned long long best[2][kScoresTile];             // the join of the waves wr = 0, 1
};
static_assert(kAssignStageChunks == 8 && kAssignPasses * kScoresBlock == 2 * kScoresTile * kAssignStageChunks, "a step is one 128-byte line per row");
static_assert(sizeof(AssignShared) <= 80 * 1024, "two workgroups per CU");

__device__ __forceinline__ int assign_swizzle(int row) { return (row >> 1) & 7; }

__global__ __launch_bounds__(kScoresBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void assign_kernel(AssignArgs a, u64 r0)
{
    __shared__ AssignShared sh;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int wr = wq >> 1, wc = wq & 1; // this wave's quarter: centres wr * 64 .. of a block, table rows wc * 64 ..
    const u64 rb = r0 + static_cast<u64>(blockIdx.x) * kScoresTile; // this workgroup's first table row (it exists)
    const bool stamp = a.clk && blockIdx.x == 0 && tid == 0;
    if (stamp) stamp_begin(a.clk);

    // ---- staging: thread t loads chunk t % 8 of line t / 8 + 32 p, p = 0 .. 7 (lines 0..127: centres, 128..255: table rows) ----
    const int chunk = tid & (kAssignStageChunks - 1);
    const int line0 = tid / kAssignStageChunks;
    constexpr int kLinesPerPass = kScoresBlock / kAssignStageChunks;
    const uint32_t CPR = a.WP / 4; // 16-byte chunks per row
    const u32x4* src[kAssignPasses];
#pragma unroll
    for (int p = kAssignPasses / 2; p < kAssignPasses; p++) { // (the table rows' lines: the same for every centre block)
        u64 row = rb + static_cast<u64>((line0 + p * kLinesPerPass) & (kScoresTile - 1));
        row = row < a.nr - 1 ? row : a.nr - 1; // (the last block: nothing past the slab is read)
        src[p] = reinterpret_cast<const u32x4*>(a.rows) + row * CPR + chunk;
    }
    if (tid < kScoresTile) {
        const u64 row = rb + tid < a.nr ? rb + tid : a.nr - 1;
        sh.rpop[tid] = a.rpop[row];
    }
    u32x4 st[kAssignPasses];
    auto load_step = [&](uint32_t c0, uint32_t nchunks) { // chunks c0 .. c0 + nchunks - 1 of every row
#pragma unroll
        for (int p = 0; p < kAssignPasses; p++) st[p] = static_cast<uint32_t>(chunk) < nchunks ? src[p][c0] : u32x4{0, 0, 0, 0};
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int p = 0; p < kAssignPasses; p++) {
            const int line = line0 + p * kLinesPerPass;
            sh.rows[buf][line * kAssignStageChunks + (chunk ^ assign_swizzle(line))] = st[p];
        }
    };

    ClassMasks km{0x11111111u, 0x22222222u, 0x44444444u};
    asm volatile("" : "+v"(km.m1), "+v"(km.m2), "+v"(km.m4)); // keep them in VGPRs
    // this lane's operand lines: centres wr * 64 + tm * 32 + i of the block, table rows wc * 64 + tn * 32 + i
    int aline[2], bline[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        aline[t] = wr * 64 + t * 32 + i;
        bline[t] = kScoresTile + wc * 64 + t * 32 + i;
    }
    unsigned long long best[2] = {0, 0}; // of the lane's table rows wc * 64 + tn * 32 + i

    const uint32_t nchunks = CPR;
    const uint32_t nblocks = (a.m + kScoresTile - 1) / kScoresTile;
    for (uint32_t cb = 0; cb < nblocks; cb++) { // (workgroup-uniform)
        const uint32_t c_first = cb * kScoresTile;
        const int par = static_cast<int>(cb & 1u);
#pragma unroll
        for (int p = 0; p < kAssignPasses / 2; p++) { // the centres' lines
            uint32_t c = c_first + static_cast<uint32_t>(line0 + p * kLinesPerPass);
            c = c < a.m - 1 ? c : a.m - 1; // (the last block: the last centre again; its keys are masked below)
            src[p] = reinterpret_cast<const u32x4*>(a.centres) + static_cast<size_t>(c) * CPR + chunk;
        }
        if (tid < kScoresTile) {
            const uint32_t c = c_first + tid < a.m ? c_first + tid : a.m - 1;
            sh.cpop[par][tid] = a.cpop[c];
        }
        v16f acc[2][2];
#pragma unroll
        for (int tm = 0; tm < 2; tm++)
#pragma unroll
            for (int tn = 0; tn < 2; tn++) acc[tm][tn] = v16f{};

        // (buffer 0 was last read two barriers ago at the latest: every block ends behind the barrier of its last step)
        load_step(0, nchunks < kAssignStageChunks ? nchunks : kAssignStageChunks);
        store_step(0);
        __syncthreads();
        int buf = 0;
        for (uint32_t c0 = 0; c0 < nchunks; c0 += kAssignStageChunks, buf ^= 1) {
            const uint32_t here = nchunks - c0 < kAssignStageChunks ? nchunks - c0 : kAssignStageChunks;
            const uint32_t next = c0 + kAssignStageChunks;
            const bool more = next < nchunks; // (workgroup-uniform)
            if (more) load_step(next, nchunks - next < kAssignStageChunks ? nchunks - next : kAssignStageChunks);
            const u32x4* rows = sh.rows[buf];
            for (uint32_t g = 0; g < here / 2; g++) {
                u32x4 xa[2], xb[2];
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    xa[t] = rows[aline[t] * kAssignStageChunks + (static_cast<int>(2 * g + h) ^ assign_swizzle(aline[t]))];
                    xb[t] = rows[bline[t] * kAssignStageChunks + (static_cast<int>(2 * g + h) ^ assign_swizzle(bline[t]))];
                }
#define GSIM_ASSIGN_CLASS(C)                                                                                   \
    {                                                                                                          \
        v4i ea[2], eb[2];                                                                                      \
        _Pragma("unroll") for (int t = 0; t < 2; t++)                                                          \
        {                                                                                                      \
            ea[t] = fp4_class<C>(xa[t], km);                                                                   \
            eb[t] = fp4_class<C>(xb[t], km);                                                                   \
        }                                                                                                      \
        _Pragma("unroll") for (int tm = 0; tm < 2; tm++)                                                       \
            _Pragma("unroll") for (int tn = 0; tn < 2; tn++) acc[tm][tn] = mfma_class<C>(ea[tm], eb[tn], acc[tm][tn]); \
    }
                GSIM_ASSIGN_CLASS(0)
                GSIM_ASSIGN_CLASS(1)
                GSIM_ASSIGN_CLASS(2)
                GSIM_ASSIGN_CLASS(3)
#undef GSIM_ASSIGN_CLASS
            }
            // the next step's buffer was last read in the previous iteration, which every wave left through the barrier below
            if (more) store_step(buf ^ 1);
            __syncthreads();
        }

        // ---- epilogue: counts -> scores -> keys; register r is one centre, the lane is one table row ----
        uint32_t bp[2];
#pragma unroll
        for (int tn = 0; tn < 2; tn++) bp[tn] = sh.rpop[wc * 64 + tn * 32 + i];
#pragma unroll
        for (int tm = 0; tm < 2; tm++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int cl = wr * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const uint32_t centre = c_first + static_cast<uint32_t>(cl);
                const uint32_t ap = sh.cpop[par][cl];
                const bool real = centre < a.m;
#pragma unroll
                for (int tn = 0; tn < 2; tn++) {
                    const float cf = acc[tm][tn][r];
                    const float den = score_den(a.metric, a.alpha, a.beta, ap, bp[tn], static_cast<uint32_t>(cf));
                    float s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, ap, bp, c)
                    s = s >= 0.0f ? s : 0.0f;     // apply_cutoff(s, 0.0f): NaN (0 / 0) is 0.0f
                    const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(s)) << 32) | static_cast<unsigned long long>(~centre);
                    const unsigned long long k = real ? key : 0ull;
                    best[tn] = k > best[tn] ? k : best[tn];
                }
            }
        }
    }

    // ---- the lane halves, then the two waves that share table rows ----
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const unsigned long long o = __shfl_xor(best[tn], 32);
        best[tn] = o > best[tn] ? o : best[tn];
        if (h == 0) sh.best[wr][wc * 64 + tn * 32 + i] = best[tn];
    }
    __syncthreads();
    if (tid < kScoresTile) {
        const unsigned long long k0 = sh.best[0][tid], k1 = sh.best[1][tid];
        const unsigned long long k = k0 > k1 ? k0 : k1;
        const u64 row = rb + static_cast<u64>(tid);
        if (row < a.nr) {
            a.label[row] = ~static_cast<uint32_t>(k);
            a.score[row] = __uint_as_float(static_cast<uint32_t>(k >> 32));
        }
    }
    if (stamp) stamp_end(a.clk);
}

} // namespace

hipError_t launch_assign(const AssignArgs& a, uint64_t r0, uint64_t r1, hipStream_t s)
{
    if (r0 >= r1) return hipSuccess;
    if (r1 > a.nr || r0 % kScoresTile || (r1 != a.nr && r1 % kScoresTile) || a.m == 0 || a.m > GSIM_ASSIGN_MAX_CENTRES || a.WP == 0 || a.WP % 8 ||
        a.WP > kNbrMaxWords || !a.centres || !a.rows || !a.cpop || !a.rpop || !a.label || !a.score)
        return hipErrorInvalidValue;
    const u64 blocks = (r1 - r0 + kScoresTile - 1) / kScoresTile;
    if (blocks > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assign_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kScoresBlock), 0, s, a, r0);
    return hipGetLastError();
}

} // namespace gsim
