// gsim_scores.hip -- dense similarity matrices (gsim_db_scores, gsim_db_scores_queries, gsim_db_scores_device): every score of
// a block of left rows against a range of table rows, written as a matrix.  The rule is stated in include/gpusim_hip.h;
// DESIGN.md section 17 has the route and the measurements.
//
// A dense matrix keeps every pair, so nothing can be dropped by a pre-filter and the intersection counts are a plain 0/1
// GEMM: c(i, j) = sum over bits of left[i][k] table[j][k].  It runs on the matrix cores with the operand scheme of the
// multi-query pass (gsim_mfma_fp4.h): four v_mfma_scale_f32_32x32x64_f8f6f4 per 256-bit group and 32 x 32 tile, FP4 classes,
// f32 accumulators that hold the counts exactly.
//
//   * a workgroup (256 threads) computes a kScoresTile x kScoresTile = 128 x 128 block of the output, each of its four waves
//     a 64 x 64 quarter as 2 x 2 MFMA tiles: 64 accumulator registers, every expanded operand used twice;
//   * LEFT rows are the A operand, TABLE rows the B operand: table rows run along the lanes, so accumulator register r of
//     a tile holds, in lanes 0..31 and 32..63, 32 consecutive floats of the output rows (r & 3) + 8 (r >> 2) + 4 h -- every
//     store instruction writes two whole 128-byte pieces of output rows;
//   * the kernel loops over the 256-bit groups of a row, kScoresStageGroups at a time (any multiple of 256 bits up to 4096:
//     no whole row is ever in registers): the 128 + 128 rows' words of a step are loaded with coalesced 16-byte loads into
//     registers while the previous step's MFMAs run, and go through LDS (two buffers, one barrier per step; chunk c of row
//     r at chunk c ^ ((r >> 1) & 7) of its 128-byte line, which makes the lanes' 16-byte fragment reads conflict-free);
//   * rows of other widths are zero-padded copies (nbr_prepare_kernel, WP = the next multiple of 8 words): zero words change
//     no count.  popc of either side comes from that kernel's arrays, never from the padded rows;
//   * edge blocks: the row index of a load is clamped to the range's last row, the store is masked;
//   * epilogue per pair: c from the accumulator, score_den, ONE correctly rounded divide (== score_of bit for bit), and the
//     >= 0 select that turns 0 / 0 into 0.0f as apply_cutoff(., 0.0f) does; non-temporal stores (the output is written once
//     and is larger than the caches).
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_mfma_fp4.h"

namespace gsim
{
namespace
{

constexpr int kScoresStageGroups = 4;                      // 256-bit groups of every row staged per step
constexpr int kScoresStageChunks = 2 * kScoresStageGroups; // 16-byte chunks per row and step: one 128-byte LDS line
constexpr int kScoresPasses = 2 * kScoresTile * kScoresStageChunks / kScoresBlock; // 16-byte loads per thread and step

struct ScoresShared {
    u32x4 rows[2][2 * kScoresTile * kScoresStageChunks]; // [buffer][line = side * 128 + row][chunk, swizzled]
    uint32_t pop[2][kScoresTile];                        // popc of the block's left rows / table rows
};
static_assert(kScoresStageChunks == 8 && kScoresBlock % kScoresStageChunks == 0 && kScoresPasses * kScoresBlock == 2 * kScoresTile * kScoresStageChunks,
              "a step is one 128-byte line per row, a pass of the workgroup covers whole lines");
static_assert(sizeof(ScoresShared) <= 80 * 1024, "two workgroups per CU");

__device__ __forceinline__ int scores_swizzle(int row) { return (row >> 1) & 7; }

__global__ __launch_bounds__(kScoresBlock) void scores_kernel(ScoresArgs a, u64 l0, u64 r0)
{
    __shared__ ScoresShared sh;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int wr = wq >> 1, wc = wq & 1; // this wave's quarter: left rows wr * 64 .., table rows wc * 64 ..
    // this block's first left row and first table row (of the call's rectangle; both exist: the launch covers no empty block)
    const u64 lb = l0 + static_cast<u64>(blockIdx.y) * kScoresTile;
    const u64 rb = r0 + static_cast<u64>(blockIdx.x) * kScoresTile;
    const bool stamp = a.clk && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0;
    if (stamp) stamp_begin(a.clk);

    // ---- staging: thread t loads chunk t % 8 of line t / 8 + 32 p, p = 0 .. 7 (lines 0..127: left rows, 128..255: table rows) ----
    const int chunk = tid & (kScoresStageChunks - 1);
    const int line0 = tid / kScoresStageChunks;
    constexpr int kLinesPerPass = kScoresBlock / kScoresStageChunks;
    const uint32_t CPR = a.WP / 4; // 16-byte chunks per row
    const u32x4* src[kScoresPasses];
#pragma unroll
    for (int p = 0; p < kScoresPasses; p++) {
        const int line = line0 + p * kLinesPerPass;
        const bool left = line < kScoresTile;
        u64 row = (left ? lb : rb) + static_cast<u64>(line & (kScoresTile - 1));
        const u64 last = (left ? a.nl : a.nr) - 1;
        row = row < last ? row : last; // (edge blocks: nothing past either range is read)
        src[p] = reinterpret_cast<const u32x4*>(left ? a.lrows : a.rrows) + row * CPR + chunk;
    }
    if (tid < kScoresTile) {
        const u64 row = lb + tid < a.nl ? lb + tid : a.nl - 1;
        sh.pop[0][tid] = a.lpop[row];
    } else {
        const int t = tid - kScoresTile;
        const u64 row = rb + t < a.nr ? rb + t : a.nr - 1;
        sh.pop[1][t] = a.rpop[row];
    }
    u32x4 st[kScoresPasses];
    auto load_step = [&](uint32_t c0, uint32_t nchunks) { // chunks c0 .. c0 + nchunks - 1 of every row
#pragma unroll
        for (int p = 0; p < kScoresPasses; p++) st[p] = static_cast<uint32_t>(chunk) < nchunks ? src[p][c0] : u32x4{0, 0, 0, 0};
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int p = 0; p < kScoresPasses; p++) {
            const int line = line0 + p * kLinesPerPass;
            sh.rows[buf][line * kScoresStageChunks + (chunk ^ scores_swizzle(line))] = st[p];
        }
    };

    ClassMasks km{0x11111111u, 0x22222222u, 0x44444444u};
    asm volatile("" : "+v"(km.m1), "+v"(km.m2), "+v"(km.m4)); // keep them in VGPRs
    v16f acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++) acc[tm][tn] = v16f{};
    // this lane's operand lines: left rows wr * 64 + tm * 32 + i, table rows wc * 64 + tn * 32 + i
    int aline[2], bline[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        aline[t] = wr * 64 + t * 32 + i;
        bline[t] = kScoresTile + wc * 64 + t * 32 + i;
    }

    const uint32_t nchunks = CPR;
    load_step(0, nchunks < kScoresStageChunks ? nchunks : kScoresStageChunks);
    store_step(0);
    __syncthreads();
    int buf = 0;
    for (uint32_t c0 = 0; c0 < nchunks; c0 += kScoresStageChunks, buf ^= 1) {
        const uint32_t here = nchunks - c0 < kScoresStageChunks ? nchunks - c0 : kScoresStageChunks;
        const uint32_t next = c0 + kScoresStageChunks;
        const bool more = next < nchunks; // (workgroup-uniform)
        if (more) load_step(next, nchunks - next < kScoresStageChunks ? nchunks - next : kScoresStageChunks);
        const u32x4* rows = sh.rows[buf];
        for (uint32_t g = 0; g < here / 2; g++) {
            u32x4 xa[2], xb[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                xa[t] = rows[aline[t] * kScoresStageChunks + (static_cast<int>(2 * g + h) ^ scores_swizzle(aline[t]))];
                xb[t] = rows[bline[t] * kScoresStageChunks + (static_cast<int>(2 * g + h) ^ scores_swizzle(bline[t]))];
            }
#define GSIM_SCORES_CLASS(C)                                                                                   \
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
            GSIM_SCORES_CLASS(0)
            GSIM_SCORES_CLASS(1)
            GSIM_SCORES_CLASS(2)
            GSIM_SCORES_CLASS(3)
#undef GSIM_SCORES_CLASS
        }
        // the next step's buffer was last read in the previous iteration, which every wave left through the barrier below
        if (more) store_step(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: counts -> scores, 32 consecutive floats of one output row per lane half and register ----
    uint32_t bp[2];
    u64 col[2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const int c = wc * 64 + tn * 32 + i;
        bp[tn] = sh.pop[1][c];
        col[tn] = rb + static_cast<u64>(c);
    }
    typedef __attribute__((address_space(1))) float* g_f32p;
#pragma unroll
    for (int tm = 0; tm < 2; tm++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int lrow = wr * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const u64 row = lb + static_cast<u64>(lrow);
            const uint32_t ap = sh.pop[0][lrow];
            float* orow = a.out + row * a.ld;
#pragma unroll
            for (int tn = 0; tn < 2; tn++) {
                const float cf = acc[tm][tn][r];
                const float den = score_den(a.metric, a.alpha, a.beta, ap, bp[tn], static_cast<uint32_t>(cf));
                float s = __fdiv_rn(cf, den); // == score_of(metric, alpha, beta, ap, bp, c)
                s = s >= 0.0f ? s : 0.0f;     // apply_cutoff(s, 0.0f): NaN (0 / 0) is 0.0f
                if (row < a.nl && col[tn] < a.nr) __builtin_nontemporal_store(s, (g_f32p) (orow + col[tn]));
            }
        }
    }
    if (stamp) stamp_end(a.clk);
}

} // namespace

uint32_t scores_padded_words(uint32_t W)
{
    const uint32_t wp = (W + 7u) / 8u * 8u;
    return W == 0 || wp > kNbrMaxWords ? 0u : wp;
}

hipError_t launch_scores(const ScoresArgs& a, uint64_t l0, uint64_t l1, uint64_t r0, uint64_t r1, hipStream_t s)
{
    if (l0 >= l1 || r0 >= r1) return hipSuccess;
    if (l1 > a.nl || r1 > a.nr || l0 % kScoresTile || r0 % kScoresTile || a.WP == 0 || a.WP % 8 || a.WP > kNbrMaxWords || a.ld < a.nr)
        return hipErrorInvalidValue;
    const u64 by = (l1 - l0 + kScoresTile - 1) / kScoresTile, bx = (r1 - r0 + kScoresTile - 1) / kScoresTile;
    if (by > 65535u || bx > 0x7FFFFFFFu) return hipErrorInvalidValue;
    // (the kernel masks its stores with a.nl / a.nr: a launch that ends inside the rectangle ends on a block boundary)
    if ((l1 != a.nl && l1 % kScoresTile) || (r1 != a.nr && r1 % kScoresTile)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scores_kernel, dim3(static_cast<uint32_t>(bx), static_cast<uint32_t>(by)), dim3(kScoresBlock), 0, s, a, l0, r0);
    return hipGetLastError();
}

} // namespace gsim
