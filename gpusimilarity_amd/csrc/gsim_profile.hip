// gsim_profile.hip -- the two streaming passes behind the column-wise questions about a table (gsim_db_bit_counts,
// gsim_db_overlap_sums).  The rules are stated in include/gpusim_hip.h; DESIGN.md section 20 has the routes, the budget per
// word and the measurements.
//
// 1. Column counts: a positional popcount.  counts[k] = the number of counted rows with bit k set.
//   * a thread keeps ONE position of the row -- a 16-byte chunk (rows of a multiple of four words) or a single word (every
//     other width) -- and walks rows: the kProfileBlock threads of a workgroup are R = 256 / (positions per row) row lanes x
//     the positions, so one load instruction of the workgroup reads R whole consecutive rows, contiguously;
//   * the words go into bit-sliced vertical counters, Harley-Seal: eight rows are folded by seven carry-save adders into the
//     planes 1, 2, 4 and one word of weight 8, which ripples into the planes 8 ... 2048.  Twelve planes hold 4095; a
//     workgroup's slice gives a thread at most kProfileMaxIters rows, so no plane overflows and the planes are unpacked once,
//     at the end of the slice, and only as many of them as the slice can have filled;
//   * unpacked bits go into the workgroup's LDS counters (one per column; a thread starts at the column of its own position, so
//     that the 32 positions of a wave hit 32 different banks: with all of them on one bank the adds were the longest part of the
//     kernel at 1 M rows).  A workgroup takes every gridDim-th slice of the launch and keeps its LDS counters across them; at the
//     end it stores them as one row of a partials buffer, and a small reduce kernel adds the rows into the global 64-bit
//     counters with at most 32 atomic adds per counter.  Integer adds commute: the result does not depend on the grid, the
//     slices or the launches;
//   * a row set: its bitmap masks the streamed rows (every row is read; the words of an unselected row are cleared), or the
//     launch walks the set's ascending list instead of the row numbers.  Loads are never skipped under a lane's condition
//     -- the index is clamped and the value masked -- so that the eight loads of a step stay in flight together.
//
// 2. Weighted popcounts: sums[i] = sum over the set bits k of row i of weights[k], as sum_b 2^b |row_i AND plane_b| over the
//    at most 32 bit planes of the weights: a 0/1 product of the table against 32 "queries".
//   * rows of whole 256-bit groups: on the matrix cores with the operand scheme of gsim_scores.hip (gsim_mfma_fp4.h): the
//     planes are the A operand (one 32-wide tile, in LDS), 32 table rows the B operand, loaded straight from the table; the
//     f32 accumulators hold the 32 x 32 counts exactly; the epilogue shifts and adds the 16 counts of a lane in 64-bit
//     integers and adds the two lane halves.  The cost does not depend on the data or on the weights;
//   * every width: a VALU kernel.  G = min(64, next power of two >= W) lanes share a row, lane g owns the words g and g + G;
//     its one or two words of every plane stay in registers for the whole launch, so a row costs one coalesced load (four
//     rows of a lane are in flight), popc(word AND plane) with the add folded in (v_bcnt) and one shift-add per plane -- the
//     planes 0 .. 15 and 16 .. 31 summed apart in 32 bits -- and log2 G shuffles.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_mfma_fp4.h"

namespace gsim
{
namespace
{

constexpr int kProfPlanes = 12; // vertical counter planes of a word: counts up to 4095 >= kProfileMaxIters
static_assert(kProfileMaxIters % 8 == 0 && kProfileMaxIters < (1u << kProfPlanes), "a thread's planes never overflow");
constexpr uint32_t kProfMaxBits = 4096;

template <int V> __device__ __forceinline__ void prof_load(const uint32_t* p, uint32_t (&x)[V])
{
    if constexpr (V == 4) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); // (read once: as the scans' stream_load)
        x[0] = v.x;
        x[1] = v.y;
        x[2] = v.z;
        x[3] = v.w;
    } else {
        x[0] = __builtin_nontemporal_load(p);
    }
}

// carry-save adder: a + b + c = 2 * carry + sum, bit by bit
__device__ __forceinline__ void prof_csa(uint32_t a, uint32_t b, uint32_t c, uint32_t& carry, uint32_t& sum)
{
    const uint32_t u = a ^ b;
    carry = (a & b) | (u & c);
    sum = u ^ c;
}

// eight words into the vertical counter c[0 .. kProfPlanes) of one word position
__device__ __forceinline__ void prof_add8(uint32_t (&c)[kProfPlanes], uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4, uint32_t x5,
                                          uint32_t x6, uint32_t x7)
{
    uint32_t ta, tb, fa, fb, e;
    prof_csa(c[0], x0, x1, ta, c[0]);
    prof_csa(c[0], x2, x3, tb, c[0]);
    prof_csa(c[1], ta, tb, fa, c[1]);
    prof_csa(c[0], x4, x5, ta, c[0]);
    prof_csa(c[0], x6, x7, tb, c[0]);
    prof_csa(c[1], ta, tb, fb, c[1]);
    prof_csa(c[2], fa, fb, e, c[2]);
#pragma unroll
    for (int j = 3; j < kProfPlanes; j++) { // ripple the word of weight 8 upwards
        const uint32_t t = c[j] & e;
        c[j] ^= e;
        e = t;
    }
}

// MODE 0: rows [i0, i1); 1: the same under a.bits; 2: rows a.list[i0 .. i1)
template <int V, int MODE>
__global__ __launch_bounds__(kProfileBlock) void profile_count_kernel(ProfileCountArgs a, u64 i0, u64 i1, uint32_t slice, uint32_t upr, uint32_t R)
{
    __shared__ uint32_t cnt[kProfMaxBits + 1]; // the workgroup's rows per column (< 2^32: a table has fewer rows), then its rows counted
    const uint32_t tid = threadIdx.x;
    const uint32_t nbits = a.W * 32u;
    for (uint32_t k = tid; k <= nbits; k += kProfileBlock) cnt[k] = 0;
    __syncthreads();
    const uint32_t r = tid / upr, p = tid - r * upr; // row lane, position; r >= R: nothing to do
    const u64 step_rows = 8ull * R;
    const uint32_t* col = a.rows + static_cast<size_t>(p) * V;
    uint32_t nsel = 0;
    for (u64 b0 = i0 + static_cast<u64>(blockIdx.x) * slice; r < R && b0 < i1; b0 += static_cast<u64>(gridDim.x) * slice) {
        const u64 b1 = b0 + slice < i1 ? b0 + slice : i1;
        uint32_t c[V][kProfPlanes];
#pragma unroll
        for (int v = 0; v < V; v++)
#pragma unroll
            for (int j = 0; j < kProfPlanes; j++) c[v][j] = 0;
        for (u64 sb = b0; sb < b1; sb += step_rows) {
            const bool tail = sb + step_rows > b1; // (the same for the whole workgroup)
            uint32_t x[8][V];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                u64 idx = sb + r + static_cast<u64>(j) * R;
                bool ok = true;
                if (tail) {
                    ok = idx < b1;
                    idx = ok ? idx : b1 - 1;
                }
                u64 row = idx;
                if (MODE == 2) row = a.list[idx];
                if (MODE == 1) ok = ok && ((a.bits[row >> 5] >> (row & 31u)) & 1u);
                prof_load<V>(col + row * a.W, x[j]);
                if (MODE == 1 || tail) {
                    const uint32_t m = ok ? 0xFFFFFFFFu : 0u;
#pragma unroll
                    for (int v = 0; v < V; v++) x[j][v] &= m;
                }
                nsel += ok ? 1u : 0u;
            }
#pragma unroll
            for (int v = 0; v < V; v++) prof_add8(c[v], x[0][v], x[1][v], x[2][v], x[3][v], x[4][v], x[5][v], x[6][v], x[7][v]);
        }
        // unpack: only the planes a thread of this slice can have reached
        const uint32_t most = static_cast<uint32_t>((static_cast<u64>(slice) + step_rows - 1) / step_rows) * 8u;
        const int np = 32 - __clz(static_cast<int>(most));
#pragma unroll
        for (int v = 0; v < V; v++) {
            for (uint32_t b = 0; b < 32; b++) {
                const uint32_t bb = (b + p) & 31u; // (a wave's positions are consecutive: 32 lanes, 32 different LDS banks)
                uint32_t val = 0;
#pragma unroll
                for (int j = 0; j < kProfPlanes; j++)
                    if (j < np) val |= ((c[v][j] >> bb) & 1u) << j;
                if (val) atomicAdd(&cnt[(p * V + v) * 32u + bb], val);
            }
        }
    }
    if (p == 0 && nsel) atomicAdd(&cnt[nbits], nsel);
    __syncthreads();
    uint32_t* mine = a.partial + static_cast<size_t>(blockIdx.x) * (nbits + 1u);
    for (uint32_t k = tid; k <= nbits; k += kProfileBlock) mine[k] = cnt[k];
}

// counts[k] += the sum of column k of the nblocks x ncols partials: 64 columns (blockIdx.x) x a share of the rows (blockIdx.y) to a
// workgroup, its four waves a quarter of that share each; one 64-bit atomic add per column and workgroup
__global__ __launch_bounds__(kProfileBlock) void profile_reduce_kernel(const uint32_t* partial, uint32_t nblocks, uint32_t ncols, unsigned long long* counts)
{
    __shared__ unsigned long long part[kProfileBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = blockIdx.x * 64u + (tid & 63u);
    unsigned long long sum = 0;
    if (k < ncols)
        for (uint32_t g = blockIdx.y * 4u + (tid >> 6); g < nblocks; g += gridDim.y * 4u) sum += partial[static_cast<size_t>(g) * ncols + k];
    part[tid] = sum;
    __syncthreads();
    if (tid < 64 && k < ncols) {
        const unsigned long long total = part[tid] + part[tid + 64] + part[tid + 128] + part[tid + 192];
        if (total) atomicAdd(&counts[k], total);
    }
}

__global__ void profile_list_range_kernel(const uint32_t* list, uint32_t n, u64 r0, u64 r1, uint32_t* range)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int which = 0; which < 2; which++) {
        const u64 key = which ? r1 : r0;
        uint32_t lo = 0, hi = n; // the first entry >= key
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (list[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        range[which] = lo;
    }
}

// ---- weighted popcounts, VALU: NP planes (a multiple of 8 >= a.nplanes; the planes from a.nplanes on are zero), WPL words per lane ----
template <int NP, int WPL>
__global__ __launch_bounds__(kProfileBlock) void profile_overlap_valu_kernel(ProfileOverlapArgs a, u64 r0, u64 r1, uint32_t lg)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t G = 1u << lg;
    const uint32_t g = tid & (G - 1u);
    const uint32_t rows_per_block = kProfileBlock >> lg;
    uint32_t pl[WPL][NP];
    uint32_t wi[WPL], wm[WPL];
#pragma unroll
    for (int m = 0; m < WPL; m++) {
        const uint32_t w = g + static_cast<uint32_t>(m) * G;
        wm[m] = w < a.W ? 0xFFFFFFFFu : 0u;
        wi[m] = w < a.W ? w : a.W - 1u;
#pragma unroll
        for (int b = 0; b < NP; b++) pl[m][b] = a.planes[static_cast<size_t>(b) * a.W + wi[m]] & wm[m];
    }
    // four rows of a lane in flight (one row at a time the kernel waits for a 4-byte load per lane and row: 0.7 TB/s at 1024 bits)
    const u64 stride = static_cast<u64>(gridDim.x) * rows_per_block;
    for (u64 row0 = r0 + static_cast<u64>(blockIdx.x) * rows_per_block + (tid >> lg); row0 < r1; row0 += 4u * stride) {
        uint32_t x[4][WPL];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 row = row0 + static_cast<u64>(j) * stride;
            const uint32_t* src = a.rows + (row < r1 ? row : r1 - 1) * a.W; // (past the range: the last row again, nothing stored)
#pragma unroll
            for (int m = 0; m < WPL; m++) x[j][m] = __builtin_nontemporal_load(src + wi[m]) & wm[m];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 row = row0 + static_cast<u64>(j) * stride;
            uint32_t pc = 0;
#pragma unroll
            for (int m = 0; m < WPL; m++) pc += __popc(x[j][m]);
            // the planes 0 .. 15 and 16 .. 31 apart, in 32 bits each: a row's counts are at most 4096 (< 2^13, << 15: < 2^32)
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int b = 0; b < NP; b++) {
                uint32_t n = 0;
#pragma unroll
                for (int m = 0; m < WPL; m++) n += __popc(x[j][m] & pl[m][b]);
                if (b < 16) lo += n << b;
                else hi += n << (b - 16);
            }
            // the G lanes of a row share row0: every partner is active
            for (uint32_t off = G >> 1; off; off >>= 1) {
                lo += __shfl_xor(lo, static_cast<int>(off));
                hi += __shfl_xor(hi, static_cast<int>(off));
                pc += __shfl_xor(pc, static_cast<int>(off));
            }
            if (g == 0 && row < r1) {
                a.sums[row - a.out0] = static_cast<u64>(lo) + (static_cast<u64>(hi) << 16);
                if (a.popc) a.popc[row - a.out0] = pc;
            }
        }
    }
}

// ---- weighted popcounts on the matrix cores: rows of whole 256-bit groups ----
constexpr uint32_t kProfMaxChunks = kProfMaxBits / 128; // 16-byte chunks of the widest row

__global__ __launch_bounds__(kProfileBlock) void profile_overlap_mfma_kernel(ProfileOverlapArgs a, u64 r0, u64 r1)
{
    // plane b's chunk c at [b * (CPR + 1) + c]: the odd stride makes the lanes' 16-byte fragment reads conflict-free
    __shared__ u32x4 planes[32 * (kProfMaxChunks + 1)];
    const uint32_t tid = threadIdx.x;
    const uint32_t CPR = a.W / 4u, LS = CPR + 1u;
    for (uint32_t idx = tid; idx < 32u * CPR; idx += kProfileBlock) {
        const uint32_t b = idx / CPR, c = idx - b * CPR;
        planes[b * LS + c] = reinterpret_cast<const u32x4*>(a.planes)[idx];
    }
    __syncthreads();
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t i = lane & 31u, h = lane >> 5;
    ClassMasks km{0x11111111u, 0x22222222u, 0x44444444u};
    asm volatile("" : "+v"(km.m1), "+v"(km.m2), "+v"(km.m4)); // keep them in VGPRs
    const u64 ntiles = (r1 - r0 + 31u) / 32u;
    const u32x4* aline = planes + i * LS + h;
    for (u64 t = static_cast<u64>(blockIdx.x) * 4u + wave; t < ntiles; t += static_cast<u64>(gridDim.x) * 4u) { // (the same for a whole wave)
        const u64 row = r0 + t * 32u + i;
        const bool live = row < r1;
        const u32x4* src = reinterpret_cast<const u32x4*>(a.rows) + (live ? row : r1 - 1) * CPR + h; // (a tile's last rows: nothing past the range is read)
        v16f acc = v16f{}, acc2 = v16f{}; // (two chains: an MFMA never waits for the one just issued)
        uint32_t pc = 0;
        for (uint32_t g = 0; g < CPR / 2u; g++) { // one 256-bit group: lane half h holds its chunk 2 g + h
            const u32x4 xb = src[2u * g];
            const u32x4 xa = aline[2u * g];
            pc += __popc(xb.x) + __popc(xb.y) + __popc(xb.z) + __popc(xb.w);
            acc = mfma_class<0>(fp4_class<0>(xa, km), fp4_class<0>(xb, km), acc);
            acc = mfma_class<1>(fp4_class<1>(xa, km), fp4_class<1>(xb, km), acc);
            acc2 = mfma_class<2>(fp4_class<2>(xa, km), fp4_class<2>(xb, km), acc2);
            acc2 = mfma_class<3>(fp4_class<3>(xa, km), fp4_class<3>(xb, km), acc2);
        }
        // register r of lane (i, h): |row i AND plane (r & 3) + 8 (r >> 2) + 4 h|
        u64 s = 0;
#pragma unroll
        for (int r = 0; r < 16; r++)
            s += static_cast<u64>(static_cast<uint32_t>(acc[r]) + static_cast<uint32_t>(acc2[r])) << ((r & 3) + 8 * (r >> 2) + 4 * static_cast<int>(h));
        s += __shfl_xor(s, 32);
        pc += __shfl_xor(pc, 32);
        if (live && h == 0) {
            a.sums[row - a.out0] = s;
            if (a.popc) a.popc[row - a.out0] = pc;
        }
    }
}

template <int V, int MODE>
void count_launch(const ProfileCountArgs& a, u64 i0, u64 i1, uint32_t grid, uint32_t slice, uint32_t upr, uint32_t R, hipStream_t s)
{
    hipLaunchKernelGGL((profile_count_kernel<V, MODE>), dim3(grid), dim3(kProfileBlock), 0, s, a, i0, i1, slice, upr, R);
    const uint32_t ncols = a.W * 32u + 1u;
    hipLaunchKernelGGL(profile_reduce_kernel, dim3((ncols + 63u) / 64u, std::min((grid + 31u) / 32u, 32u)), dim3(kProfileBlock), 0, s, a.partial, grid, ncols,
                       a.counts);
}

template <int NP> void overlap_valu_launch(const ProfileOverlapArgs& a, u64 r0, u64 r1, uint32_t grid, uint32_t lg, bool two, hipStream_t s)
{
    if (two) hipLaunchKernelGGL((profile_overlap_valu_kernel<NP, 2>), dim3(grid), dim3(kProfileBlock), 0, s, a, r0, r1, lg);
    else hipLaunchKernelGGL((profile_overlap_valu_kernel<NP, 1>), dim3(grid), dim3(kProfileBlock), 0, s, a, r0, r1, lg);
}

} // namespace

hipError_t launch_profile_count(const ProfileCountArgs& a, uint64_t i0, uint64_t i1, int num_cus, hipStream_t s)
{
    if (i0 >= i1) return hipSuccess;
    if (a.W == 0 || a.W * 32u > kProfMaxBits || (a.bits && a.list) || !a.rows || !a.counts || !a.partial) return hipErrorInvalidValue;
    const int V = a.W % 4u == 0 ? 4 : 1;
    const uint32_t upr = a.W / static_cast<uint32_t>(V);  // positions per row: at most 32 chunks, or 127 words
    const uint32_t R = kProfileBlock / upr;               // row lanes of a workgroup: at least 2
    const uint64_t n = i1 - i0, step = 8ull * R;
    // The grid: the workgroups the device holds at once (four per CU at this kernel's registers), each with an equal share of the
    // range cut into k equal slices of whole steps -- as few as keep a thread's rows per slice within kProfileSliceIters, far
    // below what its planes hold -- so that a slice's unpacking is a small part of its adds and no workgroup gets a slice more.
    const uint64_t most = profile_count_blocks(num_cus);
    const uint64_t share = (n + most - 1) / most;
    const uint64_t k = (share + static_cast<uint64_t>(kProfileSliceIters) * R - 1) / (static_cast<uint64_t>(kProfileSliceIters) * R);
    const uint64_t slice = std::max<uint64_t>(((share + k - 1) / k + step - 1) / step * step, step);
    const uint64_t grid = std::min((n + slice - 1) / slice, most);
    static_assert(kProfileSliceIters % 8 == 0 && kProfileSliceIters <= kProfileMaxIters, "a slice never overflows a thread's planes");
    const uint32_t gr = static_cast<uint32_t>(grid), sl = static_cast<uint32_t>(slice);
    const int mode = a.list ? 2 : a.bits ? 1 : 0;
    if (V == 4) {
        if (mode == 0) count_launch<4, 0>(a, i0, i1, gr, sl, upr, R, s);
        else if (mode == 1) count_launch<4, 1>(a, i0, i1, gr, sl, upr, R, s);
        else count_launch<4, 2>(a, i0, i1, gr, sl, upr, R, s);
    } else {
        if (mode == 0) count_launch<1, 0>(a, i0, i1, gr, sl, upr, R, s);
        else if (mode == 1) count_launch<1, 1>(a, i0, i1, gr, sl, upr, R, s);
        else count_launch<1, 2>(a, i0, i1, gr, sl, upr, R, s);
    }
    return hipGetLastError();
}

uint32_t profile_count_blocks(int num_cus) { return 4u * static_cast<uint32_t>(std::max(num_cus, 1)); }

hipError_t launch_profile_list_range(const uint32_t* list, uint32_t n, uint64_t r0, uint64_t r1, uint32_t* range, hipStream_t s)
{
    hipLaunchKernelGGL(profile_list_range_kernel, dim3(1), dim3(64), 0, s, list, n, r0, r1, range);
    return hipGetLastError();
}

bool profile_overlap_matrix(uint32_t W) { return W != 0 && W % 8u == 0 && W * 32u <= kProfMaxBits; }

hipError_t launch_profile_overlap(const ProfileOverlapArgs& a, uint64_t r0, uint64_t r1, bool matrix, int num_cus, hipStream_t s)
{
    if (r0 >= r1) return hipSuccess;
    if (a.W == 0 || a.W * 32u > kProfMaxBits || a.nplanes < 1 || a.nplanes > 32 || r0 < a.out0 || !a.rows || !a.planes || !a.sums)
        return hipErrorInvalidValue;
    const uint64_t n = r1 - r0;
    const uint64_t most = 8ull * static_cast<uint64_t>(std::max(num_cus, 1)); // (measured: 8 per CU 3.5 ms, 4 per CU 4.6 ms at 100 M x 1024 bits)
    if (matrix) {
        if (!profile_overlap_matrix(a.W)) return hipErrorInvalidValue;
        const uint64_t blocks = ((n + 31) / 32 + 3) / 4; // four waves, a tile of 32 rows each
        hipLaunchKernelGGL(profile_overlap_mfma_kernel, dim3(static_cast<uint32_t>(std::min(blocks, most))), dim3(kProfileBlock), 0, s, a, r0, r1);
        return hipGetLastError();
    }
    uint32_t lg = 0;
    while ((1u << lg) < a.W && lg < 6) lg++; // G = min(64, the next power of two >= W) lanes per row
    const bool two = a.W > (1u << lg);       // (W <= 128: at most two words per lane)
    const uint64_t rows_per_block = kProfileBlock >> lg;
    const uint32_t grid = static_cast<uint32_t>(std::min((n + rows_per_block - 1) / rows_per_block, most));
    if (a.nplanes <= 8) overlap_valu_launch<8>(a, r0, r1, grid, lg, two, s);
    else if (a.nplanes <= 16) overlap_valu_launch<16>(a, r0, r1, grid, lg, two, s);
    else if (a.nplanes <= 24) overlap_valu_launch<24>(a, r0, r1, grid, lg, two, s);
    else overlap_valu_launch<32>(a, r0, r1, grid, lg, two, s);
    return hipGetLastError();
}

} // namespace gsim
