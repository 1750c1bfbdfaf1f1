// gsim_linkage.hip -- the device side of gsim_db_linkage: complete- and average-linkage dendrograms of up to 65 536 rows on the
// dense similarity matrix, by the nearest-neighbour chain.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 31.
//
//   link_mirror_kernel   the matrix as the chain reads it, from the matrix-core pass's scores (gsim_scores.hip): symmetric, so that
//                        the row of a slot holds its similarity to every other slot.  Only s(i, j) with i < j is read -- the rule's
//                        "lower row on the left" -- and written to both [i][j] and [j][i], the transposed half through an LDS tile so
//                        that both stores run along rows.  Complete linkage keeps the f32 scores (in place), average linkage widens
//                        q(s) = (uint32) floor(s * 2^31) into 64-bit sums, slab by slab.
//   link_chain_kernel    ONE workgroup of 1024 threads.  A step scans the row of the chain's tip X for the live slot Y first in
//                        (similarity descending, Y ascending): 16-byte loads, four in flight per thread, an argmax per wave by
//                        shuffles and across the 16 waves through LDS.  Y is pushed, or -- when it is the element below the tip --
//                        merged with it: the lower slot a gets min(row a, row b) or row a + row b, along its row (vector stores) and
//                        down its column (one store per live slot), and b dies.  The chain, the sizes (0 = dead) and the raw merges
//                        live in device memory; a launch runs at most `steps` steps and writes its counters back, the host relaunches.
//                        Nothing in it waits on another workgroup: there is none.  Every loop is bounded by `steps` or by ld / 4.
//                        All matrix offsets are 64-bit (8 x n^2 passes 4 GiB at n = 23 171).
//   Similarities of average linkage are the exact fractions Q / (|X| |Y|); for a fixed X they are compared as Q_y |Z| against Q_z |Y|
//   in 96 bits (Q < 2^63 + 1, sizes <= 2^16).
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"

namespace gsim
{

namespace
{

__global__ __launch_bounds__(256) void link_init_kernel(LinkArgs a)
{
    const u64 z = static_cast<u64>(blockIdx.x) * 256 + threadIdx.x;
    if (z < a.ld) a.size[z] = z < a.n ? 1u : 0u;
    if (z < kLinkCtlWords) a.ctl[z] = 0;
}

template <bool kAvg> __global__ __launch_bounds__(256) void link_mirror_kernel(LinkArgs a, const float* in, u64 ld_in, u64 col0, u64 first, u64 rows)
{
    __shared__ float tile[kLinkTile][kLinkTile + 1];
    const u64 i0 = first + static_cast<u64>(blockIdx.y) * kLinkTile, j0 = static_cast<u64>(blockIdx.x) * kLinkTile;
    if (j0 < i0) return; // (below the diagonal: whole workgroups, ahead of the barrier)
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const u64 n = a.n, i_end = first + rows < n ? first + rows : n;
    using T = typename std::conditional<kAvg, u64, float>::type;
    T* mat = static_cast<T*>(a.mat);
    for (uint32_t r = ty; r < kLinkTile; r += 8) {
        const u64 i = i0 + r, j = j0 + tx;
        tile[r][tx] = i < i_end && j < n ? in[(i - first) * ld_in + (j - col0)] : 0.0f; // (j >= j0 >= i0 >= first >= col0)
    }
    __syncthreads();
    for (uint32_t r = ty; r < kLinkTile; r += 8) {
        // the upper half as it is (complete linkage has it already) ...
        const u64 i = i0 + r, j = j0 + tx;
        if constexpr (kAvg) {
            if (i < i_end && j < n && j >= i) mat[i * a.ld + j] = j > i ? static_cast<u64>(__float2uint_rz(tile[r][tx] * 2147483648.0f)) : 0;
        }
        // ... and transposed: row j0 + r, column i0 + tx
        const u64 jt = j0 + r, it = i0 + tx;
        if (it < i_end && jt < n && jt > it) {
            const float s = tile[tx][r];
            if constexpr (kAvg) mat[jt * a.ld + it] = static_cast<u64>(__float2uint_rz(s * 2147483648.0f));
            else mat[jt * a.ld + it] = s;
        }
    }
}

struct LinkCand {
    u64 v;
    uint32_t size, idx;
};

// does x come before y for a fixed tip: the greater similarity, then the lower slot.  "Nothing yet" is {0, 1, 0xFFFFFFFF}.
template <bool kAvg> __device__ __forceinline__ bool link_before(const LinkCand& x, const LinkCand& y)
{
    if constexpr (kAvg) {
        // x.v / x.size against y.v / y.size: x.v * y.size against y.v * x.size, 96 bits each
        const u64 xl = x.v * y.size, xh = __umul64hi(x.v, static_cast<u64>(y.size));
        const u64 yl = y.v * x.size, yh = __umul64hi(y.v, static_cast<u64>(x.size));
        if (xh != yh) return xh > yh;
        if (xl != yl) return xl > yl;
    } else {
        if (x.v != y.v) return x.v > y.v;
    }
    return x.idx < y.idx;
}

__device__ __forceinline__ u64 link_shfl_xor(u64 v, int d)
{
    const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v)), d, 64));
    const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v >> 32)), d, 64));
    return (static_cast<u64>(hi) << 32) | lo;
}

// four consecutive entries of a row: one 16-byte load of floats, two of 64-bit sums
__device__ __forceinline__ void link_load4(const float* row, uint32_t g, u64 (&v)[4])
{
    const u32x4 w = reinterpret_cast<const u32x4*>(row)[g];
    v[0] = w.x;
    v[1] = w.y;
    v[2] = w.z;
    v[3] = w.w;
}
__device__ __forceinline__ void link_load4(const u64* row, uint32_t g, u64 (&v)[4])
{
    const ulonglong2 p = reinterpret_cast<const ulonglong2*>(row)[2 * static_cast<u64>(g)];
    const ulonglong2 q = reinterpret_cast<const ulonglong2*>(row)[2 * static_cast<u64>(g) + 1];
    v[0] = p.x;
    v[1] = p.y;
    v[2] = q.x;
    v[3] = q.y;
}
__device__ __forceinline__ void link_store4(float* row, uint32_t g, const u64 (&v)[4])
{
    u32x4 w;
    w.x = static_cast<uint32_t>(v[0]);
    w.y = static_cast<uint32_t>(v[1]);
    w.z = static_cast<uint32_t>(v[2]);
    w.w = static_cast<uint32_t>(v[3]);
    reinterpret_cast<u32x4*>(row)[g] = w;
}
__device__ __forceinline__ void link_store4(u64* row, uint32_t g, const u64 (&v)[4])
{
    reinterpret_cast<ulonglong2*>(row)[2 * static_cast<u64>(g)] = make_ulonglong2(v[0], v[1]);
    reinterpret_cast<ulonglong2*>(row)[2 * static_cast<u64>(g) + 1] = make_ulonglong2(v[2], v[3]);
}
__device__ __forceinline__ void link_store1(float* p, u64 v) { *p = __uint_as_float(static_cast<uint32_t>(v)); }
__device__ __forceinline__ void link_store1(u64* p, u64 v) { *p = v; }

constexpr int kLinkWaves = kLinkBlock / 64;
constexpr int kLinkUnroll = 4; // 16-byte groups a thread has in flight

template <bool kAvg> __global__ __launch_bounds__(kLinkBlock) void link_chain_kernel(LinkArgs a, uint32_t steps)
{
    using T = typename std::conditional<kAvg, u64, float>::type;
    __shared__ LinkCand sh_best[2][kLinkWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = a.n, ngroups = static_cast<uint32_t>(a.ld / 4);
    T* mat = static_cast<T*>(a.mat);
    const u32x4* size4 = reinterpret_cast<const u32x4*>(a.size);
    if (tid == 0) stamp_begin(a.ctl + kLinkCtlClk);

    // the carried state, the same in every thread
    uint32_t len = static_cast<uint32_t>(a.ctl[kLinkCtlLen]), merged = static_cast<uint32_t>(a.ctl[kLinkCtlMerged]);
    uint32_t chain_max = static_cast<uint32_t>(a.ctl[kLinkCtlChainMax]);
    u64 scans = a.ctl[kLinkCtlScans];
    bool failed = false;
    uint32_t tip = len >= 1 ? a.chain[len - 1] : 0, below = len >= 2 ? a.chain[len - 2] : 0;

    for (uint32_t step = 0; step < steps && merged + 1 < n; step++) {
        if (len == 0) {
            // the lowest live slot: a merged cluster keeps the lower slot, so slot 0 never dies
            tip = 0;
            len = 1;
            if (tid == 0) a.chain[0] = 0;
            if (chain_max < 1) chain_max = 1;
        }
        // ---- the scan of row `tip` ----
        const T* row = mat + static_cast<u64>(tip) * a.ld;
        LinkCand best{0, 1, 0xFFFFFFFFu};
        for (uint32_t g0 = tid; g0 < ngroups; g0 += kLinkUnroll * kLinkBlock) {
            u64 v[kLinkUnroll][4];
            u32x4 sz[kLinkUnroll];
#pragma unroll
            for (int u = 0; u < kLinkUnroll; u++) {
                const uint32_t g = g0 + u * kLinkBlock;
                sz[u] = u32x4{0, 0, 0, 0};
                v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0;
                if (g < ngroups) {
                    sz[u] = size4[g];
                    link_load4(row, g, v[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kLinkUnroll; u++) {
                const uint32_t y0 = (g0 + u * kLinkBlock) * 4;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const LinkCand cand{v[u][c], sz[u][c], y0 + c};
                    if (cand.size != 0 && cand.idx != tip && link_before<kAvg>(cand, best)) best = cand;
                }
            }
        }
        for (int d = 32; d > 0; d >>= 1) {
            LinkCand o;
            o.v = link_shfl_xor(best.v, d);
            o.size = static_cast<uint32_t>(__shfl_xor(static_cast<int>(best.size), d, 64));
            o.idx = static_cast<uint32_t>(__shfl_xor(static_cast<int>(best.idx), d, 64));
            if (link_before<kAvg>(o, best)) best = o;
        }
        // (two sets of slots: the waves that are still reading this step's are a barrier ahead of the step after the next one's stores)
        if (lane == 0) sh_best[step & 1][wave] = best;
        __syncthreads();
        best = sh_best[step & 1][0];
#pragma unroll
        for (int w = 1; w < kLinkWaves; w++) {
            const LinkCand o = sh_best[step & 1][w];
            if (link_before<kAvg>(o, best)) best = o;
        }
        scans++;
        const uint32_t y = best.idx; // (two live slots or more: there is one; the chain's elements are distinct live slots)
        if (y >= n || len >= n) { // never, while the state is what this kernel left: stop instead of following a wild index
            failed = true;
            break;
        }

        if (len >= 2 && y == below) {
            // ---- the merge of tip and below: slot lo takes both, slot hi dies ----
            const uint32_t lo = tip < below ? tip : below, hi = tip < below ? below : tip;
            T* row_lo = mat + static_cast<u64>(lo) * a.ld;
            const T* row_hi = mat + static_cast<u64>(hi) * a.ld;
            for (uint32_t g = tid; g < ngroups; g += kLinkBlock) {
                const u32x4 sz = size4[g];
                u64 x[4], w[4];
                link_load4(row_lo, g, x);
                link_load4(row_hi, g, w);
                bool any = false;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t z = g * 4 + c;
                    // (the bits of non-negative floats order as the floats do)
                    if (sz[c] != 0 && z != lo && z != hi) {
                        x[c] = kAvg ? x[c] + w[c] : (x[c] < w[c] ? x[c] : w[c]);
                        link_store1(mat + static_cast<u64>(z) * a.ld + lo, x[c]);
                        any = true;
                    }
                }
                if (any) link_store4(row_lo, g, x);
            }
            if (tid == 0) { // (the other threads skip slots lo and hi by their index, whatever their sizes say)
                const uint32_t size_lo = a.size[lo], size_hi = a.size[hi];
                a.raw[merged] = LinkRaw{lo, hi, size_lo, size_hi, best.v};
                a.size[lo] = size_lo + size_hi;
                a.size[hi] = 0;
            }
            merged++;
            len -= 2;
            __syncthreads(); // the row, the column and the sizes, ahead of the next scan
            tip = len >= 1 ? a.chain[len - 1] : 0;
            below = len >= 2 ? a.chain[len - 2] : 0;
        } else {
            if (tid == 0) a.chain[len] = y;
            below = tip;
            tip = y;
            len++;
            if (chain_max < len) chain_max = len;
        }
    }
    if (tid == 0) {
        a.ctl[kLinkCtlLen] = len;
        a.ctl[kLinkCtlMerged] = merged;
        a.ctl[kLinkCtlScans] = scans;
        a.ctl[kLinkCtlChainMax] = chain_max;
        a.ctl[kLinkCtlDone] = failed ? 2 : merged + 1 >= n ? 1 : 0;
        stamp_end(a.ctl + kLinkCtlClk);
    }
}

} // namespace

hipError_t launch_link_init(const LinkArgs& a, hipStream_t s)
{
    const u64 items = a.ld > kLinkCtlWords ? a.ld : kLinkCtlWords;
    hipLaunchKernelGGL(link_init_kernel, dim3(static_cast<uint32_t>((items + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_link_mirror(const LinkArgs& a, const float* in, uint64_t ld_in, uint64_t col0, uint64_t first, uint64_t rows, hipStream_t s)
{
    if (rows == 0 || a.n == 0) return hipSuccess;
    if (first % kLinkTile || first + rows > a.n || col0 > first || ld_in < a.n - col0 || a.ld < a.n) return hipErrorInvalidValue;
    if (!a.average && (in != static_cast<const float*>(a.mat) || col0 != 0 || first != 0 || rows != a.n || ld_in != a.ld)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<uint32_t>((a.n + kLinkTile - 1) / kLinkTile), static_cast<uint32_t>((rows + kLinkTile - 1) / kLinkTile));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (a.average) hipLaunchKernelGGL(link_mirror_kernel<true>, grid, dim3(256), 0, s, a, in, ld_in, col0, first, rows);
    else hipLaunchKernelGGL(link_mirror_kernel<false>, grid, dim3(256), 0, s, a, in, ld_in, col0, first, rows);
    return hipGetLastError();
}

hipError_t launch_link_chain(const LinkArgs& a, uint32_t steps, hipStream_t s)
{
    if (steps == 0 || a.n < 2 || a.ld % 4 || a.ld < a.n) return hipErrorInvalidValue;
    if (a.average) hipLaunchKernelGGL(link_chain_kernel<true>, dim3(1), dim3(kLinkBlock), 0, s, a, steps);
    else hipLaunchKernelGGL(link_chain_kernel<false>, dim3(1), dim3(kLinkBlock), 0, s, a, steps);
    return hipGetLastError();
}

} // namespace gsim
