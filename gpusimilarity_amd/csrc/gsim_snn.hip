// gsim_snn.hip -- shared-nearest-neighbour counts and Jarvis-Patrick links behind gsim_db_snn and gsim_db_jarvis_patrick: the pass
// between the k-NN fold (gsim_knn.hip leaves N lists of k slots in device memory) and the forests of gsim_components.hip.  The rule
// is stated in include/gpusim_hip.h.
//
// LANE GROUPS.  A list has at most k <= 128 rows, and both kernels give every lane of a group two slots of one list: a group is G =
// 16 lanes for k <= 32, 32 lanes for k <= 64, the whole wave for k <= 128 -- so a wave works on 4, 2 or 1 lists at a time and k = 8
// idles half of its lanes, not 7 of 8.  A lane's slots are l and l + G (l its index in the group): every list access is one
// coalesced run of the group's lanes.
//
// snn_sort_kernel<G>: list i's row ids, ascending, into nbr[i * k .. i * k + k), padded with 0xFFFFFFFF (no row: a table has fewer
// than 2^32 - 1 rows).  A bitonic network over the group's 2 G slots, in registers: the exchange at distance G is inside a lane, every
// other one is a __shfl_xor within the group.  No LDS, no indexed arrays.
//
// snn_link_kernel<G>: a group takes one owner row i at a time (the workgroup's 4 waves step through the owners together, grid-stride),
// puts nbr(i) into its 2 G words of LDS, and walks list i in list order.  For the entry j it loads nbr(j) -- k consecutive words, at
// most 512 bytes; the next entry's load is issued before this entry's search --, and each lane looks its two rows up in the LDS copy
// by a branch-free binary search (log2(2 G) = 5 to 7 ds_read_b32, the first ones broadcasts).  A ballot over the group and a popcount
// give |L(i) & L(j)|; a ballot on "== i" gives mutual.  The count goes to the lane whose slot the entry has and is stored with the
// list's other counts in one run (gsim_db_snn); for the clustering lane l of the group is level l: where the entry is a link of its
// level it calls comp_unite (gsim_forest.h: the only write to the forests; the flatten kernel follows the launch).  A mutual pair is
// met from both sides; the second unite finds one root and writes nothing.  The counters are summed in registers and added once per
// wave and counter.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_forest.h"

namespace gsim
{
namespace
{

constexpr uint32_t kSnnPad = 0xFFFFFFFFu;
constexpr int kSnnBlock = 256;

__device__ __forceinline__ uint32_t shfl_xor_u32(uint32_t v, int mask)
{
    return static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), mask, 64));
}

// The 2 G values of a group (lane l: x0 at slot l, x1 at slot l + G) into ascending slot order.
template <int G> __device__ __forceinline__ void group_sort(uint32_t& x0, uint32_t& x1, uint32_t l)
{
#pragma unroll
    for (uint32_t size = 2; size <= 2u * G; size <<= 1) {
#pragma unroll
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride == static_cast<uint32_t>(G)) { // (size == 2 G: the last merge, ascending everywhere)
                const uint32_t lo = x0 < x1 ? x0 : x1, hi = x0 < x1 ? x1 : x0;
                x0 = lo;
                x1 = hi;
            } else {
                const uint32_t p0 = shfl_xor_u32(x0, static_cast<int>(stride)), p1 = shfl_xor_u32(x1, static_cast<int>(stride));
                const bool lower = (l & stride) == 0;
                const bool up0 = (l & size) == 0, up1 = ((l + G) & size) == 0;
                const uint32_t mn0 = x0 < p0 ? x0 : p0, mx0 = x0 < p0 ? p0 : x0;
                const uint32_t mn1 = x1 < p1 ? x1 : p1, mx1 = x1 < p1 ? p1 : x1;
                x0 = lower == up0 ? mn0 : mx0;
                x1 = lower == up1 ? mn1 : mx1;
            }
        }
    }
}

template <int G>
__global__ __launch_bounds__(kSnnBlock) void snn_sort_kernel(const KnnEntry* __restrict__ lists, const uint32_t* __restrict__ len, u64 nrows,
                                                             uint32_t k, uint32_t* __restrict__ nbr)
{
    const uint32_t l = threadIdx.x % G;
    const u64 o = static_cast<u64>(blockIdx.x) * (kSnnBlock / G) + threadIdx.x / G;
    const bool in = o < nrows;
    const uint32_t n = in ? len[o] : 0u;
    const u64 at = o * k;
    uint32_t x0 = l < n && l < k ? lists[at + l].row : kSnnPad;
    uint32_t x1 = l + G < n && l + G < k ? lists[at + l + G].row : kSnnPad;
    group_sort<G>(x0, x1, l); // (every lane of the wave takes part in the shuffles)
    if (in && l < k) nbr[at + l] = x0;
    if (in && l + G < k) nbr[at + l + G] = x1;
}

// y's place in the ascending 2 G words of s: is it there?
template <int G> __device__ __forceinline__ bool group_has(const uint32_t* s, uint32_t y)
{
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = G; step > 0; step >>= 1)
        if (s[pos + step - 1] < y) pos += step;
    return y != kSnnPad && s[pos] == y;
}

template <int G> __global__ __launch_bounds__(kSnnBlock) void snn_link_kernel(SnnArgs a)
{
    constexpr uint32_t GPW = 64 / G;              // groups (owners) per wave
    constexpr uint32_t PER_BLOCK = (kSnnBlock / 64) * GPW;
    __shared__ uint32_t s_nbr[(kSnnBlock / 64) * 128]; // 2 G words per group
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t l = lane % G, grp = lane / G;
    uint32_t* mine = s_nbr + wave * 128u + grp * (2u * G);
    const u64 gmask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull)) << (grp * G % 64);
    const uint32_t k = a.k;
    const bool closed = (a.flags & GSIM_SNN_CLOSED) != 0, either = (a.flags & GSIM_SNN_EITHER) != 0;
    // lane l of a group is level l of the clustering (no level: never a link)
    uint32_t my_kmin = kSnnPad;
#pragma unroll
    for (uint32_t t = 0; t < kCompMaxLevels; t++)
        if (a.parent && l == t && t < a.nlevels) my_kmin = a.kmins[t];
    uint32_t* forest = a.parent + static_cast<u64>(l < a.nlevels ? l : 0u) * a.nrows;

    uint32_t c_entries = 0, c_mutual = 0, c_links = 0, hooks = 0, lost = 0;
    for (u64 base = static_cast<u64>(blockIdx.x) * PER_BLOCK; base < a.nrows; base += static_cast<u64>(gridDim.x) * PER_BLOCK) {
        const u64 o = base + wave * GPW + grp;
        const bool in = o < a.nrows;
        const uint32_t n = in ? min(a.len[o], k) : 0u;
        const u64 at = o * k;
        __syncthreads(); // (the previous owner's searches are over)
        mine[l] = in && l < k ? a.nbr[at + l] : kSnnPad;
        mine[l + G] = in && l + G < k ? a.nbr[at + l + G] : kSnnPad;
        // the list in list order: the entry of slot l and of slot l + G
        const uint32_t j0 = l < n ? a.lists[at + l].row : 0u;
        const uint32_t j1 = l + G < n ? a.lists[at + l + G].row : 0u;
        __syncthreads();
        if (l == 0) c_entries += n;
        uint32_t r0 = 0, r1 = 0; // the counts of this lane's two entries
        // entry e of every group of the wave at once; y0, y1: this lane's two rows of nbr(j)
        uint32_t j = static_cast<uint32_t>(__shfl(static_cast<int>(j0), static_cast<int>(grp * G), 64));
        bool active = 0 < n && j < a.nrows;
        uint32_t y0 = active && l < k ? a.nbr[static_cast<u64>(j) * k + l] : kSnnPad;
        uint32_t y1 = active && l + G < k ? a.nbr[static_cast<u64>(j) * k + l + G] : kSnnPad;
        for (uint32_t e = 0; __ballot(e < n) != 0; e++) {
            // the next entry's rows, asked for before this entry's search
            const uint32_t e1 = e + 1;
            const uint32_t jn = static_cast<uint32_t>(__shfl(static_cast<int>(e1 < G ? j0 : j1), static_cast<int>(grp * G + (e1 & (G - 1u))), 64));
            const bool active_n = e1 < n && jn < a.nrows;
            const uint32_t n0 = active_n && l < k ? a.nbr[static_cast<u64>(jn) * k + l] : kSnnPad;
            const uint32_t n1 = active_n && l + G < k ? a.nbr[static_cast<u64>(jn) * k + l + G] : kSnnPad;

            const bool f0 = group_has<G>(mine, y0), f1 = group_has<G>(mine, y1);
            const uint32_t i32 = static_cast<uint32_t>(o);
            uint32_t cnt = static_cast<uint32_t>(__popcll(__ballot(f0) & gmask) + __popcll(__ballot(f1) & gmask));
            const bool mutual = (__ballot(active && (y0 == i32 || y1 == i32)) & gmask) != 0;
            if (closed) cnt += 1u + (mutual ? 1u : 0u);
            if (active) {
                if (l == (e & (G - 1u))) {
                    const uint32_t v = cnt | (mutual ? GSIM_SNN_MUTUAL_BIT : 0u);
                    if (e < G) r0 = v;
                    else r1 = v;
                }
                if (l == 0 && mutual) c_mutual++;
                if ((mutual || either) && cnt >= my_kmin) {
                    c_links++;
                    comp_unite(forest, i32, j, hooks, lost);
                }
            }
            j = jn;
            active = active_n;
            y0 = n0;
            y1 = n1;
        }
        if (a.shared) {
            if (l < n) a.shared[at + l] = r0;
            if (l + G < n) a.shared[at + l + G] = r1;
        }
    }
    // one atomic add per wave and counter (integer adds commute)
    if (__ballot((c_entries | c_mutual | c_links | hooks | lost) != 0) == 0) return;
    c_entries = wave_sum(c_entries);
    c_mutual = wave_sum(c_mutual);
    hooks = wave_sum(hooks);
    lost = wave_sum(lost);
#pragma unroll
    for (int d = G; d < 64; d <<= 1) c_links += shfl_xor_u32(c_links, d); // lane l < 8: level l's, over the wave's groups
    if (lane == 0) {
        if (c_entries) atomicAdd(a.counters + kSnnEntries, static_cast<u64>(c_entries));
        if (c_mutual) atomicAdd(a.counters + kSnnMutual, static_cast<u64>(c_mutual));
        if (hooks) atomicAdd(a.counters + kSnnUnions, static_cast<u64>(hooks));
        if (lost) atomicAdd(a.counters + kSnnCasFailed, static_cast<u64>(lost));
    }
    if (lane < kCompMaxLevels && c_links) atomicAdd(a.counters + kSnnLinks + lane, static_cast<u64>(c_links));
}

// count (owner, slot) of the lists' layout -> position indptr[owner] + slot (knn_compact_kernel's move, for the shared counts)
__global__ __launch_bounds__(256) void snn_compact_kernel(const uint32_t* __restrict__ shared, const uint32_t* __restrict__ len,
                                                          const u64* __restrict__ indptr, u64 nrows, uint32_t k, uint32_t* __restrict__ out)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    const u64 o = t / k;
    const uint32_t e = static_cast<uint32_t>(t % k);
    if (o >= nrows || e >= len[o]) return;
    out[indptr[o] + e] = shared[t];
}

// the lane group of a k: the smallest with 2 G >= k
template <class Fn> hipError_t dispatch_group(uint32_t k, Fn&& fn)
{
    if (k < 1 || k > GSIM_KNN_MAX_K) return hipErrorInvalidValue;
    if (k <= 32) return fn(std::integral_constant<int, 16>());
    if (k <= 64) return fn(std::integral_constant<int, 32>());
    return fn(std::integral_constant<int, 64>());
}

} // namespace

hipError_t launch_snn_sort(const KnnEntry* lists, const uint32_t* len, uint64_t nrows, uint32_t k, uint32_t* nbr, hipStream_t s)
{
    if (nrows == 0) return hipSuccess;
    return dispatch_group(k, [&](auto g) {
        constexpr int G = decltype(g)::value;
        const u64 blocks = (nrows + (kSnnBlock / G) - 1) / (kSnnBlock / G);
        hipLaunchKernelGGL(snn_sort_kernel<G>, dim3(static_cast<uint32_t>(blocks)), dim3(kSnnBlock), 0, s, lists, len, static_cast<u64>(nrows), k, nbr);
        return hipGetLastError();
    });
}

hipError_t launch_snn_link(const SnnArgs& a, int num_cus, hipStream_t s)
{
    if (a.nrows == 0) return hipSuccess;
    if (a.parent && (a.nlevels < 1 || a.nlevels > kCompMaxLevels)) return hipErrorInvalidValue;
    return dispatch_group(a.k, [&](auto g) {
        constexpr int G = decltype(g)::value;
        constexpr u64 per_block = (kSnnBlock / 64) * (64 / G);
        const u64 want = (a.nrows + per_block - 1) / per_block, cap = static_cast<u64>(num_cus > 0 ? num_cus : 1) * 8u;
        hipLaunchKernelGGL(snn_link_kernel<G>, dim3(static_cast<uint32_t>(want < cap ? want : cap)), dim3(kSnnBlock), 0, s, a);
        return hipGetLastError();
    });
}

hipError_t launch_snn_compact(const uint32_t* shared, const uint32_t* len, const uint64_t* indptr, uint64_t nrows, uint32_t k, uint32_t* out,
                              hipStream_t s)
{
    const u64 threads = nrows * k;
    if (threads == 0) return hipSuccess;
    hipLaunchKernelGGL(snn_compact_kernel, dim3(static_cast<uint32_t>((threads + 255) / 256)), dim3(256), 0, s, shared, len,
                       reinterpret_cast<const u64*>(indptr), static_cast<u64>(nrows), k, out);
    return hipGetLastError();
}

} // namespace gsim
