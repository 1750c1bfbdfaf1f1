// gsim_labels.hip -- the column counts of every label in one pass (gsim_db_label_counts, the count step of gsim_db_kmeans) and
// the changed-label count of the k-means loop.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 21 has the route,
// the budget and the measurements.
//
//   1. keys = min(label, nlabels), values = row numbers, one stable radix sort over the bits nlabels needs (rocprim): the rows of a
//      label become one contiguous, ascending segment of the list; GSIM_LABEL_NONE sorts behind every label and is never visited.
//      The segments' starts are a binary search per label (labels_bounds_kernel): sizes[l] = first[l + 1] - first[l].
//   2. The counting kernel walks the sorted list.  A thread keeps ONE position of the row -- a 16-byte chunk (rows of a multiple
//      of four words) or a single word -- the kLabelsBlock threads are R row lanes x the positions, four rows of a lane in flight:
//      a STEP is 4 R consecutive list entries.  The list is sorted, so a step holds one label exactly when its first and last
//      keys are equal, which every thread reads from the same two addresses (workgroup-uniform, no vote):
//        * a one-label step adds its set bits into the workgroup's LDS counters (one per column).  They are flushed -- the non-zero
//          ones, 32-bit atomic adds into that label's row of the global counters -- only when a one-label step of ANOTHER label
//          arrives or the workgroup ends: a long segment costs fp_bits global adds per workgroup, not per step;
//        * a step that holds several labels (segments shorter than a step, or a boundary) never touches LDS: every lane adds the
//          set bits of its row straight into the row's own label's global counters.  10^6 clusters of 5 rows are steps of this
//          kind only: no counter is zeroed or flushed for them, the cost is one global add per set bit.
//      Loads are never skipped under a lane's condition: the index is clamped and the value masked.
//      Integer adds commute: the counters do not depend on the grid, the slices, the launches or on which of the two ways a row went.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"

namespace gsim
{
namespace
{

constexpr uint32_t kLabelsMaxBits = 4096;
constexpr int kLabelsInFlight = 4; // rows of a row lane per step

__global__ __launch_bounds__(kLabelsBlock) void labels_keys_kernel(const uint32_t* labels, u64 n, uint32_t nlabels, uint32_t row0, uint32_t* keys,
                                                                    uint32_t* vals)
{
    const u64 i = static_cast<u64>(blockIdx.x) * kLabelsBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = labels[i];
    keys[i] = l < nlabels ? l : nlabels;
    vals[i] = row0 + static_cast<uint32_t>(i);
}

__global__ __launch_bounds__(kLabelsBlock) void labels_bounds_kernel(const uint32_t* keys, u64 n, uint32_t nlabels, uint32_t* first)
{
    const u64 l = static_cast<u64>(blockIdx.x) * kLabelsBlock + threadIdx.x;
    if (l > nlabels) return;
    u64 lo = 0, hi = n; // the first entry >= l
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (keys[mid] < l) lo = mid + 1;
        else hi = mid;
    }
    first[l] = static_cast<uint32_t>(lo);
}

template <int V> __device__ __forceinline__ void labels_load(const uint32_t* p, uint32_t (&x)[V])
{
    if constexpr (V == 4) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p);
        x[0] = v.x;
        x[1] = v.y;
        x[2] = v.z;
        x[3] = v.w;
    } else {
        x[0] = *p;
    }
}

template <int V> __global__ __launch_bounds__(kLabelsBlock) void labels_count_kernel(LabelCountArgs a, u64 i0, u64 i1, uint32_t upr, uint32_t R)
{
    __shared__ uint32_t cnt[kLabelsMaxBits];
    const uint32_t tid = threadIdx.x;
    const uint32_t nbits = a.W * 32u;
    for (uint32_t k = tid; k < nbits; k += kLabelsBlock) cnt[k] = 0;
    __syncthreads();
    const uint32_t r = tid / upr;
    const bool lane_on = r < R; // (the threads past the last whole row lane only take part in the flushes)
    const uint32_t rc = lane_on ? r : 0u, p = lane_on ? tid - r * upr : 0u;
    const uint32_t* col = a.rows + static_cast<size_t>(p) * V;
    const uint32_t col0 = p * V * 32u; // this thread's first column
    const u64 step = static_cast<u64>(kLabelsInFlight) * R;
    uint32_t cur = 0;   // the label whose counts the LDS counters hold (workgroup-uniform, as `dirty`)
    bool dirty = false;
    auto flush = [&]() {
        __syncthreads();
        uint32_t* dst = a.counts + static_cast<size_t>(cur) * nbits;
        for (uint32_t k = tid; k < nbits; k += kLabelsBlock) {
            const uint32_t v = cnt[k];
            if (v) {
                atomicAdd(&dst[k], v);
                cnt[k] = 0;
            }
        }
        __syncthreads();
        dirty = false;
    };
    for (u64 b0 = i0 + static_cast<u64>(blockIdx.x) * kLabelsSlice; b0 < i1; b0 += static_cast<u64>(gridDim.x) * kLabelsSlice) {
        const u64 b1 = b0 + kLabelsSlice < i1 ? b0 + kLabelsSlice : i1;
        for (u64 sb = b0; sb < b1; sb += step) {
            const u64 se = sb + step < b1 ? sb + step : b1;
            const uint32_t first = a.keys[sb], last = a.keys[se - 1]; // (the same two addresses for the whole workgroup)
            const bool one = first == last && first < a.nlabels;
            if (one && dirty && first != cur) flush();
            uint32_t x[kLabelsInFlight][V], lab[kLabelsInFlight];
#pragma unroll
            for (int j = 0; j < kLabelsInFlight; j++) {
                u64 idx = sb + rc + static_cast<u64>(j) * R;
                const bool ok = lane_on && idx < se;
                idx = ok ? idx : se - 1;
                lab[j] = a.keys[idx];
                labels_load<V>(col + static_cast<size_t>(a.list[idx]) * a.W, x[j]);
                const uint32_t m = ok && lab[j] < a.nlabels ? 0xFFFFFFFFu : 0u; // (no entry of a launch is GSIM_LABEL_NONE; nothing is added out of range if one were)
                lab[j] = lab[j] < a.nlabels ? lab[j] : 0u;
#pragma unroll
                for (int v = 0; v < V; v++) x[j][v] &= m;
            }
            if (one) {
                cur = first;
                dirty = true;
#pragma unroll
                for (int j = 0; j < kLabelsInFlight; j++)
#pragma unroll
                    for (int v = 0; v < V; v++)
                        for (uint32_t w = x[j][v]; w; w &= w - 1u) atomicAdd(&cnt[col0 + v * 32u + static_cast<uint32_t>(__ffs(static_cast<int>(w)) - 1)], 1u);
            } else {
#pragma unroll
                for (int j = 0; j < kLabelsInFlight; j++) {
                    uint32_t* dst = a.counts + static_cast<size_t>(lab[j]) * nbits + col0;
#pragma unroll
                    for (int v = 0; v < V; v++)
                        for (uint32_t w = x[j][v]; w; w &= w - 1u) atomicAdd(&dst[v * 32u + static_cast<uint32_t>(__ffs(static_cast<int>(w)) - 1)], 1u);
                }
            }
        }
    }
    if (dirty) flush();
}

__global__ __launch_bounds__(kLabelsBlock) void labels_changed_kernel(const uint32_t* a, const uint32_t* b, u64 n, unsigned long long* changed)
{
    uint32_t mine = 0;
    for (u64 i = static_cast<u64>(blockIdx.x) * kLabelsBlock + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * kLabelsBlock) mine += a[i] != b[i] ? 1u : 0u;
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(changed, static_cast<unsigned long long>(mine));
}

uint32_t labels_end_bit(uint32_t nlabels)
{
    uint32_t bits = 1;
    while (bits < 32 && (nlabels >> bits)) bits++;
    return bits; // keys are 0 .. nlabels
}

} // namespace

hipError_t launch_labels_keys(const uint32_t* labels, uint64_t n, uint32_t nlabels, uint32_t row0, uint32_t* keys, uint32_t* vals, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(labels_keys_kernel, dim3(static_cast<uint32_t>((n + kLabelsBlock - 1) / kLabelsBlock)), dim3(kLabelsBlock), 0, s, labels, n, nlabels,
                       row0, keys, vals);
    return hipGetLastError();
}

hipError_t labels_sort_bytes(uint64_t n, uint32_t nlabels, size_t* bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                     static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<size_t>(n), 0u,
                                     labels_end_bit(nlabels));
}

hipError_t launch_labels_sort(void* tmp, size_t tmp_bytes, const uint32_t* keys, uint32_t* keys_sorted, const uint32_t* vals, uint32_t* vals_sorted,
                              uint64_t n, uint32_t nlabels, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    size_t bytes = tmp_bytes;
    return rocprim::radix_sort_pairs(tmp, bytes, keys, keys_sorted, vals, vals_sorted, static_cast<size_t>(n), 0u, labels_end_bit(nlabels), s);
}

hipError_t launch_labels_bounds(const uint32_t* keys_sorted, uint64_t n, uint32_t nlabels, uint32_t* first, hipStream_t s)
{
    const u64 threads = static_cast<u64>(nlabels) + 1;
    hipLaunchKernelGGL(labels_bounds_kernel, dim3(static_cast<uint32_t>((threads + kLabelsBlock - 1) / kLabelsBlock)), dim3(kLabelsBlock), 0, s, keys_sorted, n,
                       nlabels, first);
    return hipGetLastError();
}

hipError_t launch_labels_count(const LabelCountArgs& a, uint64_t i0, uint64_t i1, int num_cus, hipStream_t s)
{
    if (i0 >= i1) return hipSuccess;
    if (a.W == 0 || a.W * 32u > kLabelsMaxBits || !a.rows || !a.keys || !a.list || !a.counts || a.nlabels == 0) return hipErrorInvalidValue;
    const int V = a.W % 4u == 0 ? 4 : 1;
    const uint32_t upr = a.W / static_cast<uint32_t>(V); // positions per row: at most 32 chunks, or 127 words
    const uint32_t R = kLabelsBlock / upr;               // row lanes of a workgroup: at least 2
    const uint64_t slices = (i1 - i0 + kLabelsSlice - 1) / kLabelsSlice;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(slices, 8ull * static_cast<uint64_t>(std::max(num_cus, 1))));
    if (V == 4) hipLaunchKernelGGL(labels_count_kernel<4>, dim3(grid), dim3(kLabelsBlock), 0, s, a, i0, i1, upr, R);
    else hipLaunchKernelGGL(labels_count_kernel<1>, dim3(grid), dim3(kLabelsBlock), 0, s, a, i0, i1, upr, R);
    return hipGetLastError();
}

hipError_t launch_labels_changed(const uint32_t* a, const uint32_t* b, uint64_t n, unsigned long long* changed, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((n + kLabelsBlock - 1) / kLabelsBlock, 4096));
    hipLaunchKernelGGL(labels_changed_kernel, dim3(grid), dim3(kLabelsBlock), 0, s, a, b, n, changed);
    return hipGetLastError();
}

} // namespace gsim
