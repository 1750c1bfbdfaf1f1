// gsim_forest.h -- the device half of the lock-free union-find forest that comp_tile_kernel (gsim_components.hip) and
// dbscan_link_kernel (gsim_dbscan.hip) feed: the load, the unite and the wave's smallest value.  The protocol -- what may be
// written where, why stale values are harmless and why every loop terminates -- is the head comment of gsim_components.hip; the
// numbers below are its invariants.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include "gsim_device_common.h"

namespace gsim
{
namespace
{

__device__ __forceinline__ uint32_t parent_load(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Unites the components of a and b (members of them) in one forest; returns the root both belong to afterwards as this lane saw
// it.  Invariants 2 to 5 of gsim_components.hip's head comment.
__device__ __forceinline__ uint32_t comp_unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t& hooks, uint32_t& lost)
{
    for (;;) {
        if (a == b) return a;
        if (a < b) {
            const uint32_t x = a;
            a = b;
            b = x;
        }
        // a > b: climb from a
        const uint32_t pa = parent_load(parent + a);
        if (pa != a) {
            a = pa;
            continue;
        }
        const uint32_t pb = parent_load(parent + b);
        if (pb != b) {
            b = pb;
            continue;
        }
        const uint32_t old = atomicCAS(parent + a, a, b);
        if (old == a) {
            hooks++;
            return b;
        }
        lost++;
        a = old;
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t y = static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), off, 64));
        x = y < x ? y : x;
    }
    return x;
}

} // namespace
} // namespace gsim
