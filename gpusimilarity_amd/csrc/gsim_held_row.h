// gsim_held_row.h -- the held-row pair count of the tile kernels: nbr_tile_kernel (gsim_neighbors.hip, the joins included) and
// comp_tile_kernel (gsim_components.hip).  Internal.
//
//   * every lane HOLDS one whole zero-padded row of WP words in VGPRs (HeldRow) and knows its popcount;
//   * the OTHER side's row is wave-uniform: its words come through the scalar path and are the SGPR operand of v_and_b32, so a
//     word-pair costs v_and + the accumulating v_bcnt_u32_b32 (bcnt_acc), into four accumulators summed as
//     (acc0 + acc1) + (acc2 + acc3);
//   * the other side's popcounts (nbr_prepare_kernel) are fetched 64 at a time, one per lane, and handed out with v_readlane
//     (Handout64).
// What a kernel does with the count -- which pairs are valid, the band of gsim_prefilter.h, the one divide, what is kept and
// where -- is its own and stays in its file.
//
// The fold kernels (knn_fold_kernel, mst_fold_kernel, hist_tile_kernel) hold the same count written out: built on HeldRow they
// compile to the same instructions at other addresses and in other registers, and ran 0.3 to 1.9 % slower than before (the
// histogram's loop by its alignment alone: two s_nop in front of it gave the old time back).  They share what does not touch their
// loops: the typedef, readlane_u32 and dispatch_wp, the host-side dispatch over the six padded widths.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "gsim_device_common.h"

namespace gsim
{
namespace
{

typedef const __attribute__((address_space(4))) u32x4* const_u32x4p; // wave-uniform rows: read with s_load

__device__ __forceinline__ uint32_t readlane_u32(uint32_t v, uint32_t l)
{
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(l)));
}

template <int WP> struct HeldRow {
    u32x4 r4[WP / 4];

    // Row `row` of `rows` (WP words each) if `in`, else zero words: nothing to count there.  `row` is a row that exists either
    // way (the caller clamps it).  Returns the row's popcount.
    __device__ __forceinline__ uint32_t load(const void* rows, u64 row, bool in)
    {
        const u32x4* rp = reinterpret_cast<const u32x4*>(rows) + row * (WP / 4);
#pragma unroll
        for (int w = 0; w < WP / 4; w++) r4[w] = in ? rp[w] : u32x4{0, 0, 0, 0};
        uint32_t p = 0;
#pragma unroll
        for (int w = 0; w < WP / 4; w++) p += __popc(r4[w].x) + __popc(r4[w].y) + __popc(r4[w].z) + __popc(r4[w].w);
        return p;
    }

    // popc(held row & other row); `other` is wave-uniform
    __device__ __forceinline__ uint32_t common(const_u32x4p other) const
    {
        uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
#pragma unroll
        for (int w = 0; w < WP / 4; w++) {
            const u32x4 q = other[w]; // s_load
            acc0 = bcnt_acc(r4[w].x & q.x, acc0);
            acc1 = bcnt_acc(r4[w].y & q.y, acc1);
            acc2 = bcnt_acc(r4[w].z & q.z, acc2);
            acc3 = bcnt_acc(r4[w].w & q.w, acc3);
        }
        return (acc0 + acc1) + (acc2 + acc3);
    }
};

// One value of a side array per step of a walk over the other side's rows.  At every 64th step (due(t)), step t being row
// `at`, lane l fetches src[at + l] (0 from `end` on); every step reads its own value back with v_readlane (wave-uniform).
struct Handout64 {
    uint32_t v = 0;

    static __device__ __forceinline__ bool due(uint32_t t) { return (t & 63u) == 0; }
    __device__ __forceinline__ void fetch(const uint32_t* src, u64 at, uint32_t lane, u64 end)
    {
        const u64 x = at + lane;
        v = x < end ? src[x] : 0u;
    }
    __device__ __forceinline__ uint32_t get(uint32_t t) const { return readlane_u32(v, t & 63u); }
};

// f(std::integral_constant<int, WP>) for the padded width WP of a call: the instantiations of a held-row kernel
template <class F> hipError_t dispatch_wp(uint32_t WP, F&& f)
{
    switch (WP) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    default: return hipErrorInvalidValue;
    }
}

} // namespace
} // namespace gsim
