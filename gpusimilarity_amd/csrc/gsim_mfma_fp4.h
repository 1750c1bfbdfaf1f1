// gsim_mfma_fp4.h -- packed fingerprint bits as FP4 operands of gfx950's block-scaled MFMA: what the matrix-core kernels
// (gsim_batch_mfma.hip, gsim_scores.hip) share.  Internal, device code only.
//
// Packed bits -> FP4 (E2M1) operands with ONE v_and per operand dword (scripts/mfma_fp4_probe.hip):
//   x & 0x11111111 -> nibbles {0, 0.5}    block scale 2^1
//   x & 0x22222222 -> nibbles {0, 1.0}    block scale 2^0
//   x & 0x44444444 -> nibbles {0, 2.0}    block scale 2^-1
//   (x >> 3) & 0x11111111                 (0x8 is the FP4 sign bit: -0, so that class is shifted)
// i.e. each 256-bit group of a row (8 words: 4 per lane half) feeds four MFMAs, one per class; with both operands scaled
// the same way every set bit pair contributes exactly 1.0, and the f32 accumulators hold the intersection counts exactly
// (< 2^24).  Which bit lands in which k slot is irrelevant as long as both operands use the same map.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsim_device_common.h"

namespace gsim
{
namespace
{

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kScale1 = 0x80808080;  // E8M0 2^1
constexpr int kScale0 = 0x7F7F7F7F;  // 2^0
constexpr int kScaleM = 0x7E7E7E7E;  // 2^-1

// The class masks are passed in VGPRs: v_and_b32 with two vector operands issues in 2 cycles,
// with a literal or scalar operand in 4 (scripts/valu_op_rate_probe.hip).
struct ClassMasks {
    uint32_t m1, m2, m4;
};

template <int CLS> __device__ __forceinline__ uint32_t fp4_word(uint32_t x, const ClassMasks& k)
{
    return CLS == 0 ? (x & k.m1) : CLS == 1 ? (x & k.m2) : CLS == 2 ? (x & k.m4) : ((x >> 3) & k.m1);
}

// element by element: a vector AND with a splat mask makes hipcc keep four copies of every mask
template <int CLS> __device__ __forceinline__ v4i fp4_class(u32x4 x, const ClassMasks& k)
{
    return v4i{static_cast<int>(fp4_word<CLS>(x.x, k)), static_cast<int>(fp4_word<CLS>(x.y, k)),
               static_cast<int>(fp4_word<CLS>(x.z, k)), static_cast<int>(fp4_word<CLS>(x.w, k))};
}

template <int CLS> __device__ __forceinline__ v16f mfma_class(v4i qa, v4i rb, v16f acc)
{
    const v8i A = {qa.x, qa.y, qa.z, qa.w, 0, 0, 0, 0};
    const v8i B = {rb.x, rb.y, rb.z, rb.w, 0, 0, 0, 0};
    constexpr int sc = CLS == 1 ? kScale0 : (CLS == 2 ? kScaleM : kScale1);
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, acc, /*A fp4*/ 4, /*B fp4*/ 4, 0, sc, 0, sc);
}

} // namespace
} // namespace gsim
