// gsim_rowhash_hash.h -- the library's 64-bit hash of a row and the slot rule of the row-hash table, as include/gpusim_hip.h states
// them (gsim_row_hash): one definition for the kernels (gsim_rowhash.hip) and for the host functions (capi_rowhash_host.cpp, which
// is built without HIP -- the file depends on <stdint.h> alone).  32-bit arithmetic only; a word's contribution depends on its
// position and the contributions are summed, so that the lanes that share a row each hash their own words and add.  Internal.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GSIM_RH_FN __host__ __device__ inline
#else
#define GSIM_RH_FN inline
#endif

namespace gsim
{

constexpr uint32_t kRowhashGold = 0x9E3779B9u;
constexpr uint64_t kRowhashMinSlots = 1024;

GSIM_RH_FN uint32_t rowhash_m1(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

GSIM_RH_FN uint32_t rowhash_m2(uint32_t x)
{
    x ^= x >> 15;
    x *= 0x2C1B3C6Du;
    x ^= x >> 12;
    x *= 0x297A2D39u;
    x ^= x >> 15;
    return x;
}

// the position key of word i
GSIM_RH_FN uint32_t rowhash_key(uint32_t i)
{
    return (i + 1u) * kRowhashGold;
}

// word w under the position key k: its two contributions, added to the sums
GSIM_RH_FN void rowhash_word(uint32_t w, uint32_t k, uint32_t& A, uint32_t& B)
{
    uint32_t a = (w ^ k) * 0x85EBCA6Bu;
    a ^= a >> 15;
    uint32_t b = (((w << 16) | (w >> 16)) + k) * 0xC2B2AE35u;
    b ^= b >> 13;
    A += a;
    B += b;
}

// the avalanche of the two sums: a bijection of (A, B)
GSIM_RH_FN uint64_t rowhash_final(uint32_t A, uint32_t B)
{
    const uint32_t lo = rowhash_m1(A ^ rowhash_m2(B));
    const uint32_t hi = rowhash_m2(B ^ lo);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// slots of the table of n rows: 0 for none, else the smallest power of two >= 2 n, at least kRowhashMinSlots; a row's first slot is
// hash & (slots - 1)
inline uint64_t rowhash_slots(uint64_t n)
{
    if (n == 0) return 0;
    uint64_t s = kRowhashMinSlots;
    while (s < 2 * n) s <<= 1;
    return s;
}

} // namespace gsim
