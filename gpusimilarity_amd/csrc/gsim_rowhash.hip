// gsim_rowhash.hip -- row-hash indexes (gsim_rowhash_*): which rows of a table are the same fingerprint, and where a given
// fingerprint is.  An open-addressing table in global memory, one slot = {row, count} (two 32-bit words, 8 bytes, side by side so
// that a probe touches one line):
//   rowhash_init_kernel       every slot {GSIM_ROW_NONE, 0}
//   rowhash_x4_kernel<LPR>    INSERT: one streaming pass over the table (walk_rows_x4, gsim_row_units.h: 16 B per lane,
//                             non-temporal): the LPR lanes that share a row hash their own four words and add (group_sum),
//                             then probe from the row's first slot -- compare-and-swap the row's own number into an empty slot, or
//                             gather the occupant's row, compare all words, and on equality atomicMin the slot's row and add one to
//                             its count; on a difference go to the next slot.  The occupant of a slot only ever changes to a row with
//                             the same words and a slot never empties, so every distinct fingerprint ends up owning exactly one slot
//                             whatever the interleaving, and that slot ends up holding the group's lowest row and its size.  The
//                             row's slot is recorded (8 bytes per row: slot numbers pass 2^32 above 2^31 rows).
//                             FIND: the same loader over the left rows, the probe read-only.
//   rowhash_strided_kernel<G> every other width (walk_rows_strided): one row per lane (rows of fewer than 32 words) or per wave,
//                             word by word
//   rowhash_finish_kernel     every row's {first, size} from its slot, the bitmap of the first rows, the counts
// Memory model (MI355X: the L2s of the XCDs are not coherent with one another): slots are touched ONLY through agent-scope atomics
// (load, compare-and-swap, min, add); the table's rows are immutable during a call and are read with plain loads; what one launch
// leaves for the next (the recorded slots, the slots themselves) is made visible by the launch boundary.
// No workgroup ever waits for another: there is no spin-wait, lock or grid barrier.  Every probe loop ends after `nslots` steps at
// the latest and raises `flag` if it had to, which the host turns into an error.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_row_units.h"
#include "gsim_rowhash_hash.h"

namespace gsim
{
namespace
{

constexpr int kRhBlock = kRowhashBlock;
constexpr int kRhUnroll = kRowhashUnroll; // 16-byte loads in flight per lane
constexpr uint32_t kRhNone = GSIM_ROW_NONE;

#define GSIM_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct RhTable {
    uint32_t* slots; // 2 x nslots words: {row, count}
    u64 nslots;      // a power of two
    uint32_t* flag;  // raised when a probe went round the whole table
};

// the value the first lane of every aligned group of G lanes holds (all 64 lanes active)
template <int G> __device__ __forceinline__ uint32_t group_first(uint32_t v, int lane)
{
    if (G == 1) return v;
    return static_cast<uint32_t>(__shfl(static_cast<int>(v), lane & ~(G - 1), 64));
}

// One probe per group of G lanes, all 64 lanes of the wave inside (the loop is wave-uniform: the groups that are done idle).
// `active`, `hash` and `myrow` are uniform over a group; match(ask, occ), called by every lane, says -- uniformly over a group --
// whether the group's row has the words of table row `occ` (false where `ask` is false).  INSERT: out_slot is the slot the row ended
// in.  FIND: out_row is the lowest identical row, or GSIM_ROW_NONE, and out_slot its slot.
template <int G, bool INSERT, typename Match>
__device__ __forceinline__ void probe(const RhTable& t, bool active, u64 hash, uint32_t myrow, int lane, Match&& match, uint32_t& out_row,
                                      u64& out_slot)
{
    const bool lead = (lane & (G - 1)) == 0;
    const u64 mask = t.nslots - 1;
    u64 s = hash & mask;
    u64 steps = 0;
    bool done = !active;
    out_row = kRhNone;
    out_slot = 0;
    while (__ballot(!done) != 0) {
        uint32_t occ = kRhNone;
        if (!done && lead) {
            if (INSERT) { // (a failed swap returns the occupant: the slot is looked at again through it)
                __hip_atomic_compare_exchange_strong(&t.slots[2 * s], &occ, myrow, __ATOMIC_RELAXED, GSIM_RLX);
            } else {
                occ = __hip_atomic_load(&t.slots[2 * s], GSIM_RLX);
            }
        }
        occ = group_first<G>(occ, lane);
        const bool same = match(!done && occ != kRhNone, occ);
        if (!done) {
            if (occ == kRhNone) { // INSERT: the slot is this row's now; FIND: no row has these words
                if (INSERT) {
                    if (lead) __hip_atomic_fetch_add(&t.slots[2 * s + 1], 1u, GSIM_RLX);
                    out_slot = s;
                }
                done = true;
            } else if (same) {
                if (INSERT && lead) { // (the occupant only ever gets lower: above this row it may need lowering, below it never)
                    if (myrow < occ) __hip_atomic_fetch_min(&t.slots[2 * s], myrow, GSIM_RLX);
                    __hip_atomic_fetch_add(&t.slots[2 * s + 1], 1u, GSIM_RLX);
                }
                out_row = occ;
                out_slot = s;
                done = true;
            } else {
                s = (s + 1) & mask;
                steps++;
                if (steps >= t.nslots) { // a full table: impossible at a load of 1/2 -- end, and say so
                    if (lead) __hip_atomic_fetch_or(t.flag, 1u, GSIM_RLX);
                    done = true;
                }
            }
        }
    }
}

// what a row leaves behind: INSERT its slot, FIND {row, size} of the group found
template <bool INSERT>
__device__ __forceinline__ void record(const RhTable& t, bool writer, u64 at, uint32_t out_row, u64 out_slot, u64* __restrict__ rec)
{
    if (!writer) return;
    if (INSERT) {
        rec[at] = out_slot;
    } else {
        const uint32_t size = out_row != kRhNone ? __hip_atomic_load(&t.slots[2 * out_slot + 1], GSIM_RLX) : 0u;
        rec[at] = static_cast<u64>(out_row) | (static_cast<u64>(size) << 32);
    }
}

__global__ __launch_bounds__(kRhBlock) void rowhash_init_kernel(u64* __restrict__ slots, u64 nslots)
{
    const u64 stride = static_cast<u64>(gridDim.x) * kRhBlock;
    for (u64 i = static_cast<u64>(blockIdx.x) * kRhBlock + threadIdx.x; i < nslots; i += stride) slots[i] = static_cast<u64>(kRhNone);
}

// Rows of LPR sixteen-byte units, LPR a power of two up to 64 (walk_rows_x4: chunks of kRhUnroll x 64 / LPR rows).  `src` rows
// [r0, r1) are hashed; INSERT: they are the table's rows of those numbers, rec[row] = slot; FIND: they are the left rows,
// rec[row] = the answer.
template <int LPR, bool INSERT>
__global__ __launch_bounds__(kRhBlock) void rowhash_x4_kernel(const u32x4* __restrict__ src, u64 r0, u64 r1, const u32x4* __restrict__ table, RhTable t,
                                                              u64* __restrict__ rec)
{
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const u64 w = static_cast<u64>(blockIdx.x) * (kRhBlock / 64) + (threadIdx.x >> 6);
    const u64 nwaves = static_cast<u64>(gridDim.x) * (kRhBlock / 64);
    const uint32_t k0 = rowhash_key(4u * sub), k1 = rowhash_key(4u * sub + 1u), k2 = rowhash_key(4u * sub + 2u), k3 = rowhash_key(4u * sub + 3u);
    walk_rows_x4<LPR, kRhUnroll>(src, r0, r1, w, nwaves, lane, [&](u64 row, bool in, const u32x4& mine) {
        uint32_t A = 0, B = 0;
        rowhash_word(mine.x, k0, A, B);
        rowhash_word(mine.y, k1, A, B);
        rowhash_word(mine.z, k2, A, B);
        rowhash_word(mine.w, k3, A, B);
        A = group_sum<LPR>(A);
        B = group_sum<LPR>(B);
        auto match = [&](bool ask, uint32_t occ) {
            uint32_t ne = 0;
            if (ask) {
                const u32x4 o = table[static_cast<u64>(occ) * LPR + sub];
                ne = ((o.x ^ mine.x) | (o.y ^ mine.y) | (o.z ^ mine.z) | (o.w ^ mine.w)) != 0 ? 1u : 0u;
            }
            return ask && group_sum<LPR>(ne) == 0;
        };
        uint32_t out_row;
        u64 out_slot;
        probe<LPR, INSERT>(t, in, rowhash_final(A, B), static_cast<uint32_t>(row), lane, match, out_row, out_slot);
        record<INSERT>(t, sub == 0 && in, row, out_row, out_slot, rec);
    });
}

// Every other width, G lanes per row striding over its words (walk_rows_strided): G = 1 or 64.
template <int G, bool INSERT>
__global__ __launch_bounds__(kRhBlock) void rowhash_strided_kernel(const uint32_t* __restrict__ src, u64 r0, u64 r1, uint32_t W,
                                                                   const uint32_t* __restrict__ table, RhTable t, u64* __restrict__ rec)
{
    const int lane = threadIdx.x & 63;
    const uint32_t sub = static_cast<uint32_t>(lane % G);
    const u64 w = static_cast<u64>(blockIdx.x) * (kRhBlock / 64) + (threadIdx.x >> 6);
    const u64 nwaves = static_cast<u64>(gridDim.x) * (kRhBlock / 64);
    walk_rows_strided<G>(src, r0, r1, W, w, nwaves, lane, [&](u64 row, bool in, const uint32_t* mine) {
        uint32_t A = 0, B = 0;
        if (in)
            for (uint32_t i = sub; i < W; i += G) rowhash_word(mine[i], rowhash_key(i), A, B);
        A = group_sum<G>(A);
        B = group_sum<G>(B);
        auto match = [&](bool ask, uint32_t occ) {
            uint32_t ne = 0;
            if (ask) {
                const uint32_t* o = table + static_cast<u64>(occ) * W;
                for (uint32_t i = sub; i < W && ne == 0; i += G) ne = o[i] != mine[i] ? 1u : 0u;
            }
            return ask && group_sum<G>(ne) == 0;
        };
        uint32_t out_row;
        u64 out_slot;
        probe<G, INSERT>(t, in, rowhash_final(A, B), static_cast<uint32_t>(row), lane, match, out_row, out_slot);
        record<INSERT>(t, sub == 0 && in, row, out_row, out_slot, rec);
    });
}

// rec[row]: the row's slot -> {first, size} of its group (first in the low word, without a row base); bit `row` of `bits` says
// first == row; counters: groups, groups of two rows or more, the largest size, the sizes of the groups summed (= n).  Wave w takes
// the tiles of 64 rows w, w + nwaves, ...
__global__ __launch_bounds__(kRhBlock) void rowhash_finish_kernel(u64* __restrict__ rec, u64 n, RhTable t, uint32_t* __restrict__ bits, u64 nbitwords,
                                                                  u64* __restrict__ counters)
{
    const int lane = threadIdx.x & 63;
    const u64 w = static_cast<u64>(blockIdx.x) * (kRhBlock / 64) + (threadIdx.x >> 6);
    const u64 nwaves = static_cast<u64>(gridDim.x) * (kRhBlock / 64);
    const u64 ntiles = (n + 63) / 64;
    u64 groups = 0, repeated = 0, largest = 0, total = 0;
    bool bad = false;
    for (u64 tile = w; tile < ntiles; tile += nwaves) {
        const u64 row = tile * 64 + static_cast<u64>(lane);
        const bool active = row < n;
        uint32_t first = kRhNone, size = 0;
        if (active) {
            const u64 s = rec[row];
            if (s < t.nslots) {
                const u64 v = __hip_atomic_load(reinterpret_cast<const u64*>(t.slots) + s, GSIM_RLX);
                first = static_cast<uint32_t>(v);
                size = static_cast<uint32_t>(v >> 32);
            }
            bad = bad || first > row || size == 0;
            rec[row] = static_cast<u64>(first) | (static_cast<u64>(size) << 32);
        }
        const bool is_first = active && first == row;
        const u64 m = __ballot(is_first);
        if (lane == 0 && 2 * tile < nbitwords) bits[2 * tile] = static_cast<uint32_t>(m);
        if (lane == 32 && 2 * tile + 1 < nbitwords) bits[2 * tile + 1] = static_cast<uint32_t>(m >> 32);
        if (is_first) {
            groups++;
            repeated += size >= 2 ? 1 : 0;
            total += size;
        }
        largest = size > largest ? size : largest;
    }
    for (int d = 32; d > 0; d >>= 1) {
        groups += __shfl_xor(groups, d, 64);
        repeated += __shfl_xor(repeated, d, 64);
        total += __shfl_xor(total, d, 64);
        const u64 o = __shfl_xor(largest, d, 64);
        largest = o > largest ? o : largest;
    }
    if (__ballot(bad) != 0 && lane == 0) __hip_atomic_fetch_or(t.flag, 2u, GSIM_RLX);
    if (lane == 0 && w < ntiles) {
        __hip_atomic_fetch_add(&counters[0], groups, GSIM_RLX);
        __hip_atomic_fetch_add(&counters[1], repeated, GSIM_RLX);
        __hip_atomic_fetch_max(&counters[2], largest, GSIM_RLX);
        __hip_atomic_fetch_add(&counters[3], total, GSIM_RLX);
    }
}

uint32_t rh_blocks(uint64_t waves_of_work, int num_cus)
{
    // eight waves per SIMD where there is work for them: a probe is a chain of dependent atomics and gathers, hidden by the waves beside it
    const uint64_t want = (waves_of_work + (kRhBlock / 64) - 1) / (kRhBlock / 64);
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(want, static_cast<uint64_t>(num_cus > 0 ? num_cus : 1) * 8u)));
}

template <int LPR, bool INSERT>
hipError_t launch_x4_t(const void* src, uint64_t r0, uint64_t r1, const void* table, const RhTable& t, u64* rec, int num_cus, hipStream_t s)
{
    const uint64_t ch = static_cast<uint64_t>(kRhUnroll) * (64 / LPR);
    hipLaunchKernelGGL((rowhash_x4_kernel<LPR, INSERT>), dim3(rh_blocks((r1 - r0 + ch - 1) / ch, num_cus)), dim3(kRhBlock), 0, s,
                       static_cast<const u32x4*>(src), static_cast<u64>(r0), static_cast<u64>(r1), static_cast<const u32x4*>(table), t, rec);
    return hipGetLastError();
}

template <int G, bool INSERT>
hipError_t launch_strided_t(const void* src, uint64_t r0, uint64_t r1, uint32_t W, const void* table, const RhTable& t, u64* rec, int num_cus,
                            hipStream_t s)
{
    const uint64_t rpw = 64 / G;
    hipLaunchKernelGGL((rowhash_strided_kernel<G, INSERT>), dim3(rh_blocks((r1 - r0 + rpw - 1) / rpw, num_cus)), dim3(kRhBlock), 0, s,
                       static_cast<const uint32_t*>(src), static_cast<u64>(r0), static_cast<u64>(r1), W, static_cast<const uint32_t*>(table), t, rec);
    return hipGetLastError();
}

template <bool INSERT>
hipError_t launch_rows_t(const void* src, uint64_t r0, uint64_t r1, uint32_t W, const void* table, const RhTable& t, u64* rec, int num_cus, hipStream_t s)
{
    if (r0 >= r1) return hipSuccess;
    if (W == 0 || !src || !table || !t.slots || !t.flag || !rec || t.nslots == 0 || (t.nslots & (t.nslots - 1)) != 0) return hipErrorInvalidValue;
    if (const uint32_t lpr = pow2_lanes_per_row(W))
        return dispatch_lpr(lpr, [&](auto l) { return launch_x4_t<decltype(l)::value, INSERT>(src, r0, r1, table, t, rec, num_cus, s); });
    if (W < 32u) return launch_strided_t<1, INSERT>(src, r0, r1, W, table, t, rec, num_cus, s);
    return launch_strided_t<64, INSERT>(src, r0, r1, W, table, t, rec, num_cus, s);
}

} // namespace

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------

hipError_t launch_rowhash_init(uint32_t* slots, uint64_t nslots, int num_cus, hipStream_t s)
{
    if (nslots == 0) return hipSuccess;
    if (!slots) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rowhash_init_kernel, dim3(rh_blocks((nslots + 63) / 64, num_cus)), dim3(kRhBlock), 0, s, reinterpret_cast<u64*>(slots),
                       static_cast<u64>(nslots));
    return hipGetLastError();
}

hipError_t launch_rowhash_insert(const void* rows, uint64_t r0, uint64_t r1, uint32_t W, uint32_t* slots, uint64_t nslots, uint32_t* flag,
                                 unsigned long long* slot_of, int num_cus, hipStream_t s)
{
    return launch_rows_t<true>(rows, r0, r1, W, rows, RhTable{slots, nslots, flag}, slot_of, num_cus, s);
}

hipError_t launch_rowhash_finish(unsigned long long* rec, uint64_t n, uint32_t* slots, uint64_t nslots, uint32_t* flag, uint32_t* bits,
                                 uint64_t nbitwords, unsigned long long* counters, int num_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (!rec || !slots || !flag || !bits || !counters || nslots == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rowhash_finish_kernel, dim3(rh_blocks((n + 63) / 64, num_cus)), dim3(kRhBlock), 0, s, rec, static_cast<u64>(n),
                       RhTable{slots, nslots, flag}, bits, static_cast<u64>(nbitwords), counters);
    return hipGetLastError();
}

hipError_t launch_rowhash_find(const void* left, uint64_t nl, const void* rows, uint32_t W, const uint32_t* slots, uint64_t nslots, uint32_t* flag,
                               unsigned long long* found, int num_cus, hipStream_t s)
{
    return launch_rows_t<false>(left, 0, nl, W, rows, RhTable{const_cast<uint32_t*>(slots), nslots, flag}, found, num_cus, s);
}

} // namespace gsim
