// gsim_label_search.hip -- label-grouped search (gsim_db_search_labels): the best hit and the hit count of every label for a tile
// of queries, in one streaming pass over the table.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 30 has the
// routes, the budget and the measurements.
//
// The scan has group_scan_kernel's layout (gsim_group.hip): a lane holds RPL whole rows in registers, the row's popcount is taken
// once, the queries of the pass are wave-uniform (constant address space: scalar loads, the SGPR operand of v_and_b32), and the
// labels of a chunk are one coalesced 4-byte load per row.  Where the group scan reduces a row's scores over the queries and offers
// the row to the streaming top-k filter, this one reduces over the ROWS of a label: a kept row's candidate key
// make_key(score, row) -- unique, its descending order the canonical (score descending, row ascending) order, never 0 -- goes into
// best[q][label] by a 64-bit max, and into kept[q][label] by a 32-bit add where a count was asked for.  Max and integer add commute:
// the tables depend neither on the grid nor on the launch cut nor on the route.
//   route LDS     the table is the workgroup's (zeroed at the start of a launch); at the end of the launch its non-zero entries are
//                 merged into the global table;
//   route global  the same updates go straight to the global table.
// Either way the max is GUARDED by a plain read: only a lane whose key improves the entry issues the atomic.  A table stored in
// cluster order puts the 64 rows of a load on one address: the read is a broadcast, and after the first few chunks of a label
// almost no lane improves on it.  The count has no such guard; when every kept row of a wave's load carries one label (the same
// tables) one lane adds the whole number.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

typedef const __attribute__((address_space(4))) uint32_t* ConstWords; // constant address space: wave-uniform reads are scalar loads

// the first chunk of wave w at or after c0 (chunk c belongs to wave c % nwaves in every launch of the pass)
__device__ __forceinline__ u64 first_chunk(u64 c0, uint32_t w, uint32_t nwaves)
{
    const uint32_t r = static_cast<uint32_t>(c0 % nwaves);
    return c0 + (w >= r ? w - r : w + nwaves - r);
}

// One row against one query: the score as gsim_db_search makes it, and the two updates.
struct LabelTable {
    u64* best;      // the pass's table: the workgroup's (LDS) or the call's (global)
    uint32_t* kept; // nullptr: not counted
    bool has_cutoff;

    __device__ __forceinline__ void add(bool live, uint32_t row, uint32_t label, size_t qbase, float raw, float cutoff, int lane) const
    {
        const float s = apply_cutoff(raw, cutoff); // (NaN -> 0)
        const bool keep = live && (!has_cutoff || s != 0.0f);
        if (keep) {
            const u64 key = make_key(s, row);
            u64* p = best + qbase + label;
            if (*p < key) atomicMax(p, key);
        }
        if (kept) { // (wave-uniform)
            const u64 m = __ballot(keep);
            if (m != 0) {
                const int first = __ffsll(static_cast<long long>(m)) - 1;
                const uint32_t l0 = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(label), first));
                if (__ballot(keep && label != l0) == 0) {
                    if (lane == first) atomicAdd(kept + qbase + l0, static_cast<uint32_t>(__popcll(m)));
                } else if (keep) {
                    atomicAdd(kept + qbase + label, 1u);
                }
            }
        }
    }
};

// WORDS != 0: rows of WORDS words (a multiple of 4) held in registers, RPL rows per lane.  WORDS == 0: any width, one row per lane,
// word by word (the row is read again for every query -- from the cache; correct, not fast).
// LDS: the pass's table lives in the workgroup's dynamic LDS (a.lds_bytes); the workgroup has a.block threads, up to 1024.
template <int WORDS, int RPL, bool LDS>
__global__ __launch_bounds__(LDS ? 1024 : kScanBlock) void label_scan_kernel(LabelSearchArgs a)
{
    extern __shared__ u64 s_table[];
    const int lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (a.block / 64) + (threadIdx.x >> 6));
    const uint32_t nq = a.nq;
    const size_t cells = static_cast<size_t>(nq) * a.nlabels;
    LabelTable t;
    t.has_cutoff = a.cutoff > 0.0f;
    if constexpr (LDS) {
        t.best = s_table;
        t.kept = a.kept ? reinterpret_cast<uint32_t*>(s_table + cells) : nullptr;
        for (size_t i = threadIdx.x; i < cells; i += a.block) s_table[i] = 0;
        if (t.kept)
            for (size_t i = threadIdx.x; i < cells; i += a.block) t.kept[i] = 0;
        __syncthreads();
    } else {
        t.best = a.best;
        t.kept = a.kept;
    }
    const ConstWords qbase = (ConstWords) a.queries;
    const ConstWords qpop = (ConstWords) a.qpop;

    if constexpr (WORDS != 0) {
        constexpr int CHR = 64 * RPL;
        const u32x4* __restrict__ db = reinterpret_cast<const u32x4*>(a.rows);
        for (u64 c = first_chunk(a.c0, w, a.nwaves); c < a.c1; c += a.nwaves) {
            u32x4 r4[RPL][WORDS / 4];
            uint32_t bb[RPL], lab[RPL];
            bool live[RPL];
            u64 rowi[RPL];
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                rowi[r] = c * CHR + r * 64 + lane;
                const bool active = rowi[r] < a.nrows;
                const u32x4* p = db + rowi[r] * (WORDS / 4);
#pragma unroll
                for (int j = 0; j < WORDS / 4; j++) r4[r][j] = active ? p[j] : u32x4{0, 0, 0, 0};
                lab[r] = active ? a.labels[rowi[r]] : GSIM_LABEL_NONE;
                live[r] = lab[r] != GSIM_LABEL_NONE;
            }
#pragma unroll
            for (int r = 0; r < RPL; r++) {
                bb[r] = 0;
#pragma unroll
                for (int j = 0; j < WORDS / 4; j++) bb[r] += __popc(r4[r][j].x) + __popc(r4[r][j].y) + __popc(r4[r][j].z) + __popc(r4[r][j].w);
            }
            for (uint32_t q = 0; q < nq; q++) {
                const ConstWords qw = qbase + static_cast<size_t>(q) * WORDS;
                uint32_t cnt[RPL][4];
#pragma unroll
                for (int r = 0; r < RPL; r++) cnt[r][0] = cnt[r][1] = cnt[r][2] = cnt[r][3] = 0;
#pragma unroll
                for (int j = 0; j < WORDS / 4; j++) {
                    const uint32_t q0w = qw[4 * j + 0], q1w = qw[4 * j + 1], q2w = qw[4 * j + 2], q3w = qw[4 * j + 3];
#pragma unroll
                    for (int r = 0; r < RPL; r++) {
                        cnt[r][0] = bcnt_acc(r4[r][j].x & q0w, cnt[r][0]);
                        cnt[r][1] = bcnt_acc(r4[r][j].y & q1w, cnt[r][1]);
                        cnt[r][2] = bcnt_acc(r4[r][j].z & q2w, cnt[r][2]);
                        cnt[r][3] = bcnt_acc(r4[r][j].w & q3w, cnt[r][3]);
                    }
                }
                const uint32_t qa = qpop[q];
                const size_t qb = static_cast<size_t>(q) * a.nlabels;
#pragma unroll
                for (int r = 0; r < RPL; r++) {
                    const uint32_t cc = (cnt[r][0] + cnt[r][1]) + (cnt[r][2] + cnt[r][3]);
                    t.add(live[r], static_cast<uint32_t>(rowi[r]), lab[r], qb, score_of(a.metric, a.alpha, a.beta, qa, bb[r], cc), a.cutoff, lane);
                }
            }
        }
    } else {
        const uint32_t* __restrict__ db = static_cast<const uint32_t*>(a.rows);
        const uint32_t W = a.W;
        for (u64 c = first_chunk(a.c0, w, a.nwaves); c < a.c1; c += a.nwaves) {
            const u64 rowi = c * 64u + static_cast<uint32_t>(lane);
            const bool active = rowi < a.nrows;
            const uint32_t* r = db + (active ? rowi : 0) * W;
            const uint32_t lab = active ? a.labels[rowi] : GSIM_LABEL_NONE;
            const bool live = lab != GSIM_LABEL_NONE;
            uint32_t bb = 0;
            if (live)
                for (uint32_t i = 0; i < W; i++) bb += __popc(r[i]);
            for (uint32_t q = 0; q < nq; q++) {
                const ConstWords qw = qbase + static_cast<size_t>(q) * W;
                uint32_t cc = 0;
                if (live)
                    for (uint32_t i = 0; i < W; i++) cc += __popc(r[i] & qw[i]);
                t.add(live, static_cast<uint32_t>(rowi), lab, static_cast<size_t>(q) * a.nlabels, score_of(a.metric, a.alpha, a.beta, qpop[q], bb, cc), a.cutoff,
                      lane);
            }
        }
    }

    if constexpr (LDS) {
        // the workgroup's table into the call's: the entries that hold something
        __syncthreads();
        for (size_t i = threadIdx.x; i < cells; i += a.block) {
            const u64 key = s_table[i];
            if (key != 0 && a.best[i] < key) atomicMax(a.best + i, key);
        }
        if (t.kept)
            for (size_t i = threadIdx.x; i < cells; i += a.block) {
                const uint32_t n = t.kept[i];
                if (n != 0) atomicAdd(a.kept + i, n);
            }
    }
}

// One thread per (query, label): the hit behind the entry's key.  The grid's y is the query; totals[2 q], totals[2 q + 1]: the
// labels with a row, the kept rows.
__global__ __launch_bounds__(256) void label_finish_kernel(LabelSearchArgs a, uint32_t row_base, gsim_hit* label_best, u64* totals)
{
    const uint32_t q = blockIdx.y;
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    const bool in = l < a.nlabels;
    const size_t cell = static_cast<size_t>(q) * a.nlabels + (in ? l : 0u);
    const u64 key = in ? a.best[cell] : 0;
    if (in) {
        gsim_hit h{0xFFFFFFFFu, 0.0f, 0, 0};
        if (key != 0) {
            const uint32_t row = ~static_cast<uint32_t>(key);
            const uint32_t* r = static_cast<const uint32_t*>(a.rows) + static_cast<u64>(row) * a.W;
            const uint32_t* qw = a.queries + static_cast<size_t>(q) * a.W;
            uint32_t cc = 0, bb = 0;
            for (uint32_t j = 0; j < a.W; j++) {
                cc += __popc(r[j] & qw[j]);
                bb += __popc(r[j]);
            }
            h.row = row + row_base;
            h.score = key_score(static_cast<uint32_t>(key >> 32));
            h.common = static_cast<uint16_t>(cc);
            h.popc_db = static_cast<uint16_t>(bb);
        }
        label_best[cell] = h;
    }
    const uint32_t found = wave_sum(key != 0 ? 1u : 0u);
    const uint32_t rows = wave_sum(in && a.kept ? a.kept[cell] : 0u);
    if ((threadIdx.x & 63) == 0) {
        if (found) atomicAdd(totals + 2 * q, static_cast<u64>(found));
        if (rows) atomicAdd(totals + 2 * q + 1, static_cast<u64>(rows));
    }
}

__global__ __launch_bounds__(256) void label_emit_kernel(const u64* sorted, const uint32_t* labels, const gsim_hit* label_best, uint32_t kk, gsim_hit* hits,
                                                         uint32_t* hit_labels)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= kk) return;
    const u64 key = sorted[i];
    if (key == 0) return; // (fewer labels with a row than kk: the host takes min(k, approx) entries)
    const uint32_t l = labels[~static_cast<uint32_t>(key)];
    hits[i] = label_best[l];
    hit_labels[i] = l;
}

template <int WORDS, int RPL> hipError_t launch_label_scan_t(const LabelSearchArgs& a, hipStream_t s)
{
    const dim3 grid(a.nwaves / (a.block / 64)), block(a.block);
    if (a.lds_bytes) {
        static DynLdsOnce once;
        const hipError_t e = once.ensure(reinterpret_cast<const void*>(label_scan_kernel<WORDS, RPL, true>), kLabelLdsBudget);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((label_scan_kernel<WORDS, RPL, true>), grid, block, a.lds_bytes, s, a);
    } else {
        hipLaunchKernelGGL((label_scan_kernel<WORDS, RPL, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

} // namespace

// rows of a chunk: 64 x the rows a lane holds (launch_label_scan's switch), 64 for the word loop
uint32_t label_chunk_rows(uint32_t W)
{
    return 64u * (W == 4 || W == 8 || W == 16 ? 4u : (W == 32 ? 2u : 1u));
}

// LDS decides the occupancy of route LDS: a compute unit has 160 KiB, so tables of up to 40 KiB leave room for four workgroups,
// up to 80 KiB for two, beyond for one -- of 256, 512 and 1024 threads: kLabelScanWavesPerCu = 16 waves in every class.
uint32_t label_block_threads(uint32_t lds_bytes)
{
    return lds_bytes <= 40u * 1024u ? 256u : (lds_bytes <= 80u * 1024u ? 512u : 1024u);
}

hipError_t launch_label_scan(const LabelSearchArgs& a, hipStream_t s)
{
    if (a.c0 >= a.c1) return hipSuccess;
    const size_t need = static_cast<size_t>(a.nq) * a.nlabels * (a.kept ? 12u : 8u);
    if (a.block != label_block_threads(a.lds_bytes) || a.nwaves == 0 || a.nwaves % (a.block / 64) != 0 || a.lds_bytes > kLabelLdsBudget ||
        (a.lds_bytes != 0 && a.lds_bytes != need))
        return hipErrorInvalidValue;
    switch (a.W) {
    case 4: return launch_label_scan_t<4, 4>(a, s);
    case 8: return launch_label_scan_t<8, 4>(a, s);
    case 16: return launch_label_scan_t<16, 4>(a, s);
    case 32: return launch_label_scan_t<32, 2>(a, s);
    case 64: return launch_label_scan_t<64, 1>(a, s);
    default: return launch_label_scan_t<0, 1>(a, s);
    }
}

hipError_t launch_label_finish(const LabelSearchArgs& a, uint32_t row_base, void* label_best, unsigned long long* totals, hipStream_t s)
{
    hipLaunchKernelGGL(label_finish_kernel, dim3((a.nlabels + 255u) / 256u, a.nq), dim3(256), 0, s, a, row_base, static_cast<gsim_hit*>(label_best), totals);
    return hipGetLastError();
}

hipError_t label_rank_bytes(uint32_t nlabels, size_t* bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_keys_desc(nullptr, *bytes, static_cast<const u64*>(nullptr), static_cast<u64*>(nullptr), static_cast<size_t>(nlabels));
}

hipError_t launch_label_rank(void* tmp, size_t tmp_bytes, const unsigned long long* best, unsigned long long* sorted, uint32_t nlabels, hipStream_t s)
{
    size_t bytes = tmp_bytes;
    return rocprim::radix_sort_keys_desc(tmp, bytes, best, sorted, static_cast<size_t>(nlabels), 0u, 64u, s);
}

hipError_t launch_label_emit(const unsigned long long* sorted, const uint32_t* labels, const void* label_best, uint32_t kk, void* hits, uint32_t* hit_labels,
                             hipStream_t s)
{
    if (kk == 0) return hipSuccess;
    hipLaunchKernelGGL(label_emit_kernel, dim3((kk + 255u) / 256u), dim3(256), 0, s, sorted, labels, static_cast<const gsim_hit*>(label_best), kk,
                       static_cast<gsim_hit*>(hits), hit_labels);
    return hipGetLastError();
}

} // namespace gsim
