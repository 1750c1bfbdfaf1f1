// gsim_subset.hip -- row sets (gsim_rowset_*, gsim_db_search_rows): exact top-k restricted to a subset of the table.
//
// A row set on the device is a bitmap (one bit per table row, bit r % 32 of word r / 32) and the ascending list of the selected
// rows (4 B each, without the row base).  Both are built here: the caller's rows are marked with atomic ORs (duplicates
// collapse), or the caller's bitmap is copied; GSIM_ROWSET_EXCLUDE inverts; the bits past the last row are cleared; the list
// is the bitmap expanded at the exclusive prefix sums (launch_scan_u32) of its words' popcounts -- ascending by construction.
//
// Two scans feed the four-kernel pipeline's tail (compact_kernel -> select_kernel, or the large-k select and sort) with exactly
// what scan_kernel leaves: per-wave candidate segments, seg_count, QueryState::ghist / kept / ncand, the gate convention.
//   subset_scan_kernel   (dense sets) the table streamed through the scan's own loops (gsim_scan_inl.h, join_kernel's dispatch)
//                        with Masked<WaveFilter>: the rows of one offer are 64 consecutive rows, their mask bits are three
//                        consecutive words fetched with wave-uniform SCALAR loads (constant address space: they count on
//                        lgkmcnt, the loop's vmcnt queue holds the prefetched chunk and nothing else) -- in the power-of-two
//                        loop a trip ahead of their use; unselected rows are inactive before WaveFilter sees them; a round
//                        with no selected row issues nothing.
//   subset_gather_kernel (sparse sets) a wave walks the list: every group of LPR lanes loads one selected row (16 B per lane,
//                        rows + list[i] * LPR + sub), U loads per lane per chunk, the next chunk's loads and the indices of the
//                        one after it in flight while the current one is reduced (reduce_listed, gsim_row_units.h); rows are
//                        offered under their real numbers.  Widths without a power-of-two number of 16-byte units: one row per
//                        lane (listed_lane_kernel<false>, gsim_row_units.h).
// Seeding: none.  Both scans start from gtau = 0 ("emit everything") and raise the threshold through ghist, which only ever
// counts selected rows; sample_kernel's seed counts rows of the whole table and may lie above the subset's k-th best.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include "../../include/gpusim_hip.h"
#include "gsim_device_common.h"
#include "gsim_filter_inl.h"
#include "gsim_row_units.h"
#include "gsim_scan_inl.h"

namespace gsim
{
namespace
{

// ---------------------------------------------------------------------------
// building a row set
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rowset_mark_kernel(const uint32_t* __restrict__ rows, u64 n, uint32_t row_base, u64 nrows,
                                                          uint32_t* __restrict__ bits)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= n) return;
    const uint32_t r = rows[t] - row_base;
    if (r < nrows) atomicOr(&bits[r >> 5], 1u << (r & 31u)); // (the host has checked the range: never false)
}

// words [0, nalloc): the set's final bitmap (src: the caller's words, or null: what the marks left), inverted for an exclusion
// set, zero past the last row; popc[t] = popc(word t) for the prefix sums (nalloc > nwords: popc[nwords] = 0 closes them)
__global__ __launch_bounds__(256) void rowset_finish_kernel(uint32_t* __restrict__ bits, const uint32_t* __restrict__ src, u64 nrows,
                                                            u64 nwords, u64 nalloc, int invert, uint32_t* __restrict__ popc)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= nalloc) return;
    uint32_t w = 0;
    if (t < nwords) {
        w = src ? src[t] : bits[t];
        if (invert) w = ~w;
        if (t == nwords - 1 && (nrows & 31u) != 0) w &= (1u << (nrows & 31u)) - 1u;
    }
    bits[t] = w;
    if (t <= nwords) popc[t] = static_cast<uint32_t>(__popc(w));
}

__global__ __launch_bounds__(256) void rowset_list_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ offs, u64 nwords,
                                                          uint32_t* __restrict__ list)
{
    const u64 t = static_cast<u64>(blockIdx.x) * 256u + threadIdx.x;
    if (t >= nwords) return;
    uint32_t w = bits[t];
    uint32_t o = offs[t];
    while (w) {
        list[o++] = static_cast<uint32_t>(t * 32u) + static_cast<uint32_t>(__ffs(static_cast<int>(w)) - 1);
        w &= w - 1u;
    }
}

// ---------------------------------------------------------------------------
// streaming route
// ---------------------------------------------------------------------------

typedef const __attribute__((address_space(4))) uint32_t* MaskWords; // constant address space: wave-uniform reads are scalar loads

// Filter adaptor of the streaming loops: a row that is not in the set is inactive before the inner filter sees it.
// Every loop offers 64 consecutive rows at a time, lane 0 the first of them (reduce_chunk: row0 + 64 r + sub * RPL + grp; the
// others: row0 + lane), under wave-uniform control flow -- so the mask of an offer is bits [first, first + 64) of the bitmap.
// NARROW: the inner filter may take its narrow-row shortcut (WaveFilter's division-free test is proven up to 512 bits: only the
// power-of-two loop passes its width on; the others offer as scan_rows_ragged does).
template <typename Inner, bool NARROW, uint32_t CH> struct Masked {
    static constexpr bool kFused = Inner::kFused;
    Inner in;
    MaskWords bits;
    uint32_t last_word; // index of the bitmap's last word (two zero words follow it)
    // CH != 0 (the power-of-two loop, CH rows per chunk): the words of the NEXT offer are fetched while this one is scored -- the
    // next 64 rows of the chunk, or the first 64 of the wave's next chunk, `stride` rows on -- so that a trip does not wait
    // for a scalar load's round trip.  A wrong guess (the loop's last trips) is fetched again on the spot.
    uint32_t stride;
    uint32_t pf_first, pf0, pf1, pf2;

    __device__ __forceinline__ void init_mask(const uint32_t* b, uint32_t last, uint32_t stride_rows)
    {
        bits = (MaskWords) b;
        last_word = last;
        stride = stride_rows;
        pf_first = 0xFFFFFFFFu;
        pf0 = pf1 = pf2 = 0;
    }
    __device__ __forceinline__ void checkpoint(uint32_t trip, int lane) { in.checkpoint(trip, lane); }
    __device__ __forceinline__ uint32_t load_gtau() const { return in.load_gtau(); }
    __device__ __forceinline__ void refresh(uint32_t g, int lane) { in.refresh(g, lane); }

    // the three words that hold bits [first, first + 64)
    // (an offer that starts past the table -- the rounds behind the last row of a partial chunk -- has no active lane: its
    // word index is clamped into the bitmap and what it reads does not matter)
    __device__ __forceinline__ void fetch(uint32_t first, uint32_t& w0, uint32_t& w1, uint32_t& w2) const
    {
        uint32_t wi = first >> 5;
        wi = wi < last_word ? wi : last_word;
        w0 = bits[wi], w1 = bits[wi + 1u], w2 = bits[wi + 2u];
    }

    template <int LPR> __device__ __forceinline__ void offer_counts(bool active, uint32_t row, uint32_t val, const ScanArgs& a, int lane)
    {
        const uint32_t first = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(row)));
        uint32_t w0, w1, w2;
        if constexpr (CH != 0) {
            if (first != pf_first) {
                asm volatile(""); // (keeps this a branch: as a select both fetches would be issued, and waited for, every time)
                fetch(first, pf0, pf1, pf2);
            }
            w0 = pf0, w1 = pf1, w2 = pf2;
            const uint32_t pos = first & (CH - 1u);
            pf_first = pos + 64u < CH ? first + 64u : first - pos + stride;
            fetch(pf_first, pf0, pf1, pf2);
        } else {
            fetch(first, w0, w1, w2);
        }
        const uint32_t sh = first & 31u;
        u64 m = ((static_cast<u64>(w1) << 32) | w0) >> sh;
        if (sh) m |= static_cast<u64>(w2) << (64u - sh);
        if (m == 0) return; // no row of this round is in the set: nothing is scored, nothing issued
        active = active && ((m >> ((row - first) & 63u)) & 1ull) != 0;
        in.template offer_counts<(NARROW ? LPR : 64)>(active, row, val, a, lane);
    }
};

// LDS of one workgroup: the filter and (rows of 3 ... 22 words: scan_rows_wragged) every wave's word area, in one object
template <int NLW> struct SubsetShared {
    BlockFilter filter;
    uint32_t words[kScanBlock / 64][NLW ? NLW * 256 : 1];
};

// KIND 0: scan_rows<LPR, U>; 1: scan_rows_ragged<LPR, U>; 2: scan_rows_wragged<LPR, U> (LPR = words per row); 3: scan_rows_lane.
template <int KIND, int LPR, int U>
__global__ __launch_bounds__(kScanBlock) void subset_scan_kernel(ScanArgs a, ScanGeometry g, const uint32_t* bits, uint32_t last_word)
{
    constexpr int NLW = KIND == 2 ? (LPR % 2 ? LPR : LPR / 2) * U : 0;
    __shared__ SubsetShared<NLW> sh;
    if (a.gate && *a.gate == 0) return;
    const int lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (threadIdx.x >> 6));
    block_filter_init(&sh.filter, a.k, a.state->gtau);

    Masked<WaveFilter, KIND == 0, (KIND == 0 ? U * 64u / (LPR ? LPR : 1) : 0u)> f;
    f.init_mask(bits, last_word, g.nwaves * g.chunk_rows);
    f.in.init(&sh.filter, a.state, a.cand + static_cast<u64>(w) * g.seg_cap, a.cand_cb + static_cast<u64>(w) * g.seg_cap, a.k, a.cutoff);
    if constexpr (KIND == 0) {
        const u32x4 q = reinterpret_cast<const u32x4*>(a.query)[lane % LPR];
        scan_rows<LPR, U>(a, g, f, q, w, lane);
    } else if constexpr (KIND == 1) {
        scan_rows_ragged<LPR, U>(a, g, f, w, lane);
    } else if constexpr (KIND == 2) {
        scan_rows_wragged<LPR, U>(a, g, f, w, lane, sh.words[wv]);
    } else {
        scan_rows_lane(a, g, f, w, lane);
    }
    f.in.finish(w, a, lane);
    block_filter_flush(&sh.filter, a);
}

template <int KIND, int LPR, int U>
hipError_t launch_scan_t(const ScanArgs& a, const ScanGeometry& g, const uint32_t* bits, uint32_t last_word, hipStream_t s)
{
    hipLaunchKernelGGL((subset_scan_kernel<KIND, LPR, U>), dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, a, g, bits, last_word);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// gather route
// ---------------------------------------------------------------------------

// One wavefront over the list: chunks w, w + nwaves, ... of CH = U * 64 / LPR list entries.  Per trip, in this order: the
// indices of the chunk after next (U 4-byte loads, one cache line per wave), the rows of the next chunk (their indices
// arrived a trip ago), then the current chunk is reduced -- waiting for a chunk's indices never waits for the rows issued
// behind them, so U ... 2 U row loads stay in flight per lane throughout.
template <int LPR, int U, typename Filter>
__device__ __forceinline__ void gather_rows(const ScanArgs& a, const ScanGeometry& g, Filter& f, const u32x4& q,
                                            const uint32_t* __restrict__ list, uint32_t nsel, uint32_t w, int lane)
{
    constexpr int RPL = 64 / LPR;
    constexpr int CH = U * RPL;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const u32x4* __restrict__ db = reinterpret_cast<const u32x4*>(a.rows);
    uint32_t gt = 0;
    uint32_t trip = 0;
    const uint32_t wib = w % (kScanBlock / 64);

    const u64 nfull = nsel / CH; // chunks with all CH entries present
    if (w < nfull) {
        const u64 last = w + (nfull - 1 - w) / g.nwaves * g.nwaves; // this wave's last full chunk
        uint32_t ix[U], ixn[U];
        u32x4 nxt[U];
        {
            const uint32_t* p = list + static_cast<u64>(w) * CH + grp;
#pragma unroll
            for (int j = 0; j < U; j++) ix[j] = p[j * RPL];
            const u64 c1 = w + g.nwaves <= last ? w + g.nwaves : last;
            const uint32_t* p1 = list + c1 * CH + grp;
#pragma unroll
            for (int j = 0; j < U; j++) ixn[j] = p1[j * RPL];
#pragma unroll
            for (int j = 0; j < U; j++) nxt[j] = stream_load(db + static_cast<u64>(ix[j]) * LPR + sub);
        }
        for (u64 c = w;; c += g.nwaves) {
            u32x4 d[U];
            uint32_t ixc[U];
#pragma unroll
            for (int j = 0; j < U; j++) {
                d[j] = nxt[j];
                ixc[j] = ix[j];
            }
            // on the final trips the prefetches re-read the last chunk (no branch in the body)
            const u64 cn = c + g.nwaves <= last ? c + g.nwaves : last;
            const u64 cnn = cn + g.nwaves <= last ? cn + g.nwaves : last;
            uint32_t ixnn[U];
            const uint32_t* p2 = list + cnn * CH + grp;
#pragma unroll
            for (int j = 0; j < U; j++) ixnn[j] = p2[j * RPL];
#pragma unroll
            for (int j = 0; j < U; j++) nxt[j] = stream_load(db + static_cast<u64>(ixn[j]) * LPR + sub);
#pragma unroll
            for (int j = 0; j < U; j++) {
                ix[j] = ixn[j];
                ixn[j] = ixnn[j];
            }
            poll_threshold(f, gt, trip, wib, lane);
            reduce_listed<LPR, U, true>(d, ixc, q, c * CH, nsel, a, f, lane);
            if (c == last) break;
        }
    }
    if (nfull * CH < nsel && w == nfull % g.nwaves) { // the list's partial last chunk
        const u64 e0 = nfull * CH;
        uint32_t ix[U];
        u32x4 d[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const u64 e = e0 + static_cast<u64>(j * RPL + grp);
            ix[j] = e < nsel ? list[e] : 0u;
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            const u64 e = e0 + static_cast<u64>(j * RPL + grp);
            d[j] = e < nsel ? stream_load(db + static_cast<u64>(ix[j]) * LPR + sub) : u32x4{0, 0, 0, 0};
        }
        f.refresh(f.load_gtau(), lane);
        reduce_listed<LPR, U, false>(d, ix, q, e0, nsel, a, f, lane);
    }
}

template <int LPR, int U>
__global__ __launch_bounds__(kScanBlock) void subset_gather_kernel(ScanArgs a, ScanGeometry g, const uint32_t* list, uint32_t nsel)
{
    __shared__ BlockFilter s_filter;
    if (a.gate && *a.gate == 0) return;
    const int lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (kScanBlock / 64) + (threadIdx.x >> 6));
    block_filter_init(&s_filter, a.k, a.state->gtau);
    const u32x4 q = reinterpret_cast<const u32x4*>(a.query)[lane % LPR];
    WaveFilter f;
    f.init(&s_filter, a.state, a.cand + static_cast<u64>(w) * g.seg_cap, a.cand_cb + static_cast<u64>(w) * g.seg_cap, a.k, a.cutoff);
    gather_rows<LPR, U>(a, g, f, q, list, nsel, w, lane);
    f.finish(w, a, lane);
    block_filter_flush(&s_filter, a);
}

template <int LPR, int U>
hipError_t launch_gather_t(const ScanArgs& a, const ScanGeometry& g, const uint32_t* list, uint32_t nsel, hipStream_t s)
{
    hipLaunchKernelGGL((subset_gather_kernel<LPR, U>), dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, a, g, list, nsel);
    return hipGetLastError();
}

// candidate slots per wave: every row of a wave's chunks may be a candidate
void set_seg_cap(ScanGeometry& g)
{
    const uint64_t per = (g.nchunks + g.nwaves - 1) / g.nwaves;
    g.seg_cap = static_cast<uint32_t>((per ? per : 1) * g.chunk_rows);
}

} // namespace

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------

hipError_t launch_rowset_mark(const uint32_t* d_rows, uint64_t n, uint32_t row_base, uint64_t nrows, uint32_t* bits, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rowset_mark_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, d_rows, static_cast<u64>(n), row_base,
                       static_cast<u64>(nrows), bits);
    return hipGetLastError();
}

hipError_t launch_rowset_finish(uint32_t* bits, const uint32_t* src, uint64_t nrows, uint64_t nalloc, int invert, uint32_t* popc, hipStream_t s)
{
    hipLaunchKernelGGL(rowset_finish_kernel, dim3(static_cast<uint32_t>((nalloc + 255) / 256)), dim3(256), 0, s, bits, src, static_cast<u64>(nrows),
                       static_cast<u64>(rowset_words(nrows)), static_cast<u64>(nalloc), invert, popc);
    return hipGetLastError();
}

hipError_t launch_rowset_list(const uint32_t* bits, const uint32_t* offs, uint64_t nwords, uint32_t* list, hipStream_t s)
{
    if (nwords == 0) return hipSuccess;
    hipLaunchKernelGGL(rowset_list_kernel, dim3(static_cast<uint32_t>((nwords + 255) / 256)), dim3(256), 0, s, bits, offs, static_cast<u64>(nwords), list);
    return hipGetLastError();
}

ScanGeometry subset_scan_geometry(uint64_t nrows, uint32_t W, int num_cus)
{
    ScanGeometry g = maxmin_geometry(nrows, W, num_cus);
    set_seg_cap(g);
    return g;
}

ScanGeometry subset_gather_geometry(uint64_t nsel, uint32_t W, int num_cus)
{
    // a "table" of nsel rows, eight waves per CU (two per SIMD: a gathered load waits longer than a streamed one)
    ScanGeometry g = scan_geometry(nsel, W, num_cus, 8, 8); // (a width without a power-of-two lane count: the gather's own geometry, below)
    if (g.lanes_per_row != 0) return g;
    g = ScanGeometry{};
    g.unroll = 1;
    g.chunk_rows = 64;
    g.nchunks = (nsel + 63) / 64;
    uint64_t nw = static_cast<uint64_t>(num_cus) * 8u;
    if (nw > g.nchunks) nw = g.nchunks;
    if (nw < 1) nw = 1;
    g.nwaves = static_cast<uint32_t>((nw + 3) / 4 * 4);
    set_seg_cap(g);
    return g;
}

hipError_t launch_subset_scan(const ScanArgs& a, const ScanGeometry& g, const uint32_t* bits, hipStream_t s)
{
    const uint32_t last_word = static_cast<uint32_t>(rowset_words(a.nrows) - 1);
#define GSIM_CASE(L) \
    if (g.lanes_per_row == L && g.unroll == 8) return launch_scan_t<0, L, 8>(a, g, bits, last_word, s);
    GSIM_CASE(1)
    GSIM_CASE(2)
    GSIM_CASE(4)
    GSIM_CASE(8)
    GSIM_CASE(16)
    GSIM_CASE(32)
    GSIM_CASE(64)
#undef GSIM_CASE
    if (g.lanes_per_row != 0) return hipErrorInvalidValue;
    if (g.ragged_words) {
        switch (a.W) {
        case 3: return launch_scan_t<2, 3, 3>(a, g, bits, last_word, s);
        case 5: return launch_scan_t<2, 5, 2>(a, g, bits, last_word, s);
        case 7: return launch_scan_t<2, 7, 1>(a, g, bits, last_word, s);
        case 6: return launch_scan_t<2, 6, 3>(a, g, bits, last_word, s);
        case 10: return launch_scan_t<2, 10, 2>(a, g, bits, last_word, s);
        case 14: return launch_scan_t<2, 14, 1>(a, g, bits, last_word, s);
        case 9: return launch_scan_t<2, 9, 1>(a, g, bits, last_word, s);
        case 18: return launch_scan_t<2, 18, 1>(a, g, bits, last_word, s);
        case 11: return launch_scan_t<2, 11, 1>(a, g, bits, last_word, s);
        case 22: return launch_scan_t<2, 22, 1>(a, g, bits, last_word, s);
        default: return hipErrorInvalidValue;
        }
    }
    switch (g.ragged_loads) {
    case 0: return launch_scan_t<3, 0, 1>(a, g, bits, last_word, s);
    case 3: return launch_scan_t<1, 3, 3>(a, g, bits, last_word, s);
    case 5: return launch_scan_t<1, 5, 2>(a, g, bits, last_word, s);
    case 7: return launch_scan_t<1, 7, 1>(a, g, bits, last_word, s);
    case 9: return launch_scan_t<1, 9, 1>(a, g, bits, last_word, s);
    case 11: return launch_scan_t<1, 11, 1>(a, g, bits, last_word, s);
    case 13: return launch_scan_t<1, 13, 1>(a, g, bits, last_word, s);
    case 15: return launch_scan_t<1, 15, 1>(a, g, bits, last_word, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_subset_gather(const ScanArgs& a, const ScanGeometry& g, const uint32_t* list, uint32_t nsel, hipStream_t s)
{
    if (g.lanes_per_row != 0) {
        if (g.unroll != 8) return hipErrorInvalidValue;
        return dispatch_lpr(g.lanes_per_row, [&](auto lpr) { return launch_gather_t<decltype(lpr)::value, 8>(a, g, list, nsel, s); });
    }
    hipLaunchKernelGGL(listed_lane_kernel<false>, dim3(g.nwaves / (kScanBlock / 64)), dim3(kScanBlock), 0, s, a, g, list, nsel);
    return hipGetLastError();
}

} // namespace gsim
