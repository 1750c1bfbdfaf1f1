// capi_linkage.cpp -- gsim_db_linkage (complete- and average-linkage dendrograms of a range of rows: the dense matrix from the
// matrix-core score pass, the nearest-neighbour chain on the device, the replay into greedy order on the host) and its host twin
// gsim_linkage (the same chain on a matrix in host memory).  The argument checks, the matrix slabs and the launch loop of a call;
// the device side is gsim_linkage.hip.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 31.
#include "capi_front.h"

#include <queue>

namespace gsim_host
{
namespace
{

using gsim::LinkRaw;
typedef unsigned __int128 u128;

// A chain step, measured on Morgan-shaped 1024-bit rows (profiles/linkage_time.txt; a third of the steps are
// merges, whose rows and column are in the figure): 4.0 / 7.8 / 27 us at n = 4096 / 16 384 / 65 536 with complete linkage, 7.0 / 12.5 /
// 48 us with average linkage -- about kLinkStepBaseUs plus the bytes a scan reads (the row and the 4-byte sizes) at
// kLinkStepBytesPerUs.  A launch of launch_steps = 0 is sized to kLinkLaunchUs, the 5 ms the score launches are priced at.
constexpr double kLinkStepBaseUs = 3.0;
constexpr double kLinkStepBytesPerUs = 18000.0;
constexpr double kLinkLaunchUs = 5000.0;

uint32_t auto_launch_steps(uint64_t n, bool average)
{
    const double us = kLinkStepBaseUs + static_cast<double>(n * (average ? 12 : 8)) / kLinkStepBytesPerUs;
    return static_cast<uint32_t>(std::max(kLinkLaunchUs / us, 1.0));
}

// does raw merge x come before y in ORDER L: similarity descending -- complete linkage: the f32's bits, average linkage: the exact
// fractions v / (size_a size_b), cross-multiplied --, then a, then b
bool raw_before(const LinkRaw& x, const LinkRaw& y, bool average)
{
    if (average) {
        const u128 l = static_cast<u128>(x.v) * (static_cast<uint64_t>(y.size_a) * y.size_b);
        const u128 r = static_cast<u128>(y.v) * (static_cast<uint64_t>(x.size_a) * x.size_b);
        if (l != r) return l > r;
    } else if (x.v != y.v) {
        return x.v > y.v;
    }
    if (x.a != y.a) return x.a < y.a;
    return x.b < y.b;
}

// The n - 1 merges the chain executed, in the order the greedy rule executes them: among the merges whose two clusters exist, the
// one first in L (every executed merge was of a reciprocal pair, which stays one while others merge: DESIGN.md section 31).
// `offset` is added to a and b.  STATE when the list is not a dendrogram of n leaves.
int replay_in_order(const std::vector<LinkRaw>& raw, uint64_t n, bool average, uint32_t offset, gsim_linkage_merge* merges)
{
    const size_t nm = raw.size();
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> last(n, kNone), next(nm, kNone), waits(nm, 0), id(n), size(n, 1);
    for (size_t r = 0; r < nm; r++) {
        const LinkRaw& m = raw[r];
        if (!(m.a < m.b) || m.b >= n || m.size_a == 0 || m.size_b == 0) return fail(GSIM_ERR_STATE, "linkage: the chain reported an impossible merge");
        for (const uint32_t slot : {m.a, m.b})
            if (last[slot] != kNone) {
                next[last[slot]] = static_cast<uint32_t>(r);
                waits[r]++;
            }
        last[m.a] = static_cast<uint32_t>(r);
        last[m.b] = kNone;
    }
    auto later = [&](uint32_t x, uint32_t y) { return raw_before(raw[y], raw[x], average); };
    std::priority_queue<uint32_t, std::vector<uint32_t>, decltype(later)> ready(later);
    for (size_t r = 0; r < nm; r++)
        if (waits[r] == 0) ready.push(static_cast<uint32_t>(r));
    for (uint64_t i = 0; i < n; i++) id[i] = static_cast<uint32_t>(i);
    size_t out = 0;
    while (!ready.empty()) {
        const uint32_t r = ready.top();
        ready.pop();
        const LinkRaw& m = raw[r];
        if (size[m.a] != m.size_a || size[m.b] != m.size_b) return fail(GSIM_ERR_STATE, "linkage: the chain's cluster sizes do not add up");
        gsim_linkage_merge g{};
        g.a = m.a + offset;
        g.b = m.b + offset;
        g.left = id[m.a];
        g.right = id[m.b];
        g.size = m.size_a + m.size_b;
        if (average) {
            const uint64_t pairs = static_cast<uint64_t>(m.size_a) * m.size_b;
            g.sum_q = m.v;
            g.score = static_cast<float>((static_cast<double>(m.v) / static_cast<double>(pairs)) * 0x1p-31);
        } else {
            const uint32_t bits = static_cast<uint32_t>(m.v);
            std::memcpy(&g.score, &bits, 4);
            g.sum_q = static_cast<uint32_t>(g.score * 2147483648.0f); // (exact product, truncating conversion: q)
        }
        if (out && g.score > merges[out - 1].score) return fail(GSIM_ERR_STATE, "linkage: a merge above its predecessor");
        merges[out] = g;
        id[m.a] = static_cast<uint32_t>(n + out);
        size[m.a] = g.size;
        size[m.b] = 0;
        out++;
        if (next[r] != kNone && --waits[next[r]] == 0) ready.push(next[r]);
    }
    if (out != nm) return fail(GSIM_ERR_STATE, "linkage: the chain's merges do not form a dendrogram");
    return GSIM_OK;
}

// ---- the chain on the host: what link_chain_kernel does, one entry at a time ----

inline bool cand_before(uint64_t v, uint32_t size, uint32_t idx, uint64_t bv, uint32_t bsize, uint32_t bidx, bool average)
{
    if (average) {
        const u128 l = static_cast<u128>(v) * bsize, r = static_cast<u128>(bv) * size;
        if (l != r) return l > r;
    } else if (v != bv) {
        return v > bv;
    }
    return idx < bidx;
}

// mat: n x n, symmetric (the bits of the scores, or q of them)
template <class T> void host_chain(std::vector<T>& mat, uint64_t n, bool average, std::vector<LinkRaw>& raw, uint64_t* scans)
{
    std::vector<uint32_t> size(n, 1), chain;
    chain.reserve(64);
    uint64_t nscans = 0;
    while (raw.size() + 1 < n) {
        if (chain.empty()) chain.push_back(0); // the lowest live slot: slot 0 never dies
        const uint32_t tip = chain.back();
        const T* row = mat.data() + static_cast<size_t>(tip) * n;
        uint64_t bv = 0;
        uint32_t bsize = 1, by = 0xFFFFFFFFu;
        for (uint32_t y = 0; y < n; y++)
            if (size[y] != 0 && y != tip && cand_before(row[y], size[y], y, bv, bsize, by, average)) {
                bv = row[y];
                bsize = size[y];
                by = y;
            }
        nscans++;
        if (chain.size() >= 2 && chain[chain.size() - 2] == by) {
            const uint32_t lo = std::min(tip, by), hi = std::max(tip, by);
            T* row_lo = mat.data() + static_cast<size_t>(lo) * n;
            const T* row_hi = mat.data() + static_cast<size_t>(hi) * n;
            for (uint32_t z = 0; z < n; z++)
                if (size[z] != 0 && z != lo && z != hi) {
                    row_lo[z] = average ? static_cast<T>(row_lo[z] + row_hi[z]) : std::min(row_lo[z], row_hi[z]);
                    mat[static_cast<size_t>(z) * n + lo] = row_lo[z];
                }
            raw.push_back(LinkRaw{lo, hi, size[lo], size[hi], bv});
            size[lo] += size[hi];
            size[hi] = 0;
            chain.pop_back();
            chain.pop_back();
        } else {
            chain.push_back(by);
        }
    }
    if (scans) *scans = nscans;
}

template <class T> int host_linkage(const float* scores, uint64_t n, uint64_t ld, bool average, gsim_linkage_merge* merges, uint64_t* scans)
{
    std::vector<T> mat(static_cast<size_t>(n) * n, 0);
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t j = i + 1; j < n; j++) {
            const float s = scores[i * ld + j] + 0.0f; // (-0.0f becomes 0.0f)
            uint32_t bits;
            std::memcpy(&bits, &s, 4);
            const T v = average ? static_cast<T>(static_cast<uint32_t>(s * 2147483648.0f)) : static_cast<T>(bits);
            mat[i * n + j] = v;
            mat[j * n + i] = v;
        }
    std::vector<LinkRaw> raw;
    raw.reserve(n - 1);
    host_chain(mat, n, average, raw, scans);
    return replay_in_order(raw, n, average, 0, merges);
}

// ---- the call on the device ----

struct LinkCall {
    uint64_t rb, n; // the table rows [rb, rb + n), n >= 2
    bool average;
    int metric;
    float alpha, beta;
    uint32_t launch_steps;
};

int linkage(gsim_db* db, Shard& s, const LinkCall& c, gsim_linkage_merge* merges, gsim_linkage_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    gsim_linkage_stats ls{};
    const uint64_t n = c.n, n4 = (n + 3) & ~uint64_t{3};
    ls.rows = n;
    ls.merges = n - 1;
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    auto drain = [&](int rc) { // (nothing of the call is still running when its buffers go)
        (void) hipStreamSynchronize(st);
        return rc;
    };

    DevBuf<> mat;
    DevBuf<float> stage;
    DevBuf<uint32_t> size, chain;
    DevBuf<LinkRaw> d_raw;
    DevBuf<unsigned long long> ctl;
    GSIM_ALLOC(mat, n * n4 * (c.average ? 8 : 4), "the linkage (the matrix)");
    // average linkage: slabs of whole rows, whole mirror tiles
    uint64_t slab_rows = n;
    if (c.average) {
        const uint64_t tile = gsim::kLinkTile;
        slab_rows = std::max<uint64_t>(static_cast<uint64_t>(db->knobs.scores_stage_bytes) / (n4 * 4) / tile * tile, tile);
        slab_rows = std::min(slab_rows, n);
        GSIM_ALLOC(stage, slab_rows * n4 * 4, "the linkage (staging slab)");
    }
    GSIM_ALLOC(size, n4 * 4, "the linkage (cluster sizes)");
    GSIM_ALLOC(chain, n * 4, "the linkage (the chain)");
    GSIM_ALLOC(d_raw, (n - 1) * sizeof(LinkRaw), "the linkage (executed merges)");
    GSIM_ALLOC(ctl, gsim::kLinkCtlWords * 8, "the linkage (control block)");

    gsim::LinkArgs a{};
    a.mat = mat;
    a.ld = n4;
    a.n = static_cast<uint32_t>(n);
    a.average = c.average ? 1 : 0;
    a.size = size;
    a.chain = chain;
    a.raw = d_raw;
    a.ctl = ctl;

    // ---- the matrix ----
    const uint32_t* d_rows = static_cast<const uint32_t*>(s.d_rows) + c.rb * s.W;
    GSIM_HIP(gsim::launch_link_init(a, st));
    if (!c.average) {
        const ScoresCall sc{c.rb, n, c.metric, c.alpha, c.beta, nullptr, mat.as<float>(), n4, nullptr};
        if (const int rc = scores(db, s, d_rows, n, sc)) return drain(rc);
        GSIM_HIP(gsim::launch_link_mirror(a, mat.as<float>(), n4, 0, 0, n, st));
    } else {
        for (uint64_t first = 0; first < n; first += slab_rows) {
            // rows [first, first + rows) against the rows from `first` on: nothing below the diagonal is read
            const uint64_t rows = std::min(slab_rows, n - first);
            const ScoresCall sc{c.rb + first, n - first, c.metric, c.alpha, c.beta, nullptr, stage, n4, nullptr};
            if (const int rc = scores(db, s, d_rows + first * s.W, rows, sc)) return drain(rc);
            const hipError_t e = gsim::launch_link_mirror(a, stage, n4, first, first, rows, st);
            if (e != hipSuccess) return drain(fail_hip(e, "launch_link_mirror"));
            // (the next slab's scores overwrite the staging memory: on the same stream, behind this kernel)
        }
    }
    GSIM_HIP(hipStreamSynchronize(st));
    ls.matrix_ms = ms_since(t0);

    // ---- the chain: at most 3 n scans (an element is pushed by a scan and leaves in a merge; a merge takes a scan) ----
    const auto t1 = std::chrono::steady_clock::now();
    const uint32_t steps = c.launch_steps ? c.launch_steps : auto_launch_steps(n, c.average);
    ls.launch_steps = steps;
    const uint64_t max_launches = (3 * n + steps - 1) / steps + 1;
    LaunchClocks clocks;
    unsigned long long h_ctl[gsim::kLinkCtlWords] = {};
    for (uint64_t l = 0; l < max_launches && !h_ctl[gsim::kLinkCtlDone]; l++) {
        const hipError_t e = gsim::launch_link_chain(a, steps, st);
        if (e != hipSuccess) return drain(fail_hip(e, "launch_link_chain"));
        GSIM_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipStreamSynchronize(st));
        clocks.add(h_ctl + gsim::kLinkCtlClk, 1);
        ls.launches++;
    }
    if (h_ctl[gsim::kLinkCtlDone] != 1 || h_ctl[gsim::kLinkCtlMerged] != n - 1)
        return fail(GSIM_ERR_STATE, "linkage: the chain did not finish within the scans a dendrogram of this many rows can take");
    ls.scans = h_ctl[gsim::kLinkCtlScans];
    ls.chain_max = h_ctl[gsim::kLinkCtlChainMax];
    ls.chain_ms = ms_since(t1);

    const auto t2 = std::chrono::steady_clock::now();
    std::vector<LinkRaw> raw(n - 1);
    GSIM_HIP(hipMemcpyAsync(raw.data(), d_raw, (n - 1) * sizeof(LinkRaw), hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    ls.d2h_ms = ms_since(t2);

    const auto t3 = std::chrono::steady_clock::now();
    if (const int rc = replay_in_order(raw, n, c.average, static_cast<uint32_t>(c.rb) + db->row_base, merges)) return rc;
    ls.order_ms = ms_since(t3);
    ls.clock_mhz = clocks.mhz();
    ls.wall_ms = ms_since(t0);
    if (stats) *stats = ls;
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_linkage(gsim_db* db, uint64_t row_begin, uint64_t row_end, int linkage_kind, int metric, float alpha, float beta, uint32_t launch_steps,
                    gsim_linkage_merge* merges, uint64_t* nmerges, gsim_linkage_stats* stats)
{
    if (stats) *stats = gsim_linkage_stats{};
    if (nmerges) *nmerges = 0;
    if (!db || !nmerges) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_row_range(db, row_begin, row_end)) return rc;
    const uint64_t n = row_end - row_begin;
    if (n > GSIM_LINKAGE_MAX_ROWS) return fail(GSIM_ERR_INVALID, "linkage: more than 65536 rows");
    if (linkage_kind != GSIM_LINKAGE_COMPLETE && linkage_kind != GSIM_LINKAGE_AVERAGE) return fail(GSIM_ERR_INVALID, "linkage: unknown linkage");
    if (const int rc = check_symmetric_metric("linkage needs", "linkage", metric, alpha, beta)) return rc;
    if (db->fp_bits > 4096 || gsim::scores_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "linkage: rows wider than 4096 bits");
    if (n > 1 && !merges) return fail(GSIM_ERR_INVALID, "NULL merges");
    if (n <= 1) {
        if (stats) stats->rows = n;
        return GSIM_OK;
    }
    if (const int rc = check_table_state(db, "linkage", false)) return rc;
    const LinkCall call{row_begin, n, linkage_kind == GSIM_LINKAGE_AVERAGE, metric, alpha, beta, launch_steps};
    const int rc = on_one_shard(db, "host memory for the linkage", [&](Shard& s) { return linkage(db, s, call, merges, stats); });
    if (rc == GSIM_OK) *nmerges = n - 1;
    return rc;
}

int gsim_linkage(const float* scores, uint64_t n, uint64_t ld, int linkage_kind, gsim_linkage_merge* merges, uint64_t* nmerges, uint64_t* scans)
{
    if (nmerges) *nmerges = 0;
    if (scans) *scans = 0;
    if (!nmerges) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (n > GSIM_LINKAGE_MAX_ROWS) return fail(GSIM_ERR_INVALID, "linkage: more than 65536 rows");
    if (linkage_kind != GSIM_LINKAGE_COMPLETE && linkage_kind != GSIM_LINKAGE_AVERAGE) return fail(GSIM_ERR_INVALID, "linkage: unknown linkage");
    if (ld < n) return fail(GSIM_ERR_INVALID, "linkage: ld is less than n");
    if (n > 1 && (!scores || !merges)) return fail(GSIM_ERR_INVALID, "NULL scores or merges");
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t j = i + 1; j < n; j++)
            if (!(scores[i * ld + j] >= 0.0f && scores[i * ld + j] <= 1.0f)) return fail(GSIM_ERR_INVALID, "linkage: a score that is NaN or outside [0, 1]");
    if (n <= 1) return GSIM_OK;
    try {
        const bool average = linkage_kind == GSIM_LINKAGE_AVERAGE;
        const int rc = average ? host_linkage<uint64_t>(scores, n, ld, true, merges, scans) : host_linkage<uint32_t>(scores, n, ld, false, merges, scans);
        if (rc != GSIM_OK) return rc;
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "linkage");
    }
    *nmerges = n - 1;
    return GSIM_OK;
}

} // extern "C"
