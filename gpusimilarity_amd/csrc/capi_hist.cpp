// capi_hist.cpp -- gsim_db_histogram / gsim_db_histogram_queries: per left row, how many table rows score in each bin.  The
// family's argument checks, the launch plans of both routes and one core that takes a front's LeftSide (capi_front.h), as the
// joins, with the copies of a call.  The device side is gsim_hist.hip.  The rule is stated in include/gpusim_hip.h.
#include "capi_front.h"
#include "gsim_prefilter.h"


namespace gsim_host
{
namespace
{

// Bytes of table rows one launch of a streaming pass reads at most: as a join's pass
constexpr uint64_t kHistLaunchBytes = (256ull << 20) * 128ull;

struct PassPiece {
    uint64_t r0, nrows;
    gsim::ScanGeometry g;
};

// The launches of a pass over N rows of W words: a multiple of 64 rows each (launch starts stay 16-byte aligned for every width);
// `pairs` > 0 (GSIM_HIST_LAUNCH_PAIRS): at most that many rows -- a pass scores one left row against them -- and at least 64.
std::vector<PassPiece> plan_passes(uint64_t N, uint32_t W, int num_cus, long long pairs)
{
    uint64_t per = kHistLaunchBytes / (static_cast<uint64_t>(W) * 4u);
    if (pairs > 0) per = std::min<uint64_t>(per, static_cast<uint64_t>(pairs));
    per = std::max<uint64_t>(per / 64 * 64, 64);
    std::vector<PassPiece> out;
    for (uint64_t r0 = 0; r0 < N; r0 += per) {
        PassPiece p{r0, std::min(per, N - r0), {}};
        p.g = gsim::maxmin_geometry(p.nrows, W, num_cus);
        out.push_back(p);
    }
    return out;
}

struct HistLaunch {
    uint32_t ot0, not_; // owner tiles
    uint64_t c0, c1;    // table rows
    uint32_t chunk;     // ... of which a workgroup takes this many
};

// The tile launches of a call over nl owners and N table rows of WP words.  A launch is a group of owner tiles x a range of
// columns within the tile kernel's budget (launch_tile_budget: the same pricing, the same 2.5e11 units, as gsim_db_knn);
// `pairs` > 0 (GSIM_HIST_LAUNCH_PAIRS) replaces the budget: at most that many owner x table-row pairs, at least one 256 x 256
// tile.  Inside a launch the columns are split into chunks so that about eight workgroups per CU exist where the work allows
// it, never more than kHistMaxChunk rows to a chunk (the kernel's 16-bit counters) nor 65 535 chunks to a launch.
std::vector<HistLaunch> plan_tiles(uint64_t nl, uint64_t N, uint32_t WP, long long pairs, int num_cus)
{
    const uint64_t tile = gsim::kHistTile, ctile = gsim::kHistColTile;
    const uint64_t not_total = (nl + tile - 1) / tile;
    const uint64_t max_tiles = pairs > 0 ? std::max<uint64_t>(static_cast<uint64_t>(pairs) / (tile * ctile), 1) : launch_tile_budget(WP);
    const uint64_t group = std::min<uint64_t>(std::min(not_total, max_tiles), 1u << 30);
    const uint64_t want = 8u * static_cast<uint64_t>(std::max(num_cus, 1));
    std::vector<HistLaunch> out;
    for (uint64_t t0 = 0; t0 < not_total; t0 += group) {
        const uint64_t nt = std::min(group, not_total - t0);
        uint64_t cols = std::max(max_tiles / nt * ctile, ctile);
        const uint64_t span = std::min(cols, N);
        const uint64_t per_tile = (want + nt - 1) / nt; // chunks wanted per owner tile
        uint64_t chunk = ((span + per_tile - 1) / per_tile + ctile - 1) / ctile * ctile;
        chunk = std::min<uint64_t>(std::max(chunk, ctile), gsim::kHistMaxChunk);
        cols = std::min<uint64_t>(cols, 65535u * chunk);
        for (uint64_t c0 = 0; c0 < N; c0 += cols)
            out.push_back({static_cast<uint32_t>(t0), static_cast<uint32_t>(nt), c0, std::min(c0 + cols, N), static_cast<uint32_t>(chunk)});
    }
    return out;
}

struct HistCall {
    const float* edges;
    uint32_t nedges;
    int metric;
    float alpha, beta;
    uint64_t self0; // GSIM_HIST_EXCLUDE_SELF: left row o is table row self0 + o; ~0: no pair is excluded
    uint64_t* hist;
    uint64_t* total;
    gsim_hist_stats* stats;
};

// the left rows (W words each, on s's device) against s's table
int histogram(gsim_db* db, Shard& s, const LeftSide& ls, const HistCall& c)
{
    const auto t0 = std::chrono::steady_clock::now();
    auto wall = [&] { return ms_since(t0); };
    const uint64_t N = s.nrows, nl = ls.nl;
    const uint32_t nb = c.nedges + 1;
    gsim_hist_stats hs{};
    hs.left_rows = nl;
    std::vector<unsigned long long> h_total(nb, 0);
    if (nl > 0) {
        GSIM_HIP(set_device(s.device));
        const hipStream_t st = s.stream;
        // the coarse table: cell t = the number of edges <= t / 256 (gsim_hist.hip, hist_bin)
        std::vector<uint8_t> coarse(gsim::kHistCoarse);
        for (uint32_t t = 0; t < gsim::kHistCoarse; t++) {
            const float lo = static_cast<float>(t) / static_cast<float>(gsim::kHistCoarse);
            uint32_t n = 0;
            while (n < c.nedges && c.edges[n] <= lo) n++;
            coarse[t] = static_cast<uint8_t>(n);
        }
        DevBuf<unsigned long long> d_hist, d_total;
        DevBuf<> d_bins;
        PaddedRows table, left;
        LaunchClocks clocks;
        GSIM_ALLOC(d_hist, nl * nb * 8, "the histogram's counters");
        GSIM_ALLOC(d_total, static_cast<size_t>(nb) * 8, "the histogram's totals");
        GSIM_ALLOC(d_bins, GSIM_HIST_MAX_EDGES * 4 + gsim::kHistCoarse, "the histogram's edges");
        GSIM_HIP(hipMemsetAsync(d_hist, 0, nl * nb * 8, st));
        GSIM_HIP(hipMemcpyAsync(d_bins, c.edges, c.nedges * 4, hipMemcpyHostToDevice, st));
        GSIM_HIP(hipMemcpyAsync(d_bins.as<uint8_t>() + GSIM_HIST_MAX_EDGES * 4, coarse.data(), coarse.size(), hipMemcpyHostToDevice, st));
        gsim::HistBins bins{};
        bins.edges = d_bins.as<float>();
        bins.coarse = d_bins.as<uint8_t>() + GSIM_HIST_MAX_EDGES * 4;
        bins.nedges = c.nedges;
        bins.cut_lo = c.edges[0] <= 1.0f ? gsim::valu_cutoff_lo(c.edges[0]) : 0.0f;

        EventPair ev_run, ev_reduce, ev_d2h;
        GSIM_HIP(ev_run.create());
        GSIM_HIP(ev_reduce.create());
        GSIM_HIP(ev_d2h.create());
        const bool stream = db->knobs.hist_stream_max_rows > 0 && nl <= static_cast<uint64_t>(db->knobs.hist_stream_max_rows);
        if (N == 0) {
            GSIM_HIP(hipEventRecord(ev_run.a, st));
            GSIM_HIP(hipEventRecord(ev_run.b, st));
        } else if (stream) {
            const std::vector<PassPiece> pieces = plan_passes(N, s.W, s.num_cus, db->knobs.hist_launch_pairs);
            gsim::HistStreamArgs h{};
            h.rows = s.d_rows;
            h.W = s.W;
            h.metric = c.metric;
            h.alpha = c.alpha;
            h.beta = c.beta;
            h.left = ls.rows;
            h.self0 = c.self0;
            h.bins = bins;
            h.hist = d_hist;
            h.naive = db->knobs.hist_naive_add;
            GSIM_HIP(hipEventRecord(ev_run.a, st));
            for (uint64_t l = 0; l < nl; l++)
                for (const PassPiece& p : pieces) GSIM_HIP(gsim::launch_hist_pass(h, p.g, p.r0, p.nrows, static_cast<uint32_t>(l), st));
            GSIM_HIP(hipEventRecord(ev_run.b, st));
            hs.rows_streamed = nl;
            hs.stream_launches = nl * pieces.size();
        } else {
            // popc of every table row, and the rows of either side zero-padded to WP words unless they already are WP words
            const uint32_t WP = gsim::nbr_padded_words(s.W);
            if (const int rc = table.alloc(N, s.W, WP, "the histogram (popcounts)", "the histogram (padded rows)")) return rc;
            if (const int rc = table.prepare(s.d_rows, N, st)) return rc;
            // (the kernel counts the left rows' bits itself: only their padded copy is wanted, where the table's does not hold them)
            const uint32_t* lrows = ls.rows;
            if (WP != s.W) {
                if (ls.in_table) {
                    lrows = table.rows() + ls.row0 * WP;
                } else {
                    if (const int rc = left.alloc(nl, s.W, WP, "the histogram (popcounts of the left rows)", "the histogram (padded left rows)")) return rc;
                    if (const int rc = left.prepare(ls.rows, nl, st)) return rc;
                    lrows = left.rows();
                }
            }
            const std::vector<HistLaunch> plan = plan_tiles(nl, N, WP, db->knobs.hist_launch_pairs, s.num_cus);
            if (const int rc = clocks.own(plan.size(), "the histogram (clock stamps)")) return rc;
            GSIM_HIP(clocks.zero(plan.size(), st));
            gsim::HistTileArgs a{};
            a.rows = table.rows();
            a.pop = table.pop();
            a.lrows = lrows;
            a.nrows = N;
            a.nl = nl;
            a.WP = WP;
            a.metric = c.metric;
            a.alpha = c.alpha;
            a.beta = c.beta;
            a.self0 = c.self0;
            a.bins = bins;
            a.hist = d_hist;
            GSIM_HIP(hipEventRecord(ev_run.a, st));
            for (size_t l = 0; l < plan.size(); l++) {
                a.clk = clocks.at(l);
                GSIM_HIP(gsim::launch_hist_tiles(a, plan[l].ot0, plan[l].not_, plan[l].c0, plan[l].c1, plan[l].chunk, st));
            }
            GSIM_HIP(hipEventRecord(ev_run.b, st));
            GSIM_HIP(clocks.fetch(plan.size(), st));
            hs.rows_tiled = nl;
            hs.tile_launches = plan.size();
        }
        GSIM_HIP(hipEventRecord(ev_reduce.a, st));
        GSIM_HIP(gsim::launch_hist_total(d_hist, nl, nb, d_total, st));
        GSIM_HIP(hipEventRecord(ev_reduce.b, st));
        // only what was asked for (and the nb totals: stats.pairs is their sum)
        GSIM_HIP(hipEventRecord(ev_d2h.a, st));
        if (c.hist) GSIM_HIP(hipMemcpyAsync(c.hist, d_hist, nl * nb * 8, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipMemcpyAsync(h_total.data(), d_total, static_cast<size_t>(nb) * 8, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipEventRecord(ev_d2h.b, st));
        GSIM_HIP(hipStreamSynchronize(st));
        clocks.add(); // (nothing on the streaming route)
        hs.clock_mhz = clocks.mhz();
        (stream ? hs.stream_ms : hs.tile_ms) = ev_run.ms();
        hs.reduce_ms = ev_reduce.ms();
        hs.d2h_ms = ev_d2h.ms();
    }
    for (uint32_t b = 0; b < nb; b++) {
        hs.pairs += h_total[b];
        if (c.total) c.total[b] = h_total[b];
    }
    hs.wall_ms = wall();
    if (c.stats) *c.stats = hs;
    return GSIM_OK;
}

// what both entry points check before any device state
int check_hist_args(gsim_db* db, uint64_t nl, const HistCall& c, uint32_t flags)
{
    if (!db) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_metric("histogram", c.metric, c.alpha, c.beta)) return rc;
    if (!c.edges) return fail(GSIM_ERR_INVALID, "histogram: NULL edges");
    if (c.nedges < 1 || c.nedges > GSIM_HIST_MAX_EDGES) return fail(GSIM_ERR_INVALID, "histogram: nedges must be in [1, GSIM_HIST_MAX_EDGES = 128]");
    for (uint32_t i = 0; i < c.nedges; i++) {
        if (!std::isfinite(c.edges[i])) return fail(GSIM_ERR_INVALID, "histogram: an edge is not finite");
        if (i == 0 ? !(c.edges[0] > 0.0f) : !(c.edges[i] > c.edges[i - 1]))
            return fail(GSIM_ERR_INVALID, "histogram: the edges must be strictly ascending and > 0");
    }
    if (!c.hist && !c.total) return fail(GSIM_ERR_INVALID, "histogram: both outputs are NULL");
    if (flags & ~GSIM_HIST_EXCLUDE_SELF) return fail(GSIM_ERR_INVALID, "histogram: unknown flag bits");
    if (nl > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "histogram: 2^32 left rows or more");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "histogram: tables of 2^32 rows or more");
    if (gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "histograms support rows of up to 4096 bits");
    return GSIM_OK;
}

int run_histogram(gsim_db* db, const LeftSide& left, const HistCall& c)
{
    try {
        return histogram(db, db->shards[0], left, c);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "host memory for the histogram");
    }
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_histogram_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, const float* edges, uint32_t nedges, int metric, float alpha,
                              float beta, uint64_t* hist, uint64_t* total, gsim_hist_stats* stats)
{
    const HistCall c{edges, nedges, metric, alpha, beta, ~0ull, hist, total, stats};
    int rc = check_hist_args(db, nq, c, 0);
    if (rc != GSIM_OK) return rc;
    LeftSide left;
    rc = left.from_queries(db, queries, nq, "histograms", "the histogram's left rows");
    if (rc != GSIM_OK) return rc;
    return run_histogram(db, left, c);
}

int gsim_db_histogram(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, const float* edges, uint32_t nedges, int metric,
                      float alpha, float beta, uint32_t flags, uint64_t* hist, uint64_t* total, gsim_hist_stats* stats)
{
    if (lrow_begin > lrow_end) return fail(GSIM_ERR_INVALID, "left row range: begin past end");
    const bool exclude = (flags & GSIM_HIST_EXCLUDE_SELF) != 0;
    const HistCall c{edges, nedges, metric, alpha, beta, exclude ? lrow_begin : ~0ull, hist, total, stats};
    int rc = check_hist_args(db, lrow_end - lrow_begin, c, flags);
    if (rc != GSIM_OK) return rc;
    if (exclude && left && left != db) return fail(GSIM_ERR_INVALID, "histogram: GSIM_HIST_EXCLUDE_SELF needs left == db");
    rc = check_left_handle(db, left, lrow_end);
    if (rc != GSIM_OK) return rc;
    LeftSide ls;
    rc = ls.from_handle(db, left, lrow_begin, lrow_end, "histograms");
    if (rc != GSIM_OK) return rc;
    return run_histogram(db, ls, c);
}

} // extern "C"
