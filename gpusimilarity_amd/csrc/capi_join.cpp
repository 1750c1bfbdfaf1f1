// capi_join.cpp -- gsim_db_join / gsim_db_join_queries: every table row at or above a cutoff, per left row.  The family's
// argument checks and one core that takes "left rows in device memory, nl of them" from either front's LeftSide (capi_front.h);
// the device side is gsim_join.hip (streaming route) and the join instantiations of gsim_neighbors.hip's tile kernel.  The rule
// is stated in include/gpusim_hip.h.
#include "capi_front.h"

namespace gsim_host
{

// Bytes of table rows one launch of a streaming pass reads at most: 256 M rows x 128 B, as a MaxMin pass
constexpr uint64_t kJoinLaunchBytes = (256ull << 20) * 128ull;

namespace
{

// Rows per launch of a pass: a multiple of 64 (launch starts stay 16-byte aligned for every width)
uint64_t launch_rows(uint32_t W)
{
    uint64_t r = kJoinLaunchBytes / (static_cast<uint64_t>(W) * 4u);
#ifdef GSIM_TEST_HOOKS
    // GSIM_TEST_JOIN_LAUNCH_ROWS: a short cap, so that the tests run multi-launch passes on small tables
    const int cap = env_int("GSIM_TEST_JOIN_LAUNCH_ROWS", 0);
    if (cap > 0) r = static_cast<uint64_t>(cap);
#endif
    r = r / 64 * 64;
    return r < 64 ? 64 : r;
}

struct PassPiece {
    uint64_t r0, nrows;
    gsim::ScanGeometry g;
};

// left rows d_left[0 .. nl) (W words each, on s's device) against s's table
int join(gsim_db* db, Shard& s, const uint32_t* d_left, uint64_t nl, float cutoff, int metric, float alpha, float beta, int order,
         gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    g->kind = gsim_graph::Kind::kJoin;
    g->indptr.assign(nl + 1, 0);
    if (nl == 0 || N == 0) {
        g->join.wall_ms = g->stats.wall_ms = ms_since(t0);
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const bool stream = db->knobs.join_stream_max_rows > 0 && nl <= static_cast<uint64_t>(db->knobs.join_stream_max_rows);
    PairRun run;
    if (stream) {
        std::vector<PassPiece> pieces;
        const uint64_t per = launch_rows(s.W);
        for (uint64_t r0 = 0; r0 < N; r0 += per) {
            PassPiece p{r0, std::min(per, N - r0), {}};
            p.g = gsim::maxmin_geometry(p.nrows, s.W, s.num_cus);
            pieces.push_back(p);
        }
        const size_t nlaunch = static_cast<size_t>(nl) * pieces.size();
        DevBuf<> ctl; // [0] the cursor, [1 + l] the cursor after launch l
        GSIM_HIP(ctl.grow((1 + nlaunch) * 8));
        gsim::JoinArgs j{};
        j.rows = s.d_rows;
        j.W = s.W;
        j.metric = metric;
        j.alpha = alpha;
        j.beta = beta;
        j.cutoff = cutoff;
        j.left = d_left;
        const int rc = run_pair_launches(s, nlaunch, ctl.as<unsigned long long>(), ctl.as<unsigned long long>() + 1,
                                         [&](size_t l, const PairSink& sink) {
                                             gsim::JoinArgs jl = j;
                                             jl.keys = sink.keys;
                                             jl.vals = sink.vals;
                                             jl.cursor = sink.cursor;
                                             jl.cap = sink.cap;
                                             const PassPiece& p = pieces[l % pieces.size()];
                                             GSIM_HIP(gsim::launch_join_pass(jl, p.g, p.r0, p.nrows, static_cast<uint32_t>(l / pieces.size()), st));
                                             return static_cast<int>(GSIM_OK);
                                         },
                                         &run);
        if (rc != GSIM_OK) return rc;
        g->join.rows_streamed = nl;
        g->join.stream_launches = nlaunch;
        g->join.stream_ms = run.ms;
        g->stats.launches = nlaunch;
    } else {
        // popc of every row of either side, and the rows zero-padded to WP words unless they already are WP words
        const uint32_t WP = gsim::nbr_padded_words(s.W);
        PaddedRows table, left;
        if (const int rc = table.alloc(N, s.W, WP)) return rc;
        if (const int rc = left.alloc(nl, s.W, WP)) return rc;
        if (const int rc = table.prepare(s.d_rows, N, st)) return rc;
        if (const int rc = left.prepare(d_left, nl, st)) return rc;
        const uint64_t nlt = (nl + gsim::kNbrTile - 1) / gsim::kNbrTile;
        const uint64_t nct = (N + gsim::kNbrTile - 1) / gsim::kNbrTile;
        const std::vector<NbrLaunch> plan = plan_launches(nlt, nct, false, WP);
        DevBuf<> ctl; // [0] the cursor, [1 + l] the cursor after launch l, then 4 clock stamps per launch
        GSIM_HIP(ctl.grow((1 + 5 * plan.size()) * 8));
        LaunchClocks clocks;
        clocks.view(ctl.as<unsigned long long>() + 1 + plan.size());
        gsim::JoinTileArgs a{};
        a.rows = table.rows();
        a.pop = table.pop();
        a.lrows = left.rows();
        a.lpop = left.pop();
        a.nrows = N;
        a.row_begin = 0;
        a.row_end = nl;
        a.WP = WP;
        a.metric = metric;
        a.alpha = alpha;
        a.beta = beta;
        a.cutoff = cutoff;
        const int rc = run_pair_launches(s, plan.size(), ctl.as<unsigned long long>(), ctl.as<unsigned long long>() + 1,
                                         [&](size_t l, const PairSink& sink) {
                                             gsim::JoinTileArgs al = a;
                                             al.keys = sink.keys;
                                             al.vals = sink.vals;
                                             al.cursor = sink.cursor;
                                             al.cap = sink.cap;
                                             al.clk = clocks.at(l);
                                             GSIM_HIP(gsim::launch_join_tiles(al, plan[l].rt0, plan[l].nrt, plan[l].ct0, plan[l].nct, st));
                                             return static_cast<int>(GSIM_OK);
                                         },
                                         &run);
        if (rc != GSIM_OK) return rc;
        GSIM_HIP(clocks.fetch(plan.size(), st));
        GSIM_HIP(hipStreamSynchronize(st));
        clocks.add();
        g->join.clock_mhz = g->stats.clock_mhz = clocks.mhz();
        g->join.rows_tiled = nl;
        g->join.tile_launches = plan.size();
        g->join.tile_ms = run.ms;
        g->stats.launches = plan.size();
    }
    g->stats.launches_rerun = g->join.launches_rerun = run.rerun;
    g->stats.pairs = g->join.pairs = run.total;
    g->stats.tile_ms = run.ms;
    const int rc = build_pair_csr(db, s, run.total, nl, order, g);
    if (rc != GSIM_OK) return rc;
    g->join.csr_ms = g->stats.csr_ms;
    g->join.d2h_ms = g->stats.d2h_ms;
    g->join.wall_ms = g->stats.wall_ms = ms_since(t0);
    return GSIM_OK;
}

// what both entry points check before any device state (a NULL db leaves *out as it was: DESIGN.md section 24)
int check_join_args(gsim_db* db, gsim_graph** out, uint64_t nl, float cutoff, int metric, float alpha, float beta, int order)
{
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (const int rc = check_metric("join", metric, alpha, beta)) return rc;
    if (order != GSIM_JOIN_BY_ROW && order != GSIM_JOIN_BY_SCORE) return fail(GSIM_ERR_INVALID, "unknown join order");
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, "join cutoff must be in (0, 1]");
    if (nl > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "join: 2^32 left rows or more");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "join: tables of 2^32 rows or more");
    if (gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "joins support rows of up to 4096 bits");
    return GSIM_OK;
}

int run_join(gsim_db* db, const LeftSide& left, float cutoff, int metric, float alpha, float beta, int order, gsim_graph** out)
{
    return make_graph(out, "host memory for the join's lists",
                      [&](gsim_graph* g) { return join(db, db->shards[0], left.rows, left.nl, cutoff, metric, alpha, beta, order, g); });
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_join_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, float cutoff, int metric, float alpha, float beta, int order,
                         gsim_graph** out)
{
    int rc = check_join_args(db, out, nq, cutoff, metric, alpha, beta, order);
    if (rc != GSIM_OK) return rc;
    LeftSide left;
    rc = left.from_queries(db, queries, nq, "joins", "the join's left rows");
    if (rc != GSIM_OK) return rc;
    return run_join(db, left, cutoff, metric, alpha, beta, order, out);
}

int gsim_db_join(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, float cutoff, int metric, float alpha, float beta,
                 int order, gsim_graph** out)
{
    if (lrow_begin > lrow_end) {
        if (out) *out = nullptr;
        return fail(GSIM_ERR_INVALID, "left row range: begin past end");
    }
    int rc = check_join_args(db, out, lrow_end - lrow_begin, cutoff, metric, alpha, beta, order);
    if (rc == GSIM_OK) rc = check_left_handle(db, left, lrow_end);
    if (rc != GSIM_OK) return rc;
    LeftSide ls;
    rc = ls.from_handle(db, left, lrow_begin, lrow_end, "joins");
    if (rc != GSIM_OK) return rc;
    return run_join(db, ls, cutoff, metric, alpha, beta, order, out);
}

} // extern "C"
