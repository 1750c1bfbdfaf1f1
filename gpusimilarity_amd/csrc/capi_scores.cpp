// capi_scores.cpp -- gsim_db_scores / gsim_db_scores_queries / gsim_db_scores_device: the dense matrix of scores of a block of
// left rows against a range of table rows.  The family's argument checks and one core that takes "left rows in device memory, nl
// of them" from a front's LeftSide (capi_front.h), as the histograms, with the prepare step, the launch plan and the staging slabs
// of the host-output calls.  The device side is gsim_scores.hip.  The rule is stated in include/gpusim_hip.h.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

// Pairs of one launch of the matrix kernel, priced from the measured kernel (1.19 / 1.43 / 1.72 ms per
// 2^30 pairs at WP = 8 / 32 / 64, i.e. about 8.8e-15 s x (WP + 120) a pair -- a floor set by the epilogue and the output
// write, plus the matrix pipe's share per word): 5.6e11 / (WP + 120) pairs are about 5 ms at every width, so that no launch
// comes near 50 ms on a shared GPU.
constexpr double kScoresLaunchBudget = 5.6e11;
constexpr double kScoresPairFloor = 120.0;

struct ScoresLaunch {
    uint64_t l0, l1, r0, r1;
};

// The launches of nl x nr pairs of rows of WP words: groups of block rows x ranges of block columns, each within the budget;
// `pairs` > 0 (GSIM_SCORES_LAUNCH_PAIRS) replaces the budget: at most that many pairs, at least one kScoresTile x kScoresTile
// block.  At most 65 535 block rows to a launch (the grid's second dimension).
std::vector<ScoresLaunch> plan_scores(uint64_t nl, uint64_t nr, uint32_t WP, long long pairs)
{
    const uint64_t tile = gsim::kScoresTile;
    const uint64_t by = (nl + tile - 1) / tile, bx = (nr + tile - 1) / tile;
    const double budget = pairs > 0 ? static_cast<double>(pairs) : kScoresLaunchBudget / (WP + kScoresPairFloor);
    const uint64_t max_blocks = std::max<uint64_t>(static_cast<uint64_t>(budget / static_cast<double>(tile * tile)), 1);
    const uint64_t gy = std::min<uint64_t>(std::min(by, max_blocks), 65535u);
    const uint64_t gx = std::min<uint64_t>(std::max<uint64_t>(max_blocks / gy, 1), bx);
    std::vector<ScoresLaunch> out;
    for (uint64_t y = 0; y < by; y += gy)
        for (uint64_t x = 0; x < bx; x += gx)
            out.push_back({y * tile, std::min((y + gy) * tile, nl), x * tile, std::min((x + gx) * tile, nr)});
    return out;
}

} // namespace

// left rows d_left[0 .. nl) (W words each, on s's device) against s's table rows [c.r0, c.r0 + c.nr)
int scores(gsim_db* db, Shard& s, const uint32_t* d_left, uint64_t nl, const ScoresCall& c)
{
    const auto t0 = std::chrono::steady_clock::now();
    auto wall = [&] { return ms_since(t0); };
    const uint64_t nr = c.nr;
    gsim_scores_stats ss{};
    ss.left_rows = nl;
    ss.right_rows = nr;
    ss.pairs = nl * nr;
    if (nl > 0 && nr > 0) {
        GSIM_HIP(set_device(s.device));
        const hipStream_t st = s.stream;
        const uint32_t W = s.W, WP = gsim::scores_padded_words(W);
        const uint32_t* d_right = static_cast<const uint32_t*>(s.d_rows) + c.r0 * W;

        // popc of every row of either side, and the rows zero-padded to WP words unless they already are WP words
        PaddedRows left, right;
        LaunchClocks clocks;
        DevBuf<> stage;
        if (const int rc = left.alloc(nl, W, WP, "the score matrix (popcounts of the left rows)", "the score matrix (padded left rows)")) return rc;
        if (const int rc = right.alloc(nr, W, WP, "the score matrix (popcounts of the table rows)", "the score matrix (padded table rows)")) return rc;
        // host output: slabs of whole left rows through device memory
        const bool host_out = c.out != nullptr;
        uint64_t slab_rows = nl;
        if (host_out) {
            slab_rows = std::min<uint64_t>(std::max<uint64_t>(static_cast<uint64_t>(db->knobs.scores_stage_bytes) / (nr * 4), 1), nl);
            GSIM_ALLOC(stage, slab_rows * nr * 4, "the score matrix (staging slab)");
        }
        const uint64_t nslabs = (nl + slab_rows - 1) / slab_rows;
        const std::vector<ScoresLaunch> plan = plan_scores(slab_rows, nr, WP, db->knobs.scores_launch_pairs);
        const uint64_t last_rows = nl - (nslabs - 1) * slab_rows;
        const std::vector<ScoresLaunch> plan_last = last_rows == slab_rows ? plan : plan_scores(last_rows, nr, WP, db->knobs.scores_launch_pairs);
        const size_t nlaunch = plan.size() * (nslabs - 1) + plan_last.size();
        if (const int rc = clocks.own(nlaunch, "the score matrix (clock stamps)")) return rc;
        GSIM_HIP(clocks.zero(nlaunch, st));

        EventPair ev_prep, ev_run, ev_d2h;
        GSIM_HIP(ev_prep.create());
        GSIM_HIP(ev_run.create());
        GSIM_HIP(ev_d2h.create());
        GSIM_HIP(hipEventRecord(ev_prep.a, st));
        if (const int rc = left.prepare(d_left, nl, st)) return rc;
        if (const int rc = right.prepare(d_right, nr, st)) return rc;
        GSIM_HIP(hipEventRecord(ev_prep.b, st));

        gsim::ScoresArgs a{};
        a.rrows = right.rows();
        a.rpop = right.pop();
        a.nr = nr;
        a.WP = WP;
        a.metric = c.metric;
        a.alpha = c.alpha;
        a.beta = c.beta;
        size_t launched = 0;
        for (uint64_t sl = 0; sl < nslabs; sl++) {
            const uint64_t first = sl * slab_rows, rows = std::min(slab_rows, nl - first);
            a.lrows = left.rows() + first * WP;
            a.lpop = left.pop() + first;
            a.nl = rows;
            a.out = host_out ? stage.as<float>() : c.d_out + first * c.ld;
            a.ld = host_out ? nr : c.ld;
            GSIM_HIP(hipEventRecord(ev_run.a, st));
            for (const ScoresLaunch& l : sl + 1 == nslabs ? plan_last : plan) {
                a.clk = clocks.at(launched++);
                GSIM_HIP(gsim::launch_scores(a, l.l0, l.l1, l.r0, l.r1, st));
            }
            GSIM_HIP(hipEventRecord(ev_run.b, st));
            if (host_out) {
                GSIM_HIP(hipEventRecord(ev_d2h.a, st));
                float* dst = c.out + first * c.ld;
                if (c.ld == nr) GSIM_HIP(hipMemcpyAsync(dst, stage, rows * nr * 4, hipMemcpyDeviceToHost, st));
                else GSIM_HIP(hipMemcpy2DAsync(dst, c.ld * 4, stage, nr * 4, nr * 4, rows, hipMemcpyDeviceToHost, st));
                GSIM_HIP(hipEventRecord(ev_d2h.b, st));
            }
            // (one slab at a time: the next one's kernel overwrites the staging memory, and the events are reused)
            GSIM_HIP(hipStreamSynchronize(st));
            ss.kernel_ms += ev_run.ms();
            if (host_out) ss.d2h_ms += ev_d2h.ms();
        }
        ss.launches = nlaunch;
        ss.slabs = host_out ? nslabs : 0;
        ss.prepare_ms = ev_prep.ms();
        GSIM_HIP(clocks.fetch(nlaunch, st));
        GSIM_HIP(hipStreamSynchronize(st));
        clocks.add();
        ss.clock_mhz = clocks.mhz();
    }
    ss.wall_ms = wall();
    if (c.stats) *c.stats = ss;
    return GSIM_OK;
}

namespace
{

// what every entry point checks before any device state (`handle`: the left rows are `left`'s; else the queries entry, nl = nq)
int check_scores_args(gsim_db* db, bool handle, const gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint64_t rrow_begin, uint64_t rrow_end,
                      int metric, float alpha, float beta, const void* out, uint64_t ld)
{
    if (!db) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_metric("scores", metric, alpha, beta)) return rc;
    if (lrow_begin > lrow_end) return fail(GSIM_ERR_INVALID, "left row range: begin past end");
    // (ahead of the count of left rows: a handle's range is refused as outside its table, whatever its length)
    if (handle)
        if (const int rc = check_left_handle(db, left, lrow_end)) return rc;
    if (rrow_begin > rrow_end) return fail(GSIM_ERR_INVALID, "table row range: begin past end");
    if (rrow_end > db->nrows) return fail(GSIM_ERR_INVALID, "table row range outside the table");
    const uint64_t nl = lrow_end - lrow_begin, nr = rrow_end - rrow_begin;
    if (nl > 0xFFFFFFFFull || nr > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "scores: 2^32 rows or more on one side");
    if (ld < nr) return fail(GSIM_ERR_INVALID, "scores: ld is less than the number of table rows");
    if (gsim::scores_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "score matrices support rows of up to 4096 bits");
    if (!out && nl > 0 && nr > 0) return fail(GSIM_ERR_INVALID, "scores: NULL output");
    return GSIM_OK;
}

int run_scores(gsim_db* db, const LeftSide& left, const ScoresCall& c)
{
    try {
        return scores(db, db->shards[0], left.rows, left.nl, c);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "host memory for the score matrix");
    }
}

// the two fronts whose left rows are a handle's: `out` in host memory, or `d_out` in the table's device memory
int scores_of_handle(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint64_t rrow_begin, uint64_t rrow_end, int metric,
                     float alpha, float beta, float* out, float* d_out, uint64_t ld, gsim_scores_stats* stats)
{
    int rc = check_scores_args(db, true, left, lrow_begin, lrow_end, rrow_begin, rrow_end, metric, alpha, beta, out ? static_cast<void*>(out) : d_out, ld);
    if (rc != GSIM_OK) return rc;
    LeftSide ls;
    rc = ls.from_handle(db, left, lrow_begin, lrow_end, "score matrices");
    if (rc != GSIM_OK) return rc;
    const ScoresCall c{rrow_begin, rrow_end - rrow_begin, metric, alpha, beta, out, d_out, ld, stats};
    return run_scores(db, ls, c);
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_scores(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint64_t rrow_begin, uint64_t rrow_end, int metric,
                   float alpha, float beta, float* out, uint64_t ld, gsim_scores_stats* stats)
{
    return scores_of_handle(db, left, lrow_begin, lrow_end, rrow_begin, rrow_end, metric, alpha, beta, out, nullptr, ld, stats);
}

int gsim_db_scores_device(gsim_db* db, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint64_t rrow_begin, uint64_t rrow_end, int metric,
                          float alpha, float beta, void* d_out, uint64_t ld, gsim_scores_stats* stats)
{
    return scores_of_handle(db, left, lrow_begin, lrow_end, rrow_begin, rrow_end, metric, alpha, beta, nullptr, static_cast<float*>(d_out), ld, stats);
}

int gsim_db_scores_queries(gsim_db* db, const uint32_t* queries, uint64_t nq, uint64_t rrow_begin, uint64_t rrow_end, int metric, float alpha,
                           float beta, float* out, uint64_t ld, gsim_scores_stats* stats)
{
    int rc = check_scores_args(db, false, nullptr, 0, nq, rrow_begin, rrow_end, metric, alpha, beta, out, ld);
    if (rc != GSIM_OK) return rc;
    LeftSide left;
    // (no table rows: the core reads no left row)
    rc = left.from_queries(db, queries, nq, "score matrices", "the score matrix's left rows", rrow_end > rrow_begin);
    if (rc != GSIM_OK) return rc;
    const ScoresCall c{rrow_begin, rrow_end - rrow_begin, metric, alpha, beta, out, nullptr, ld, stats};
    return run_scores(db, left, c);
}

} // extern "C"
