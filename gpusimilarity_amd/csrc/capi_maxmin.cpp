// capi_maxmin.cpp -- gsim_db_maxmin: MaxMin diversity picking, one pass over the table per pick.  The device side is
// gsim_maxmin.hip; the rule is stated in include/gpusim_hip.h.
#include "capi_front.h"

#include <cmath>

namespace gsim_host
{

// Bytes one launch of a pass streams at most (rows + their 4-byte state): 256 M rows x 128 B, ~5 ms at the scan's rate.
constexpr uint64_t kMaxMinLaunchBytes = (256ull << 20) * 128ull;
// Tables whose rows and state take at most this many bytes stream with default-policy loads (launch_maxmin_pass_cached): they
// fit the 256 MiB Infinity Cache, and every pass re-reads them from there -- 25.7 against 30.4 us per pick at 1 M x 1024-bit
// rows (136 MB); at 100 M rows the nt loads are faster.
constexpr uint64_t kMaxMinCachedBytes = 192ull << 20;
// Passes enqueued between two looks at the done word (the passes after an early stop return at once).
constexpr uint32_t kMaxMinBatch = 64;

namespace
{

// Rows per launch of a pass: a multiple of 64 (launch starts stay 16-byte aligned for every width)
uint64_t launch_rows(uint32_t W)
{
    uint64_t r = kMaxMinLaunchBytes / (static_cast<uint64_t>(W) * 4u + 4u);
#ifdef GSIM_TEST_HOOKS
    // GSIM_TEST_MAXMIN_LAUNCH_ROWS: a short cap, so that the tests run multi-launch passes on small tables
    const int cap = env_int("GSIM_TEST_MAXMIN_LAUNCH_ROWS", 0);
    if (cap > 0) r = static_cast<uint64_t>(cap);
#endif
    r = r / 64 * 64;
    return r < 64 ? 64 : r;
}

struct PassLaunch {
    uint64_t r0, nrows;
    uint32_t wg0;
    gsim::ScanGeometry g;
};

int maxmin(gsim_db* db, Shard& s, uint32_t npicks, const uint32_t* seeds, uint32_t nseeds, int metric, float alpha, float beta,
           float max_score, uint32_t* picks, float* pick_scores, uint32_t* npicked, float* row_score, uint32_t* nearest,
           gsim_maxmin_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;
    const bool assign = row_score || nearest;

    std::vector<PassLaunch> plan;
    const uint64_t per = launch_rows(s.W);
    uint32_t nwg = 0;
    for (uint64_t r0 = 0; r0 < N; r0 += per) {
        PassLaunch l{r0, std::min(per, N - r0), nwg, {}};
        l.g = gsim::maxmin_geometry(l.nrows, s.W, s.num_cus);
        nwg += l.g.nwaves / (gsim::kScanBlock / 64);
        plan.push_back(l);
    }

    DevBuf<> d_maxsim, d_nearest, d_picks, d_scores, d_ctl, d_part;
    GSIM_HIP(d_maxsim.grow(N * 4));
    if (nearest) GSIM_HIP(d_nearest.grow(N * 4));
    GSIM_HIP(d_picks.grow(static_cast<size_t>(npicks) * 4));
    GSIM_HIP(d_scores.grow(static_cast<size_t>(npicks) * 4));
    GSIM_HIP(d_ctl.grow(gsim::kMaxMinCtlWords * 4));
    GSIM_HIP(d_part.grow(static_cast<size_t>(nwg) * 8));
    HostBuf<uint32_t> h_done(hipHostMallocDefault); // the done word after every batch, two slots
    GSIM_HIP(h_done.grow(64));

    // initial state: maxsim = -1 everywhere, pick 0 (the first seed, or row 0) marked picked, its score 0
    std::vector<uint32_t> first(std::max<uint32_t>(nseeds, 1));
    for (uint32_t j = 0; j < nseeds; j++) first[j] = static_cast<uint32_t>(seeds[j] - db->row_base);
    if (nseeds == 0) first[0] = 0;
    const float minus_one = -1.0f, picked = INFINITY, zero = 0.0f;
    uint32_t minus_one_bits, picked_bits;
    std::memcpy(&minus_one_bits, &minus_one, 4);
    std::memcpy(&picked_bits, &picked, 4);
    std::vector<uint32_t> ctl(gsim::kMaxMinCtlWords, 0u);
    ctl[gsim::kMaxMinPicked] = 1;
    GSIM_HIP(hipMemsetD32Async(static_cast<hipDeviceptr_t>(d_maxsim), static_cast<int>(minus_one_bits), N, stream));
    GSIM_HIP(hipMemcpyAsync(d_maxsim.as<uint32_t>() + first[0], &picked_bits, 4, hipMemcpyHostToDevice, stream));
    GSIM_HIP(hipMemcpyAsync(d_picks, first.data(), first.size() * 4, hipMemcpyHostToDevice, stream));
    GSIM_HIP(hipMemcpyAsync(d_scores, &zero, 4, hipMemcpyHostToDevice, stream));
    GSIM_HIP(hipMemcpyAsync(d_ctl, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice, stream));

    gsim::MaxMinArgs m{};
    m.rows = s.d_rows;
    m.nrows = N;
    m.W = s.W;
    m.metric = metric;
    m.alpha = alpha;
    m.beta = beta;
    m.max_score = max_score;
    m.maxsim = d_maxsim.as<float>();
    m.nearest = d_nearest.as<uint32_t>();
    m.picks = d_picks.as<uint32_t>();
    m.pick_scores = d_scores.as<float>();
    m.ctl = d_ctl.as<uint32_t>();
    m.partials = d_part.as<unsigned long long>();
    m.npicks = npicks;
    m.nseeds = nseeds;
    m.nwg_total = nwg;

    // pass p streams pick p's row; the last pick needs its pass only for row_score / nearest
    const uint32_t npasses = assign ? npicks : npicks - 1;
    EventPair ev_k, ev_d2h;
    GSIM_HIP(ev_k.create());
    GSIM_HIP(ev_d2h.create());
    Event ev_batch[2];
    for (auto& e : ev_batch) GSIM_HIP(e.create(hipEventDisableTiming));
    const bool cached = N * (static_cast<uint64_t>(s.W) * 4u + (nearest ? 8u : 4u)) <= kMaxMinCachedBytes;
    const auto launch = cached ? gsim::launch_maxmin_pass_cached : gsim::launch_maxmin_pass;
    uint64_t launches = 0;
    GSIM_HIP(hipEventRecord(ev_k.a, stream));
    // Batches of passes; while batch b runs the host enqueues batch b + 1, then looks at the done word batch b left.
    for (uint32_t b = 0, p0 = 0; p0 < npasses; b++, p0 += kMaxMinBatch) {
        const uint32_t p1 = std::min(npasses, p0 + kMaxMinBatch);
        for (uint32_t p = p0; p < p1; p++)
            for (const PassLaunch& l : plan) {
                GSIM_HIP(launch(m, l.g, l.r0, l.nrows, l.wg0, p, stream));
                launches++;
            }
        GSIM_HIP(hipMemcpyAsync(h_done + (b & 1), d_ctl, 4, hipMemcpyDeviceToHost, stream));
        GSIM_HIP(hipEventRecord(ev_batch[b & 1], stream));
        if (b > 0) {
            GSIM_HIP(hipEventSynchronize(ev_batch[(b - 1) & 1]));
            if (h_done[(b - 1) & 1]) break;
        }
    }
    GSIM_HIP(hipEventRecord(ev_k.b, stream));

    GSIM_HIP(hipEventRecord(ev_d2h.a, stream));
    GSIM_HIP(hipMemcpyAsync(ctl.data(), d_ctl, ctl.size() * 4, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipMemcpyAsync(picks, d_picks, static_cast<size_t>(npicks) * 4, hipMemcpyDeviceToHost, stream));
    if (pick_scores) GSIM_HIP(hipMemcpyAsync(pick_scores, d_scores, static_cast<size_t>(npicks) * 4, hipMemcpyDeviceToHost, stream));
    if (row_score) GSIM_HIP(hipMemcpyAsync(row_score, d_maxsim, N * 4, hipMemcpyDeviceToHost, stream));
    if (nearest) GSIM_HIP(hipMemcpyAsync(nearest, d_nearest, N * 4, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipEventRecord(ev_d2h.b, stream));
    GSIM_HIP(hipStreamSynchronize(stream));

    const uint32_t n = ctl[gsim::kMaxMinPicked];
    if (n < 1 || n > npicks) return fail(GSIM_ERR_STATE, "maxmin: the device reported an impossible pick count");
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t r = picks[j];
        if (row_score) row_score[r] = 1.0f; // a picked row: its own nearest pick
        if (nearest) nearest[r] = j;
        picks[j] = r + db->row_base;
    }
    *npicked = n;
    if (st) {
        st->picks = n;
        st->launches = launches;
        uint64_t upd = 0;
        std::memcpy(&upd, ctl.data() + gsim::kMaxMinUpdated, 8);
        st->rows_updated = upd;
        st->kernel_ms = ev_k.ms();
        st->d2h_ms = ev_d2h.ms();
        st->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_maxmin(gsim_db* db, uint32_t npicks, const uint32_t* seeds, uint32_t nseeds, int metric, float alpha, float beta,
                   float max_score, uint32_t* picks, float* pick_scores, uint32_t* npicked, float* row_score, uint32_t* nearest,
                   gsim_maxmin_stats* stats)
{
    if (!db || !picks || !npicked) return fail(GSIM_ERR_INVALID, "NULL argument");
    *npicked = 0;
    if (stats) *stats = gsim_maxmin_stats{};
    if (const int rc = check_symmetric_metric("maxmin needs", "maxmin", metric, alpha, beta)) return rc;
    if (!(max_score >= 0.0f && max_score <= 1.0f)) return fail(GSIM_ERR_INVALID, "max_score must be in [0, 1]");
    const uint64_t N = db->nrows;
    if (N > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "maxmin: tables of 2^32 rows or more");
    if (npicks > N) return fail(GSIM_ERR_INVALID, "npicks exceeds the number of rows");
    if (nseeds > npicks) return fail(GSIM_ERR_INVALID, "more seeds than picks");
    if (const int rc = check_seeds(db, seeds, nseeds, "maxmin seeds")) return rc;
    if (const int rc = check_table_state(db, "maxmin", false)) return rc;
    if (npicks == 0) return GSIM_OK;
    return on_one_shard(db, "host memory for maxmin", [&](Shard& s) {
        return maxmin(db, s, npicks, seeds, nseeds, metric, alpha, beta, max_score, picks, pick_scores, npicked, row_score, nearest, stats);
    });
}

} // extern "C"
