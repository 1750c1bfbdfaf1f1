// capi_dbscan.cpp -- gsim_db_dbscan (DBSCAN density clustering of a resident table in two passes over the pairs: degrees, then the
// cores' components and the border rows' anchors) and gsim_dbscan (the same rule on a symmetric scored CSR graph, host code).  The
// argument checks and the launch sequence of a call; the device side is gsim_dbscan.hip.  The rule is stated in include/gpusim_hip.h.
//
// Device memory of a call, all of it RAII (DevBuf) and freed on every return: per row 4 B of degree, 4 B of forest, 8 B of anchor key,
// 4 B of label_of and 8 B of label scratch = 28 B x N; 4 B x N more for each of anchor / first_row / sizes asked for; PaddedRows'
// 4 B x N of popcounts and, where the width is not one the tile kernels hold, the zero-padded copy of the rows; the scan's scratch
// and a control block of 7 counters and 4 clock words per launch.
#include "capi_front.h"

#include <cmath>

namespace gsim_host
{
namespace
{

int dbscan(gsim_db* db, Shard& s, float cutoff, uint32_t min_pts, int metric, float alpha, float beta, uint32_t* label_of, uint32_t* nclusters,
           uint32_t* degree, uint32_t* anchor, uint32_t* first_row, uint32_t* sizes, gsim_dbscan_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;

    // both passes walk the same tiles: one plan, run twice
    const uint64_t nt = (N + gsim::kNbrTile - 1) / gsim::kNbrTile;
    const std::vector<NbrLaunch> plan =
        N < 2 ? std::vector<NbrLaunch>() : plan_launches(nt, nt, true, WP, static_cast<uint64_t>(db->knobs.dbscan_launch_pairs));
    const size_t np = plan.size(), ctl_words = gsim::kDbscanCounters + LaunchClocks::kWords * 2 * np;
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::scan_u32_bytes(N, &tmp_bytes));
    PaddedRows table;
    DevBuf<uint32_t> d_degree, parent, d_label, d_anchor, d_first, d_sizes, d_ncl, d_flag, d_num;
    DevBuf<unsigned long long> best, ctl; // the counters, then 4 clock stamps per launch: the degree pass's, then the link pass's
    DevBuf<> tmp;
    const size_t stripe = static_cast<size_t>(N) * 4;
    if (const int rc = table.alloc(N, s.W, WP, "dbscan (popcounts)", "dbscan (the padded rows)")) return rc;
    GSIM_ALLOC(d_degree, stripe, "dbscan (the degrees)");
    GSIM_ALLOC(parent, stripe, "dbscan (the forest)");
    GSIM_ALLOC(best, stripe * 2, "dbscan (the anchor keys)");
    GSIM_ALLOC(d_label, stripe, "dbscan (label_of)");
    if (anchor) GSIM_ALLOC(d_anchor, stripe, "dbscan (anchor)");
    if (first_row) GSIM_ALLOC(d_first, stripe, "dbscan (first_row)");
    if (sizes) GSIM_ALLOC(d_sizes, stripe, "dbscan (sizes)");
    GSIM_ALLOC(d_ncl, 4, "dbscan (the count)");
    GSIM_ALLOC(d_flag, stripe, "dbscan (label scratch)");
    GSIM_ALLOC(d_num, stripe, "dbscan (label scratch)");
    GSIM_ALLOC(ctl, ctl_words * 8, "dbscan (control block)");
    GSIM_ALLOC(tmp, tmp_bytes, "dbscan (scan scratch)");
    LaunchClocks clocks;
    clocks.view(ctl + gsim::kDbscanCounters);

    gsim::DbscanArgs a{};
    a.nrows = N;
    a.WP = WP;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;
    a.min_pts = min_pts;
    a.skip = db->knobs.dbscan_skip ? 1u : 0u;
    a.degree = d_degree;
    a.parent = parent;
    a.best = best;
    a.counters = ctl;

    EventPair ev_count, ev_link, ev_label, ev_d2h;
    GSIM_HIP(ev_count.create());
    GSIM_HIP(ev_link.create());
    GSIM_HIP(ev_label.create());
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipMemsetAsync(ctl, 0, ctl_words * 8, stream));
    GSIM_HIP(hipMemsetAsync(d_degree, 0, stripe, stream));
    GSIM_HIP(hipMemsetAsync(best, 0, stripe * 2, stream));
    if (const int rc = table.prepare(s.d_rows, N, stream)) return rc;
    a.rows = table.rows();
    a.pop = table.pop();
    GSIM_HIP(gsim::launch_comp_init(parent, N, 1, stream));
    // the degree pass
    GSIM_HIP(hipEventRecord(ev_count.a, stream));
    for (size_t l = 0; l < np; l++) {
        gsim::DbscanArgs al = a;
        al.clk = clocks.at(l);
        GSIM_HIP(gsim::launch_dbscan_count(al, plan[l].rt0, plan[l].nrt, plan[l].ct0, plan[l].nct, stream));
    }
    GSIM_HIP(hipEventRecord(ev_count.b, stream));
    // the link pass, on the finished degrees: every launch is followed by the flatten (all path shortening is there; after the last
    // launch it leaves parent[x] = the smallest core of x's cluster, or x itself for a non-core row)
    GSIM_HIP(hipEventRecord(ev_link.a, stream));
    for (size_t l = 0; l < np; l++) {
        gsim::DbscanArgs al = a;
        al.clk = clocks.at(np + l);
        GSIM_HIP(gsim::launch_dbscan_link(al, plan[l].rt0, plan[l].nrt, plan[l].ct0, plan[l].nct, stream));
        GSIM_HIP(gsim::launch_comp_flatten(parent, N, 1, stream));
    }
    GSIM_HIP(hipEventRecord(ev_link.b, stream));
    GSIM_HIP(hipEventRecord(ev_label.a, stream));
    if (sizes) GSIM_HIP(hipMemsetAsync(d_sizes, 0, stripe, stream));
    // (a buffer not asked for is empty: a null pointer, which the label kernel passes over)
    GSIM_HIP(gsim::launch_dbscan_label(tmp, tmp_bytes, a, db->row_base, d_flag, d_num, d_label, d_anchor, d_first, d_sizes, d_ncl, stream));
    GSIM_HIP(hipEventRecord(ev_label.b, stream));
    std::vector<unsigned long long> h_ctl(ctl_words);
    uint32_t h_ncl = 0;
    GSIM_HIP(hipEventRecord(ev_d2h.a, stream));
    GSIM_HIP(hipMemcpyAsync(&h_ncl, d_ncl, 4, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipMemcpyAsync(h_ctl.data(), ctl, ctl_words * 8, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipMemcpyAsync(label_of, d_label, stripe, hipMemcpyDeviceToHost, stream));
    if (degree) GSIM_HIP(hipMemcpyAsync(degree, d_degree, stripe, hipMemcpyDeviceToHost, stream));
    if (anchor) GSIM_HIP(hipMemcpyAsync(anchor, d_anchor, stripe, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipStreamSynchronize(stream));
    if (h_ncl > N) return fail(GSIM_ERR_STATE, "dbscan: the device reported an impossible count");
    // (entries at and after nclusters are left untouched)
    if (first_row && h_ncl) GSIM_HIP(hipMemcpyAsync(first_row, d_first, static_cast<size_t>(h_ncl) * 4, hipMemcpyDeviceToHost, stream));
    if (sizes && h_ncl) GSIM_HIP(hipMemcpyAsync(sizes, d_sizes, static_cast<size_t>(h_ncl) * 4, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipEventRecord(ev_d2h.b, stream));
    GSIM_HIP(hipStreamSynchronize(stream));
    const uint64_t cores = h_ctl[gsim::kDbscanCores], borders = h_ctl[gsim::kDbscanBorders], noise = h_ctl[gsim::kDbscanNoise];
    if (h_ctl[gsim::kDbscanDegreeSum] != 2 * h_ctl[gsim::kDbscanKept]) return fail(GSIM_ERR_STATE, "dbscan: the degrees and the kept pairs do not add up");
    if (cores < h_ncl || h_ctl[gsim::kDbscanUnions] != cores - h_ncl) return fail(GSIM_ERR_STATE, "dbscan: the hooks, the cores and the cluster count do not add up");
    if (cores + borders + noise != N) return fail(GSIM_ERR_STATE, "dbscan: cores, border rows and noise do not add up to the rows");
    *nclusters = h_ncl;
    if (st) {
        st->rows = N;
        st->launches_count = np;
        st->launches_link = np;
        st->pairs = N * (N - 1) / 2;
        st->kept = h_ctl[gsim::kDbscanKept];
        st->cores = cores;
        st->borders = borders;
        st->noise = noise;
        st->clusters = h_ncl;
        st->unions = h_ctl[gsim::kDbscanUnions];
        st->cas_failed = h_ctl[gsim::kDbscanCasFailed];
        st->count_ms = ev_count.ms();
        st->link_ms = ev_link.ms();
        st->label_ms = ev_label.ms();
        st->d2h_ms = ev_d2h.ms();
        clocks.add(h_ctl.data() + gsim::kDbscanCounters, 2 * np); // (read with the counters, in one copy)
        st->clock_mhz = clocks.mhz();
        st->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_dbscan(gsim_db* db, float cutoff, uint32_t min_pts, int metric, float alpha, float beta, uint32_t* label_of, uint32_t* nclusters,
                   uint32_t* degree, uint32_t* anchor, uint32_t* first_row, uint32_t* sizes, gsim_dbscan_stats* stats)
{
    if (stats) *stats = gsim_dbscan_stats{};
    if (nclusters) *nclusters = 0;
    if (!db || !label_of || !nclusters) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_cutoff("dbscan", cutoff)) return rc;
    if (min_pts == 0) return fail(GSIM_ERR_INVALID, "dbscan: min_pts must be at least 1");
    if (const int rc = check_symmetric_metric("dbscan needs", "dbscan", metric, alpha, beta)) return rc;
    if (const int rc = check_tile_table(db, "dbscan")) return rc;
    const uint64_t N = db->nrows;
    if (N == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "dbscan", false)) return rc;
    return on_one_shard(db, "host memory for dbscan", [&](Shard& s) {
        return dbscan(db, s, cutoff, min_pts, metric, alpha, beta, label_of, nclusters, degree, anchor, first_row, sizes, stats);
    });
}

int gsim_dbscan(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows, uint32_t min_pts, uint32_t* label_of,
                uint32_t* anchor, uint32_t* first_row, uint32_t* sizes, uint64_t* nclusters)
{
    if (nclusters) *nclusters = 0;
    if (!indptr || !nclusters || (nrows && !label_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (min_pts == 0) return fail(GSIM_ERR_INVALID, "dbscan: min_pts must be at least 1");
    uint64_t nnz = 0;
    if (const int rc = check_csr_offsets(indptr, nrows, &nnz)) return rc;
    if (const int rc = check_csr_indices(indices, nnz, nrows)) return rc;
    if (nnz && !scores) return fail(GSIM_ERR_INVALID, "NULL scores");
    for (uint64_t e = 0; e < nnz; e++)
        if (std::isnan(scores[e])) return fail(GSIM_ERR_INVALID, "dbscan: a NaN score");
    try {
        // degree: the length of the row's list, self edges not counted
        std::vector<uint8_t> core(nrows);
        for (uint64_t r = 0; r < nrows; r++) {
            uint64_t deg = 0;
            for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++) deg += indices[e] != r;
            core[r] = deg + 1 >= min_pts;
        }
        // clusters: the components of the cores, numbered by their smallest core (a forest's root is its smallest row)
        Forest f(nrows);
        for (uint64_t r = 0; r < nrows; r++)
            for (uint64_t e = indptr[r]; core[r] && e < indptr[r + 1]; e++)
                if (core[indices[e]]) f.unite(static_cast<uint32_t>(r), indices[e]);
        std::vector<uint32_t> num(nrows);
        uint32_t nc = 0;
        for (uint64_t r = 0; r < nrows; r++)
            if (core[r] && f.root(static_cast<uint32_t>(r)) == r) {
                if (first_row) first_row[nc] = static_cast<uint32_t>(r);
                if (sizes) sizes[nc] = 0;
                num[r] = nc++;
            }
        for (uint64_t r = 0; r < nrows; r++) {
            uint32_t anc = GSIM_DBSCAN_NOISE;
            if (core[r]) anc = static_cast<uint32_t>(r);
            else {
                // the anchor: the core neighbour with the highest score, among equal scores the smallest row
                float bs = 0.0f;
                for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++) {
                    const uint32_t c = indices[e];
                    if (c == r || !core[c]) continue;
                    if (anc == GSIM_DBSCAN_NOISE || scores[e] > bs || (scores[e] == bs && c < anc)) {
                        anc = c;
                        bs = scores[e];
                    }
                }
            }
            const uint32_t label = anc == GSIM_DBSCAN_NOISE ? GSIM_DBSCAN_NOISE : num[f.root(anc)];
            label_of[r] = label;
            if (anchor) anchor[r] = anc;
            if (sizes && label != GSIM_DBSCAN_NOISE) sizes[label]++;
        }
        *nclusters = nc;
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "dbscan");
    }
    return GSIM_OK;
}

} // extern "C"
