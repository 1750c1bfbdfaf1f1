// capi_knn.cpp -- gsim_db_knn: each row's k most similar other rows, exactly, as CSR.  The argument checks and the launches of a
// call; the plan is plan_knn (capi_knn_join.cpp), the lists become CSR in capi_pairs.cpp (build_knn_csr).  The device side is
// gsim_knn.hip (the fold kernel, offsets, compaction).  The rule is stated in include/gpusim_hip.h.  The fold launches of a plan
// (knn_args, run_knn_fold) are also the core pass of the HDBSCAN calls (capi_hdbscan.cpp).
#include "capi_front.h"

namespace gsim_host
{
namespace
{

int knn(gsim_db* db, Shard& s, uint32_t k, float cutoff, int metric, float alpha, float beta, uint64_t rb, uint64_t re, gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint64_t nout = re - rb;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    g->kind = gsim_graph::Kind::kKnn;
    g->knn.rows = nout;
    g->indptr.assign(nout + 1, 0);
    if (nout == 0 || N < 2) {
        g->knn.wall_ms = g->stats.wall_ms = ms_since(t0);
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const std::vector<KnnLaunch> plan = plan_knn(nout, N, WP, db->knobs.knn_launch_pairs);

    // popc of every row, and the rows zero-padded to WP words unless they already are WP words; the lists and their lengths
    // (one more length, zero: the scan's last output is the total); [0] the insert counter, then 4 clock stamps per launch
    PaddedRows table;
    DevBuf<> ctl, tmp;
    DevBuf<gsim::KnnEntry> lists;
    DevBuf<uint32_t> len;
    DevBuf<uint64_t> d_indptr;
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::knn_scan_bytes(nout + 1, &tmp_bytes));
    if (const int rc = table.alloc(N, s.W, WP, "the k-nearest-neighbour lists (popcounts)", "the k-nearest-neighbour lists (padded rows)")) return rc;
    GSIM_ALLOC(lists, nout * k * sizeof(gsim::KnnEntry), "the k-nearest-neighbour lists");
    GSIM_ALLOC(len, (nout + 1) * 4, "the k-nearest-neighbour lists (lengths)");
    GSIM_ALLOC(d_indptr, (nout + 1) * 8, "the k-nearest-neighbour lists (row offsets)");
    GSIM_ALLOC(ctl, (1 + 4 * plan.size()) * 8, "the k-nearest-neighbour lists (control block)");
    GSIM_ALLOC(tmp, tmp_bytes, "the k-nearest-neighbour lists (scan scratch)");
    unsigned long long* d_inserts = ctl.as<unsigned long long>();
    LaunchClocks clocks;
    clocks.view(d_inserts + 1);
    GSIM_HIP(hipMemsetAsync(len, 0, (nout + 1) * 4, st));
    GSIM_HIP(hipMemsetAsync(ctl, 0, (1 + 4 * plan.size()) * 8, st));
    if (const int rc = table.prepare(s.d_rows, N, st)) return rc;

    EventPair ev_fold;
    if (const int rc = run_knn_fold(knn_args(table, N, rb, re, WP, k, cutoff, metric, alpha, beta, lists, len, d_inserts), plan, clocks, ev_fold, st))
        return rc;

    KnnCsr csr;
    if (const int rc = build_knn_csr(db, s, lists, len, nout, k, tmp, d_indptr, ctl, "the k-nearest-neighbour CSR", "knn", g, &csr)) return rc;

    clocks.add(csr.ctl.data() + 1, plan.size()); // (read with the insert counter, in one copy)
    gsim_knn_stats& ks = g->knn;
    ks.launches = plan.size();
    ks.pairs = nout * N;
    ks.inserts = csr.ctl[0];
    ks.entries = csr.total;
    ks.kernel_ms = ev_fold.ms();
    ks.csr_ms = csr.csr_ms;
    ks.d2h_ms = csr.d2h_ms;
    ks.clock_mhz = clocks.mhz();
    ks.wall_ms = ms_since(t0);
    mirror_graph_stats(ks, ks.launches, ks.kernel_ms, &g->stats);
    return GSIM_OK;
}

} // namespace

gsim::KnnArgs knn_args(const PaddedRows& table, uint64_t N, uint64_t rb, uint64_t re, uint32_t WP, uint32_t k, float cutoff, int metric,
                       float alpha, float beta, gsim::KnnEntry* lists, uint32_t* len, unsigned long long* inserts)
{
    gsim::KnnArgs a{};
    a.rows = table.rows();
    a.pop = table.pop();
    a.nrows = N;
    a.row_begin = rb;
    a.row_end = re;
    a.WP = WP;
    a.k = k;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;
    a.lists = lists;
    a.len = len;
    a.inserts = inserts;
    return a;
}

int run_knn_fold(gsim::KnnArgs a, const std::vector<KnnLaunch>& plan, const LaunchClocks& clocks, EventPair& ev_fold, hipStream_t st)
{
    GSIM_HIP(ev_fold.create());
    GSIM_HIP(hipEventRecord(ev_fold.a, st));
    for (size_t l = 0; l < plan.size(); l++) {
        a.clk = clocks.at(l);
        GSIM_HIP(gsim::launch_knn_fold(a, plan[l].ot0, plan[l].not_, plan[l].c0, plan[l].c1, st));
    }
    GSIM_HIP(hipEventRecord(ev_fold.b, st));
    return GSIM_OK;
}

} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_knn(gsim_db* db, uint32_t k, float cutoff, int metric, float alpha, float beta, uint64_t row_begin, uint64_t row_end,
                gsim_graph** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (k < 1 || k > GSIM_KNN_MAX_K) return fail(GSIM_ERR_INVALID, "knn: k must be in [1, GSIM_KNN_MAX_K = 128]");
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, "knn: the cutoff must be in (0, 1]");
    if (const int rc = check_metric("knn", metric, alpha, beta)) return rc;
    if (row_begin > row_end || row_end > db->nrows) return fail(GSIM_ERR_INVALID, "row range outside the table");
    if (db->fp_bits > 4096 || gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, "knn: rows wider than 4096 bits");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "knn: tables of 2^32 rows or more");
    if (const int rc = check_table_state(db, "knn", false)) return rc;
    const char* nomem = "host memory for the k-nearest-neighbour lists";
    return on_one_shard(db, nomem, [&](Shard& s) {
        return make_graph(out, nomem, [&](gsim_graph* g) { return knn(db, s, k, cutoff, metric, alpha, beta, row_begin, row_end, g); });
    });
}

} // extern "C"
