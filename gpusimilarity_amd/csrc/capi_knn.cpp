// capi_knn.cpp -- gsim_db_knn: each row's k most similar other rows, exactly, as CSR; and KnnListPass (capi_pairs.h), the list pass
// it shares with capi_snn.cpp and capi_hdbscan.cpp.  The plan is plan_knn (capi_knn_join.cpp), the lists become CSR in capi_pairs.cpp
// (build_knn_csr).  The device side is gsim_knn.hip (the fold kernel, offsets, compaction).  The rule is stated in include/gpusim_hip.h.
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
    // popc of every row, and the rows zero-padded to WP words unless they already are WP words; the list pass with one counter word
    PaddedRows table;
    KnnListPass pass;
    DevBuf<> tmp;
    DevBuf<uint64_t> d_indptr;
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::knn_scan_bytes(nout + 1, &tmp_bytes));
    if (const int rc = table.alloc(N, s.W, WP, "the k-nearest-neighbour lists (popcounts)", "the k-nearest-neighbour lists (padded rows)")) return rc;
    if (const int rc = pass.alloc(db, N, WP, rb, re, k, 1, 0, true, {"the k-nearest-neighbour lists", "the k-nearest-neighbour lists (lengths)",
                                  "the k-nearest-neighbour lists (control block)"}, st))
        return rc;
    GSIM_ALLOC(d_indptr, (nout + 1) * 8, "the k-nearest-neighbour lists (row offsets)");
    GSIM_ALLOC(tmp, tmp_bytes, "the k-nearest-neighbour lists (scan scratch)");
    if (const int rc = table.prepare(s.d_rows, N, st)) return rc;
    if (const int rc = pass.fold(table, cutoff, metric, alpha, beta, st)) return rc;

    KnnCsr csr;
    if (const int rc = build_knn_csr(db, s, pass.lists, pass.len, nout, k, tmp, d_indptr, pass.ctl, "the k-nearest-neighbour CSR", "knn", g, &csr))
        return rc;

    pass.add_clocks(csr.ctl.data()); // (read with the insert counter, in one copy)
    gsim_knn_stats& ks = g->knn;
    ks.launches = pass.plan.size();
    ks.pairs = nout * N;
    ks.inserts = csr.ctl[0];
    ks.entries = csr.total;
    ks.kernel_ms = pass.ev_fold.ms();
    ks.csr_ms = csr.csr_ms;
    ks.d2h_ms = csr.d2h_ms;
    ks.clock_mhz = pass.clocks.mhz();
    ks.wall_ms = ms_since(t0);
    mirror_graph_stats(ks, ks.launches, ks.kernel_ms, &g->stats);
    return GSIM_OK;
}

} // namespace

int KnnListPass::alloc(const gsim_db* db, uint64_t N, uint32_t WP, uint64_t rb, uint64_t re, uint32_t k, size_t front_words, size_t back,
                       bool total, const Names& names, hipStream_t st)
{
    const uint64_t nout = re - rb, nlen = nout + (total ? 1 : 0);
    if (k && N >= 2) plan = plan_knn(nout, N, WP, db->knobs.knn_launch_pairs);
    front = front_words;
    ctl_words = back_at() + back;
    const std::string w = "device memory for ";
    if (k && lists.grow(nout * k * sizeof(gsim::KnnEntry)) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + names.lists);
    if (k && len.grow(nlen * 4) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + names.len);
    if (ctl.grow(ctl_words * 8) != hipSuccess) return fail(GSIM_ERR_NOMEM, w + names.ctl);
    if (k) GSIM_HIP(hipMemsetAsync(len, 0, nlen * 4, st));
    GSIM_HIP(hipMemsetAsync(ctl, 0, ctl_words * 8, st));
    clocks.view(word(front));
    args.nrows = N;
    args.row_begin = rb;
    args.row_end = re;
    args.WP = WP;
    args.k = k;
    args.lists = lists;
    args.len = len;
    args.inserts = word(0);
    return GSIM_OK;
}

int KnnListPass::fold(const PaddedRows& table, float cutoff, int metric, float alpha, float beta, hipStream_t st)
{
    if (!args.k) return GSIM_OK;
    gsim::KnnArgs a = args;
    a.rows = table.rows();
    a.pop = table.pop();
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;
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
    if (const int rc = check_k_cutoff("knn", k, cutoff)) return rc;
    if (const int rc = check_metric("knn", metric, alpha, beta)) return rc;
    if (row_begin > row_end || row_end > db->nrows) return fail(GSIM_ERR_INVALID, "row range outside the table");
    if (const int rc = check_tile_table(db, "knn")) return rc;
    if (const int rc = check_table_state(db, "knn", false)) return rc;
    const char* nomem = "host memory for the k-nearest-neighbour lists";
    return on_one_shard(db, nomem, [&](Shard& s) {
        return make_graph(out, nomem, [&](gsim_graph* g) { return knn(db, s, k, cutoff, metric, alpha, beta, row_begin, row_end, g); });
    });
}

} // extern "C"
