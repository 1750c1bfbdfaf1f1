// capi_snn.cpp -- gsim_db_snn (gsim_db_knn's graph with the shared-nearest-neighbour count of every entry) and gsim_db_jarvis_patrick
// (Jarvis-Patrick clustering at up to eight kmin levels; the graph never leaves the device).  The argument checks and the launch
// sequence of a call: gsim_db_knn's list pass over all rows (KnnListPass, capi_pairs.h), the sort and link kernels of gsim_snn.hip,
// then either the k-NN calls' CSR tail (build_knn_csr) or gsim_db_components' flatten and labelling (ForestLabels, capi_front.h).
// The rule is stated in include/gpusim_hip.h; the host functions of the same rule are in capi_snn_host.cpp.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

// What both calls do first: the lists of all N >= 2 rows (KnnListPass: behind its clock stamps, the link kernel's kSnnCounters), their
// rows sorted, and the link pass.
struct SnnPass {
    PaddedRows table;
    KnnListPass knn;
    DevBuf<> tmp;
    DevBuf<uint32_t> nbr;
    EventPair ev_sort, ev_link;

    // `parent`: nlevels initialised forests, flattened here after the link launch (or nullptr); `shared`: N x k words (or nullptr)
    int run(gsim_db* db, Shard& s, uint32_t k, float cutoff, int metric, float alpha, float beta, uint32_t flags, const uint32_t* kmins,
            uint32_t nlevels, uint32_t* parent, uint32_t* shared, size_t scan_bytes)
    {
        const uint64_t N = s.nrows;
        const uint32_t WP = gsim::nbr_padded_words(s.W);
        const hipStream_t st = s.stream;
        if (const int rc = table.alloc(N, s.W, WP, "the shared-neighbour pass (popcounts)", "the shared-neighbour pass (padded rows)")) return rc;
        if (const int rc = knn.alloc(db, N, WP, 0, N, k, 1, gsim::kSnnCounters, true, {"the shared-neighbour pass (the k-nearest-neighbour lists)",
                                     "the shared-neighbour pass (the lists' lengths)", "the shared-neighbour pass (control block)"}, st))
            return rc;
        GSIM_ALLOC(nbr, N * k * 4, "the shared-neighbour pass (the sorted lists)");
        GSIM_ALLOC(tmp, scan_bytes, "the shared-neighbour pass (scan scratch)");
        if (const int rc = table.prepare(s.d_rows, N, st)) return rc;
        if (const int rc = knn.fold(table, cutoff, metric, alpha, beta, st)) return rc;
        GSIM_HIP(ev_sort.create());
        GSIM_HIP(ev_link.create());
        GSIM_HIP(hipEventRecord(ev_sort.a, st));
        GSIM_HIP(gsim::launch_snn_sort(knn.lists, knn.len, N, k, nbr, st));
        GSIM_HIP(hipEventRecord(ev_sort.b, st));
        gsim::SnnArgs a{};
        a.lists = knn.lists;
        a.len = knn.len;
        a.nbr = nbr;
        a.nrows = N;
        a.k = k;
        a.flags = flags;
        a.nlevels = nlevels;
        for (uint32_t l = 0; l < nlevels; l++) a.kmins[l] = kmins[l];
        a.parent = parent;
        a.shared = shared;
        a.counters = knn.word(knn.back_at());
        GSIM_HIP(hipEventRecord(ev_link.a, st));
        GSIM_HIP(gsim::launch_snn_link(a, s.num_cus / std::max(s.cu_share, 1), st));
        if (parent) GSIM_HIP(gsim::launch_comp_flatten(parent, N, nlevels, st));
        GSIM_HIP(hipEventRecord(ev_link.b, st));
        return GSIM_OK;
    }

    // the stats both calls fill from the control block (read back by the caller, the stream waited for)
    void fill(const unsigned long long* h_ctl, uint64_t N, uint32_t k, uint32_t nlevels, gsim_snn_stats* st)
    {
        const unsigned long long* c = h_ctl + knn.back_at();
        st->rows = N;
        st->k = k;
        st->entries = c[gsim::kSnnEntries];
        st->mutual_entries = c[gsim::kSnnMutual];
        for (uint32_t l = 0; l < nlevels; l++) st->links[l] = c[gsim::kSnnLinks + l];
        st->unions = c[gsim::kSnnUnions];
        st->cas_failed = c[gsim::kSnnCasFailed];
        st->launches = knn.plan.size();
        st->pairs = N * N;
        st->inserts = h_ctl[0];
        st->knn_ms = knn.ev_fold.ms();
        st->sort_ms = ev_sort.ms();
        st->link_ms = ev_link.ms();
        knn.add_clocks(h_ctl);
        st->clock_mhz = knn.clocks.mhz();
    }
};

int snn(gsim_db* db, Shard& s, uint32_t k, float cutoff, int metric, float alpha, float beta, uint32_t flags, gsim_graph* g)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    g->kind = gsim_graph::Kind::kSnn;
    g->snn.rows = N;
    g->snn.k = k;
    g->indptr.assign(N + 1, 0);
    if (N < 2) {
        g->snn.wall_ms = g->stats.wall_ms = ms_since(t0);
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    SnnPass pass;
    DevBuf<uint32_t> d_shared, d_out;
    DevBuf<uint64_t> d_indptr;
    size_t scan_bytes = 0;
    GSIM_HIP(gsim::knn_scan_bytes(N + 1, &scan_bytes));
    GSIM_ALLOC(d_shared, N * k * 4, "the shared-neighbour counts");
    GSIM_ALLOC(d_indptr, (N + 1) * 8, "the shared-neighbour graph (row offsets)");
    if (const int rc = pass.run(db, s, k, cutoff, metric, alpha, beta, flags, nullptr, 0, nullptr, d_shared, scan_bytes)) return rc;

    KnnCsr csr;
    if (const int rc = build_knn_csr(db, s, pass.knn.lists, pass.knn.len, N, k, pass.tmp, d_indptr, pass.knn.ctl, "the shared-neighbour CSR", "snn", g, &csr))
        return rc;
    // the counts by the same offsets
    EventPair ev_d2h;
    GSIM_HIP(ev_d2h.create());
    GSIM_ALLOC(d_out, csr.total * 4, "the shared-neighbour CSR (counts)");
    g->shared.resize(csr.total);
    GSIM_HIP(gsim::launch_snn_compact(d_shared, pass.knn.len, d_indptr, N, k, d_out, st));
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    if (csr.total) GSIM_HIP(hipMemcpyAsync(g->shared.data(), d_out, csr.total * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st));

    gsim_snn_stats& ss = g->snn;
    pass.fill(csr.ctl.data(), N, k, 0, &ss);
    if (ss.entries != csr.total) return fail(GSIM_ERR_STATE, "snn: the link pass and the CSR disagree on the number of entries");
    ss.label_ms = csr.csr_ms;
    ss.d2h_ms = csr.d2h_ms + ev_d2h.ms();
    ss.wall_ms = ms_since(t0);
    gsim_graph_stats& gs = g->stats;
    gs.launches = ss.launches;
    gs.pairs = ss.entries;
    gs.tile_ms = ss.knn_ms;
    gs.csr_ms = ss.label_ms;
    gs.d2h_ms = ss.d2h_ms;
    gs.clock_mhz = ss.clock_mhz;
    gs.wall_ms = ss.wall_ms;
    return GSIM_OK;
}

int jarvis_patrick(gsim_db* db, Shard& s, uint32_t k, const uint32_t* kmins, uint32_t nlevels, float cutoff, int metric, float alpha, float beta,
                   uint32_t flags, uint32_t* cluster_of, uint32_t* nclusters, uint32_t* first_row, uint32_t* sizes, gsim_snn_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    if (N == 1) { // no neighbour, no launch: one singleton at every level
        for (uint32_t l = 0; l < nlevels; l++) {
            cluster_of[l] = 0;
            nclusters[l] = 1;
            if (first_row) first_row[l] = db->row_base;
            if (sizes) sizes[l] = 1;
        }
        if (stats) {
            stats->rows = 1;
            stats->k = k;
            stats->wall_ms = ms_since(t0);
        }
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    SnnPass pass;
    DevBuf<uint32_t> parent;
    ForestLabels labels;
    size_t scan_bytes = 0;
    GSIM_HIP(gsim::scan_u32_bytes(N, &scan_bytes));
    GSIM_ALLOC(parent, static_cast<size_t>(N) * 4 * nlevels, "jarvis-patrick (the forests)");
    if (const int rc = labels.alloc(N, nlevels, first_row, sizes, "jarvis-patrick", "cluster_of")) return rc;
    GSIM_HIP(gsim::launch_comp_init(parent, N, nlevels, st));
    if (const int rc = pass.run(db, s, k, cutoff, metric, alpha, beta, flags, kmins, nlevels, parent, nullptr, scan_bytes)) return rc;

    // labels and outputs, as gsim_db_components
    if (const int rc = labels.run(parent, N, nlevels, db->row_base, pass.tmp, scan_bytes, pass.knn.ctl, pass.knn.ctl_words, cluster_of,
                                  first_row, sizes, st, "jarvis-patrick"))
        return rc;
    if (labels.ctl[pass.knn.back_at() + gsim::kSnnUnions] != labels.unions)
        return fail(GSIM_ERR_STATE, "jarvis-patrick: the hooks and the cluster counts do not add up");
    for (uint32_t l = 0; l < nlevels; l++) nclusters[l] = labels.ncomp[l];
    if (stats) {
        pass.fill(labels.ctl.data(), N, k, nlevels, stats);
        stats->label_ms = labels.ev_label.ms();
        stats->d2h_ms = labels.ev_d2h.ms();
        stats->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_snn(gsim_db* db, uint32_t k, float cutoff, int metric, float alpha, float beta, uint32_t flags, gsim_graph** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_k_cutoff("snn", k, cutoff)) return rc;
    if (const int rc = check_metric("snn", metric, alpha, beta)) return rc;
    if (flags & ~GSIM_SNN_CLOSED) return fail(GSIM_ERR_INVALID, "snn: unknown flags");
    if (const int rc = check_tile_table(db, "snn")) return rc;
    if (const int rc = check_table_state(db, "snn", false)) return rc;
    const char* nomem = "host memory for the shared-neighbour graph";
    return on_one_shard(db, nomem, [&](Shard& s) {
        return make_graph(out, nomem, [&](gsim_graph* g) { return snn(db, s, k, cutoff, metric, alpha, beta, flags, g); });
    });
}

int gsim_graph_copy_shared(const gsim_graph* g, uint32_t* shared)
{
    if (!g) return fail(GSIM_ERR_INVALID, "NULL graph");
    if (g->kind != gsim_graph::Kind::kSnn) return fail(GSIM_ERR_INVALID, "not the result of gsim_db_snn");
    if (!g->shared.empty() && !shared) return fail(GSIM_ERR_INVALID, "NULL shared");
    if (!g->shared.empty()) std::memcpy(shared, g->shared.data(), g->shared.size() * sizeof(uint32_t));
    return GSIM_OK;
}

int gsim_graph_get_snn_stats(const gsim_graph* g, gsim_snn_stats* out)
{
    if (!g || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (g->kind != gsim_graph::Kind::kSnn) return fail(GSIM_ERR_INVALID, "not the result of gsim_db_snn");
    *out = g->snn;
    return GSIM_OK;
}

int gsim_db_jarvis_patrick(gsim_db* db, uint32_t k, const uint32_t* kmins, uint32_t nlevels, float cutoff, int metric, float alpha, float beta,
                           uint32_t flags, uint32_t* cluster_of, uint32_t* nclusters, uint32_t* first_row, uint32_t* sizes, gsim_snn_stats* stats)
{
    if (stats) *stats = gsim_snn_stats{};
    if (!db) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_k_cutoff("jarvis-patrick", k, cutoff)) return rc;
    if (const int rc = check_metric("jarvis-patrick", metric, alpha, beta)) return rc;
    if (flags & ~(GSIM_SNN_CLOSED | GSIM_SNN_EITHER)) return fail(GSIM_ERR_INVALID, "jarvis-patrick: unknown flags");
    if (!kmins || !nclusters || (db->nrows && !cluster_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nlevels < 1 || nlevels > GSIM_COMPONENTS_MAX_LEVELS) return fail(GSIM_ERR_INVALID, "jarvis-patrick: between 1 and 8 levels");
    const uint32_t kmax = k + ((flags & GSIM_SNN_CLOSED) ? 2u : 0u);
    for (uint32_t l = 0; l < nlevels; l++) {
        if (kmins[l] > kmax) return fail(GSIM_ERR_INVALID, "jarvis-patrick: every kmin must be in [0, k], or [0, k + 2] with GSIM_SNN_CLOSED");
        if (l && !(kmins[l - 1] < kmins[l])) return fail(GSIM_ERR_INVALID, "jarvis-patrick: kmins must be strictly ascending");
    }
    if (const int rc = check_tile_table(db, "jarvis-patrick")) return rc;
    for (uint32_t l = 0; l < nlevels; l++) nclusters[l] = 0;
    if (db->nrows == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "jarvis-patrick", false)) return rc;
    return on_one_shard(db, "host memory for jarvis-patrick", [&](Shard& s) {
        return jarvis_patrick(db, s, k, kmins, nlevels, cutoff, metric, alpha, beta, flags, cluster_of, nclusters, first_row, sizes, stats);
    });
}

} // extern "C"
