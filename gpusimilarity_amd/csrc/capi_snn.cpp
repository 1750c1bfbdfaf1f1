// capi_snn.cpp -- gsim_db_snn (gsim_db_knn's graph with the shared-nearest-neighbour count of every entry) and gsim_db_jarvis_patrick
// (Jarvis-Patrick clustering at up to eight kmin levels; the graph never leaves the device).  The argument checks and the launch
// sequence of a call: gsim_db_knn's fold over all rows (knn_args, run_knn_fold: capi_knn.cpp), the sort and link kernels of
// gsim_snn.hip, then either the k-NN calls' CSR tail (build_knn_csr) or gsim_db_components' flatten and labelling.  The rule is
// stated in include/gpusim_hip.h; the host functions of the same rule are in capi_snn_host.cpp.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

// What both calls do first: the lists of all N >= 2 rows, their rows sorted, and the link pass.  The control block: [0] the fold's
// insert counter, 4 clock stamps per fold launch, then the link kernel's kSnnCounters.
struct SnnPass {
    PaddedRows table;
    DevBuf<> ctl, tmp;
    DevBuf<gsim::KnnEntry> lists;
    DevBuf<uint32_t> len, nbr;
    std::vector<KnnLaunch> plan;
    LaunchClocks clocks;
    EventPair ev_fold, ev_sort, ev_link;
    size_t ctl_words = 0, tmp_bytes = 0;

    size_t counters_at() const { return 1 + LaunchClocks::kWords * plan.size(); }

    // `parent`: nlevels initialised forests, flattened here after the link launch (or nullptr); `shared`: N x k words (or nullptr)
    int run(gsim_db* db, Shard& s, uint32_t k, float cutoff, int metric, float alpha, float beta, uint32_t flags, const uint32_t* kmins,
            uint32_t nlevels, uint32_t* parent, uint32_t* shared, size_t scan_bytes)
    {
        const uint64_t N = s.nrows;
        const uint32_t WP = gsim::nbr_padded_words(s.W);
        const hipStream_t st = s.stream;
        plan = plan_knn(N, N, WP, db->knobs.knn_launch_pairs);
        ctl_words = counters_at() + gsim::kSnnCounters;
        tmp_bytes = scan_bytes;
        if (const int rc = table.alloc(N, s.W, WP, "the shared-neighbour pass (popcounts)", "the shared-neighbour pass (padded rows)")) return rc;
        GSIM_ALLOC(lists, N * k * sizeof(gsim::KnnEntry), "the shared-neighbour pass (the k-nearest-neighbour lists)");
        GSIM_ALLOC(len, (N + 1) * 4, "the shared-neighbour pass (the lists' lengths)");
        GSIM_ALLOC(nbr, N * k * 4, "the shared-neighbour pass (the sorted lists)");
        GSIM_ALLOC(ctl, ctl_words * 8, "the shared-neighbour pass (control block)");
        GSIM_ALLOC(tmp, tmp_bytes, "the shared-neighbour pass (scan scratch)");
        unsigned long long* d_ctl = ctl.as<unsigned long long>();
        clocks.view(d_ctl + 1);
        GSIM_HIP(hipMemsetAsync(len, 0, (N + 1) * 4, st));
        GSIM_HIP(hipMemsetAsync(ctl, 0, ctl_words * 8, st));
        if (const int rc = table.prepare(s.d_rows, N, st)) return rc;
        if (const int rc = run_knn_fold(knn_args(table, N, 0, N, WP, k, cutoff, metric, alpha, beta, lists, len, d_ctl), plan, clocks, ev_fold, st))
            return rc;
        GSIM_HIP(ev_sort.create());
        GSIM_HIP(ev_link.create());
        GSIM_HIP(hipEventRecord(ev_sort.a, st));
        GSIM_HIP(gsim::launch_snn_sort(lists, len, N, k, nbr, st));
        GSIM_HIP(hipEventRecord(ev_sort.b, st));
        gsim::SnnArgs a{};
        a.lists = lists;
        a.len = len;
        a.nbr = nbr;
        a.nrows = N;
        a.k = k;
        a.flags = flags;
        a.nlevels = nlevels;
        for (uint32_t l = 0; l < nlevels; l++) a.kmins[l] = kmins[l];
        a.parent = parent;
        a.shared = shared;
        a.counters = d_ctl + counters_at();
        GSIM_HIP(hipEventRecord(ev_link.a, st));
        GSIM_HIP(gsim::launch_snn_link(a, s.num_cus / std::max(s.cu_share, 1), st));
        if (parent) GSIM_HIP(gsim::launch_comp_flatten(parent, N, nlevels, st));
        GSIM_HIP(hipEventRecord(ev_link.b, st));
        return GSIM_OK;
    }

    // the stats both calls fill from the control block (read back by the caller, the stream waited for)
    void fill(const unsigned long long* h_ctl, uint64_t N, uint32_t k, uint32_t nlevels, gsim_snn_stats* st)
    {
        const unsigned long long* c = h_ctl + counters_at();
        st->rows = N;
        st->k = k;
        st->entries = c[gsim::kSnnEntries];
        st->mutual_entries = c[gsim::kSnnMutual];
        for (uint32_t l = 0; l < nlevels; l++) st->links[l] = c[gsim::kSnnLinks + l];
        st->unions = c[gsim::kSnnUnions];
        st->cas_failed = c[gsim::kSnnCasFailed];
        st->launches = plan.size();
        st->pairs = N * N;
        st->inserts = h_ctl[0];
        st->knn_ms = ev_fold.ms();
        st->sort_ms = ev_sort.ms();
        st->link_ms = ev_link.ms();
        clocks.add(h_ctl + 1, plan.size());
        st->clock_mhz = clocks.mhz();
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
    if (const int rc = build_knn_csr(db, s, pass.lists, pass.len, N, k, pass.tmp, d_indptr, pass.ctl, "the shared-neighbour CSR", "snn", g, &csr))
        return rc;
    // the counts by the same offsets
    EventPair ev_d2h;
    GSIM_HIP(ev_d2h.create());
    GSIM_ALLOC(d_out, csr.total * 4, "the shared-neighbour CSR (counts)");
    g->shared.resize(csr.total);
    GSIM_HIP(gsim::launch_snn_compact(d_shared, pass.len, d_indptr, N, k, d_out, st));
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
    DevBuf<uint32_t> parent, d_comp, d_first, d_sizes, d_ncomp, d_flag, d_num;
    const size_t stripe = static_cast<size_t>(N) * 4, all = stripe * nlevels;
    size_t scan_bytes = 0;
    GSIM_HIP(gsim::comp_scan_bytes(N, &scan_bytes));
    GSIM_ALLOC(parent, all, "jarvis-patrick (the forests)");
    GSIM_ALLOC(d_comp, all, "jarvis-patrick (cluster_of)");
    if (first_row) GSIM_ALLOC(d_first, all, "jarvis-patrick (first_row)");
    if (sizes) GSIM_ALLOC(d_sizes, all, "jarvis-patrick (sizes)");
    GSIM_ALLOC(d_ncomp, gsim::kCompMaxLevels * 4, "jarvis-patrick (the counts)");
    GSIM_ALLOC(d_flag, stripe, "jarvis-patrick (label scratch)");
    GSIM_ALLOC(d_num, stripe, "jarvis-patrick (label scratch)");
    GSIM_HIP(gsim::launch_comp_init(parent, N, nlevels, st));
    if (const int rc = pass.run(db, s, k, cutoff, metric, alpha, beta, flags, kmins, nlevels, parent, nullptr, scan_bytes)) return rc;

    // labels, on the device, a level at a time; then the outputs, as gsim_db_components
    EventPair ev_label, ev_d2h;
    GSIM_HIP(ev_label.create());
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipEventRecord(ev_label.a, st));
    if (sizes) GSIM_HIP(hipMemsetAsync(d_sizes, 0, all, st));
    for (uint32_t l = 0; l < nlevels; l++)
        GSIM_HIP(gsim::launch_comp_label(pass.tmp, pass.tmp_bytes, parent + l * N, N, db->row_base, d_flag, d_num, d_comp + l * N,
                                         first_row ? d_first + l * N : nullptr, sizes ? d_sizes + l * N : nullptr, d_ncomp + l, st));
    GSIM_HIP(hipEventRecord(ev_label.b, st));
    std::vector<unsigned long long> h_ctl(pass.ctl_words);
    uint32_t h_ncomp[gsim::kCompMaxLevels] = {};
    GSIM_HIP(hipEventRecord(ev_d2h.a, st));
    GSIM_HIP(hipMemcpyAsync(h_ncomp, d_ncomp, nlevels * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(h_ctl.data(), pass.ctl, h_ctl.size() * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(cluster_of, d_comp, all, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    uint64_t unions = 0;
    for (uint32_t l = 0; l < nlevels; l++) {
        if (h_ncomp[l] < 1 || h_ncomp[l] > N) return fail(GSIM_ERR_STATE, "jarvis-patrick: the device reported an impossible count");
        unions += N - h_ncomp[l];
        // (entries at and after nclusters[l] of a stripe are left untouched)
        if (first_row) GSIM_HIP(hipMemcpyAsync(first_row + l * N, d_first + l * N, static_cast<size_t>(h_ncomp[l]) * 4, hipMemcpyDeviceToHost, st));
        if (sizes) GSIM_HIP(hipMemcpyAsync(sizes + l * N, d_sizes + l * N, static_cast<size_t>(h_ncomp[l]) * 4, hipMemcpyDeviceToHost, st));
    }
    GSIM_HIP(hipEventRecord(ev_d2h.b, st));
    GSIM_HIP(hipStreamSynchronize(st));
    if (h_ctl[pass.counters_at() + gsim::kSnnUnions] != unions)
        return fail(GSIM_ERR_STATE, "jarvis-patrick: the hooks and the cluster counts do not add up");
    for (uint32_t l = 0; l < nlevels; l++) nclusters[l] = h_ncomp[l];
    if (stats) {
        pass.fill(h_ctl.data(), N, k, nlevels, stats);
        stats->label_ms = ev_label.ms();
        stats->d2h_ms = ev_d2h.ms();
        stats->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

// gsim_db_knn's checks of k, cutoff and metric, then the flags
int check_lists(const char* name, uint32_t k, float cutoff, int metric, float alpha, float beta, uint32_t flags, uint32_t known)
{
    const std::string n(name);
    if (k < 1 || k > GSIM_KNN_MAX_K) return fail(GSIM_ERR_INVALID, n + ": k must be in [1, GSIM_KNN_MAX_K = 128]");
    if (!(cutoff > 0.0f && cutoff <= 1.0f)) return fail(GSIM_ERR_INVALID, n + ": the cutoff must be in (0, 1]");
    if (const int rc = check_metric(name, metric, alpha, beta)) return rc;
    if (flags & ~known) return fail(GSIM_ERR_INVALID, n + ": unknown flags");
    return GSIM_OK;
}

int check_table(const gsim_db* db, const char* name)
{
    const std::string n(name);
    if (db->fp_bits > 4096 || gsim::nbr_padded_words(db->W) == 0) return fail(GSIM_ERR_INVALID, n + ": rows wider than 4096 bits");
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, n + ": tables of 2^32 rows or more");
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
    if (const int rc = check_lists("snn", k, cutoff, metric, alpha, beta, flags, GSIM_SNN_CLOSED)) return rc;
    if (const int rc = check_table(db, "snn")) return rc;
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
    if (const int rc = check_lists("jarvis-patrick", k, cutoff, metric, alpha, beta, flags, GSIM_SNN_CLOSED | GSIM_SNN_EITHER)) return rc;
    if (!kmins || !nclusters || (db->nrows && !cluster_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nlevels < 1 || nlevels > GSIM_COMPONENTS_MAX_LEVELS) return fail(GSIM_ERR_INVALID, "jarvis-patrick: between 1 and 8 levels");
    const uint32_t kmax = k + ((flags & GSIM_SNN_CLOSED) ? 2u : 0u);
    for (uint32_t l = 0; l < nlevels; l++) {
        if (kmins[l] > kmax) return fail(GSIM_ERR_INVALID, "jarvis-patrick: every kmin must be in [0, k], or [0, k + 2] with GSIM_SNN_CLOSED");
        if (l && !(kmins[l - 1] < kmins[l])) return fail(GSIM_ERR_INVALID, "jarvis-patrick: kmins must be strictly ascending");
    }
    if (const int rc = check_table(db, "jarvis-patrick")) return rc;
    for (uint32_t l = 0; l < nlevels; l++) nclusters[l] = 0;
    if (db->nrows == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "jarvis-patrick", false)) return rc;
    return on_one_shard(db, "host memory for jarvis-patrick", [&](Shard& s) {
        return jarvis_patrick(db, s, k, kmins, nlevels, cutoff, metric, alpha, beta, flags, cluster_of, nclusters, first_row, sizes, stats);
    });
}

} // extern "C"
