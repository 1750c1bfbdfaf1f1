// capi_hdbscan.cpp -- HDBSCAN on a resident table: gsim_db_core_scores (the core pass: KnnListPass over all rows and a tail kernel
// that reads the lists' last entries), gsim_db_mreach_mst (the core pass, then gsim_db_mst's round loop -- boruvka_forest,
// capi_mst.cpp -- with the mutual-reachability fold kernel), gsim_db_hdbscan (that forest, then the selection), and the host
// companions gsim_mreach_mst (the forest's rule on a scored CSR graph) and gsim_mst_hdbscan (the condensed tree and the selection
// of clusters from any forest in order E).  The device side is gsim_mreach.hip.  The rule is stated in include/gpusim_hip.h.
#include "capi_front.h"

#include <algorithm>
#include <cmath>

namespace gsim_host
{
namespace
{

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct CorePass {
    uint64_t launches = 0, inserts = 0, dense = 0;
    double kernel_ms = 0.0, tail_ms = 0.0, clock_mhz = 0.0;
};

// d_core[0 .. N) on the device from the prepared table: the k-NN list pass of all N owners with k = min_pts - 1 (KnnListPass,
// capi_knn.cpp; no lists for min_pts == 1) and the tail kernel.  The lists live here only: they are freed on return, and the stream
// has been waited for.
int core_pass(gsim_db* db, const PaddedRows& table, uint64_t N, uint32_t WP, uint32_t min_pts, float cutoff, int metric, float alpha,
              float beta, float* d_core, hipStream_t st, CorePass* out)
{
    const uint32_t k = min_pts - 1;
    // [0] the insert counter, [1] the rows with core >= cutoff, then 4 clock stamps per launch; min_pts == 1: no lists, the tail alone
    KnnListPass pass;
    if (const int rc = pass.alloc(db, N, WP, 0, N, k, 2, 0, false, {"the core scores (the k-nearest-neighbour lists)",
                                  "the core scores (the lists' lengths)", "the core scores (control block)"}, st))
        return rc;
    EventPair ev_tail;
    GSIM_HIP(ev_tail.create());
    if (const int rc = pass.fold(table, cutoff, metric, alpha, beta, st)) return rc;
    GSIM_HIP(hipEventRecord(ev_tail.a, st));
    GSIM_HIP(gsim::launch_mreach_core(pass.lists, pass.len, N, k, cutoff, d_core, pass.word(1), st));
    GSIM_HIP(hipEventRecord(ev_tail.b, st));
    std::vector<unsigned long long> h_ctl(pass.ctl_words);
    GSIM_HIP(hipMemcpyAsync(h_ctl.data(), pass.ctl, pass.ctl_words * 8, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    if (h_ctl[1] > N) return fail(GSIM_ERR_STATE, "core scores: the device reported an impossible count");
    pass.add_clocks(h_ctl.data());
    out->launches = pass.plan.size();
    out->inserts = h_ctl[0];
    out->dense = h_ctl[1];
    out->kernel_ms = k ? pass.ev_fold.ms() : 0.0;
    out->tail_ms = ev_tail.ms();
    out->clock_mhz = pass.clocks.mhz();
    return GSIM_OK;
}

// a table of one row: no neighbour, no launch
float lone_core(uint32_t min_pts) { return min_pts == 1 ? 1.0f : 0.0f; }

int core_scores(gsim_db* db, Shard& s, uint32_t min_pts, float cutoff, int metric, float alpha, float beta, float* core, gsim_knn_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;
    PaddedRows table;
    DevBuf<float> d_core;
    if (const int rc = table.alloc(N, s.W, WP, "the core scores (popcounts)", "the core scores (the padded rows)")) return rc;
    GSIM_ALLOC(d_core, N * 4, "the core scores");
    if (const int rc = table.prepare(s.d_rows, N, stream)) return rc;
    CorePass cp;
    if (const int rc = core_pass(db, table, N, WP, min_pts, cutoff, metric, alpha, beta, d_core, stream, &cp)) return rc;
    EventPair ev_d2h;
    GSIM_HIP(ev_d2h.create());
    GSIM_HIP(hipEventRecord(ev_d2h.a, stream));
    GSIM_HIP(hipMemcpyAsync(core, d_core, N * 4, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipEventRecord(ev_d2h.b, stream));
    GSIM_HIP(hipStreamSynchronize(stream));
    if (st) {
        st->rows = N;
        st->launches = cp.launches;
        st->pairs = cp.launches ? N * N : 0;
        st->inserts = cp.inserts;
        st->entries = cp.dense;
        st->kernel_ms = cp.kernel_ms;
        st->csr_ms = cp.tail_ms;
        st->d2h_ms = ev_d2h.ms();
        st->clock_mhz = cp.clock_mhz;
        st->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

int mreach_forest(gsim_db* db, Shard& s, uint32_t min_pts, float cutoff, int metric, float alpha, float beta, uint32_t row_base,
                  gsim_mst_edge* edges, uint64_t* nedges, float* core, gsim_mreach_stats* st)
{
    const uint64_t N = s.nrows;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    DevBuf<float> d_core;
    CorePass cp;
    ForestFold ff;
    ff.prepare = [&](const PaddedRows& table, hipStream_t stream) {
        GSIM_ALLOC(d_core, N * 4, "the spanning forest (the core scores)");
        return core_pass(db, table, N, WP, min_pts, cutoff, metric, alpha, beta, d_core, stream, &cp);
    };
    ff.fold = [&](const gsim::MstArgs& a, uint32_t ot0, uint32_t not_, uint64_t c0, uint64_t c1, uint32_t nchunk, hipStream_t stream) {
        const gsim::MreachArgs ma{a, d_core};
        return gsim::launch_mreach_fold(ma, ot0, not_, c0, c1, nchunk, stream);
    };
    if (const int rc = boruvka_forest(db, s, cutoff, metric, alpha, beta, row_base, ff, edges, nedges, st ? &st->mst : nullptr)) return rc;
    if (N < 2) {
        if (core) core[0] = lone_core(min_pts);
        cp.dense = lone_core(min_pts) >= cutoff ? 1 : 0;
    } else if (core) {
        GSIM_HIP(hipMemcpyAsync(core, d_core, N * 4, hipMemcpyDeviceToHost, s.stream));
        GSIM_HIP(hipStreamSynchronize(s.stream));
    }
    if (st) {
        st->core_launches = cp.launches;
        st->core_inserts = cp.inserts;
        st->core_rows = cp.dense;
        st->core_kernel_ms = cp.kernel_ms;
        st->core_tail_ms = cp.tail_ms;
    }
    return GSIM_OK;
}

// ---- the condensed tree and the selection (gsim_mst_hdbscan) ----

// A node at level s of the multiway dendrogram: its children are nodes (a chain through `next`) and single rows (a chain through
// next_row[]); both chains keep their tail, so that two nodes being built at the same level join in O(1).
struct TreeNode {
    float level;
    uint32_t size = 0, minrow = kNone;
    uint32_t child_head = kNone, child_tail = kNone, next = kNone;
    uint32_t row_head = kNone, row_tail = kNone;
};

struct Cluster {
    uint32_t parent, node, size, minrow;
    float birth;
    double stability = 0.0, sub = 0.0, shat = 0.0;
    uint32_t nchild = 0, number = kNone, sel = kNone;
    bool chosen = false, covered = false;
};

struct Condenser {
    std::vector<TreeNode> nodes;
    std::vector<uint32_t> next_row, cur, last; // per row: its chain; per forest root: the component's node; the last cluster of the row
    std::vector<float> left;                   // per row: the level at which it left that cluster
    std::vector<Cluster> clusters;
    std::vector<uint32_t> stack;

    void take_row(TreeNode& v, uint32_t r)
    {
        if (v.row_head == kNone) v.row_head = r;
        else next_row[v.row_tail] = r;
        v.row_tail = r;
        v.size++;
        v.minrow = std::min(v.minrow, r);
    }
    void take_node(TreeNode& v, uint32_t c)
    {
        if (v.child_head == kNone) v.child_head = c;
        else nodes[v.child_tail].next = c;
        v.child_tail = c;
        v.size += nodes[c].size;
        v.minrow = std::min(v.minrow, nodes[c].minrow);
    }
    // the component whose root is r becomes a child of node v
    void attach(uint32_t v, uint32_t r)
    {
        if (cur[r] == kNone) take_row(nodes[v], r);
        else take_node(nodes[v], cur[r]);
    }
    // node w, built at the same level, dissolves into node v
    void absorb(uint32_t v, uint32_t w)
    {
        TreeNode &a = nodes[v], &b = nodes[w];
        if (b.child_head != kNone) {
            if (a.child_head == kNone) a.child_head = b.child_head;
            else nodes[a.child_tail].next = b.child_head;
            a.child_tail = b.child_tail;
        }
        if (b.row_head != kNone) {
            if (a.row_head == kNone) a.row_head = b.row_head;
            else next_row[a.row_tail] = b.row_head;
            a.row_tail = b.row_tail;
        }
        a.size += b.size;
        a.minrow = std::min(a.minrow, b.minrow);
    }
    // every row below node v left cluster c at level s
    void leave_all(uint32_t v, uint32_t c, float s)
    {
        stack.assign(1, v);
        while (!stack.empty()) {
            const uint32_t x = stack.back();
            stack.pop_back();
            for (uint32_t r = nodes[x].row_head; r != kNone; r = next_row[r]) {
                last[r] = c;
                left[r] = s;
            }
            for (uint32_t y = nodes[x].child_head; y != kNone; y = nodes[y].next) stack.push_back(y);
        }
    }
    uint32_t born(uint32_t parent, uint32_t node, float birth)
    {
        Cluster c{};
        c.parent = parent;
        c.node = node;
        c.size = nodes[node].size;
        c.minrow = nodes[node].minrow;
        c.birth = birth;
        clusters.push_back(c);
        if (parent != kNone) clusters[parent].nchild++;
        return static_cast<uint32_t>(clusters.size() - 1);
    }
};

int hdbscan_select(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows, float floor, uint32_t mcs, uint32_t flags, uint32_t* label_of,
                   uint64_t* nclusters, float* leave, uint32_t* first_row, uint32_t* sizes, float* birth, double* stability)
{
    Condenser t;
    t.nodes.reserve(nedges);
    t.next_row.assign(nrows, kNone);
    t.cur.assign(nrows, kNone);
    t.last.assign(nrows, kNone);
    t.left.assign(nrows, 0.0f);
    Forest f(nrows);
    // the multiway dendrogram, bottom-up: the edges of one score build the nodes at that level
    for (uint64_t e = 0; e < nedges; e++) {
        const float s = edges[e].score;
        if (e && s > edges[e - 1].score) return fail(GSIM_ERR_INVALID, "hdbscan: the scores of a forest's edges must not increase");
        if (!(s >= floor)) return fail(GSIM_ERR_INVALID, "hdbscan: the floor must not be above an edge score");
        const uint32_t x = f.root(edges[e].a), y = f.root(edges[e].b);
        if (x == y) return fail(GSIM_ERR_INVALID, "hdbscan: an edge whose ends are already connected");
        const bool xs = t.cur[x] != kNone && t.nodes[t.cur[x]].level == s, ys = t.cur[y] != kNone && t.nodes[t.cur[y]].level == s;
        uint32_t v;
        if (xs && ys) {
            v = t.cur[x];
            t.absorb(v, t.cur[y]);
        } else if (xs || ys) {
            v = xs ? t.cur[x] : t.cur[y];
            t.attach(v, xs ? y : x);
        } else {
            v = static_cast<uint32_t>(t.nodes.size());
            TreeNode n{};
            n.level = s;
            t.nodes.push_back(n);
            t.attach(v, x);
            t.attach(v, y);
        }
        f.unite(x, y);
        t.cur[std::min(x, y)] = v;
    }
    // the clusters, top-down: a root cluster per tree of at least mcs rows (a forest root is its tree's smallest row)
    std::vector<uint32_t> work, large;
    for (uint64_t r = 0; r < nrows; r++) {
        const uint32_t v = t.cur[r];
        if (f.parent[r] == r && v != kNone && t.nodes[v].size >= mcs) work.push_back(t.born(kNone, v, floor));
    }
    while (!work.empty()) {
        const uint32_t c = work.back();
        work.pop_back();
        const double b = static_cast<double>(t.clusters[c].birth);
        double stab = 0.0;
        for (uint32_t v = t.clusters[c].node;;) {
            const float s = t.nodes[v].level;
            const double gain = static_cast<double>(s) - b;
            large.clear();
            uint64_t kept = 0;
            for (uint32_t y = t.nodes[v].child_head; y != kNone; y = t.nodes[y].next) {
                if (t.nodes[y].size >= mcs) {
                    large.push_back(y);
                    kept += t.nodes[y].size;
                } else t.leave_all(y, c, s);
            }
            for (uint32_t r = t.nodes[v].row_head; r != kNone; r = t.next_row[r]) {
                t.last[r] = c;
                t.left[r] = s;
            }
            stab += static_cast<double>(t.nodes[v].size - kept) * gain;
            if (large.empty()) break;
            if (large.size() == 1) {
                v = large[0];
                continue;
            }
            stab += static_cast<double>(kept) * gain;
            for (const uint32_t y : large) work.push_back(t.born(c, y, s));
            break;
        }
        t.clusters[c].stability = stab;
    }
    // the selection, bottom-up (a cluster's children have larger indices), then top-down: a chosen cluster below a chosen one is not selected
    std::vector<Cluster>& cl = t.clusters;
    const bool leaf_mode = (flags & 1u) == GSIM_HDBSCAN_LEAF, no_roots = (flags & GSIM_HDBSCAN_NO_ROOTS) != 0;
    for (size_t c = cl.size(); c-- > 0;) {
        const bool leaf = cl[c].nchild == 0;
        cl[c].chosen = leaf || (!leaf_mode && cl[c].stability >= cl[c].sub);
        if (no_roots && cl[c].parent == kNone && !leaf) cl[c].chosen = false;
        cl[c].shat = cl[c].chosen ? cl[c].stability : cl[c].sub;
        if (cl[c].parent != kNone) cl[cl[c].parent].sub += cl[c].shat;
    }
    std::vector<uint32_t> selected;
    for (size_t c = 0; c < cl.size(); c++) {
        const bool above = cl[c].parent != kNone && cl[cl[c].parent].covered;
        const bool sel = cl[c].chosen && !above;
        cl[c].covered = sel || above;
        cl[c].sel = sel ? static_cast<uint32_t>(c) : (cl[c].parent != kNone ? cl[cl[c].parent].sel : kNone);
        if (sel) selected.push_back(static_cast<uint32_t>(c));
    }
    std::sort(selected.begin(), selected.end(), [&](uint32_t x, uint32_t y) { return cl[x].minrow < cl[y].minrow; });
    for (size_t n = 0; n < selected.size(); n++) {
        const Cluster& c = cl[selected[n]];
        cl[selected[n]].number = static_cast<uint32_t>(n);
        if (first_row) first_row[n] = c.minrow;
        if (sizes) sizes[n] = c.size;
        if (birth) birth[n] = c.birth;
        if (stability) stability[n] = c.stability;
    }
    for (uint64_t r = 0; r < nrows; r++) {
        const uint32_t in = t.last[r] == kNone ? kNone : cl[t.last[r]].sel;
        label_of[r] = in == kNone ? GSIM_HDBSCAN_NOISE : cl[in].number;
        if (leave) leave[r] = t.left[r];
    }
    *nclusters = selected.size();
    return GSIM_OK;
}

int check_selection(uint32_t min_cluster_size, uint32_t flags)
{
    if (min_cluster_size < 2) return fail(GSIM_ERR_INVALID, "hdbscan: min_cluster_size must be at least 2");
    if (flags > (GSIM_HDBSCAN_LEAF | GSIM_HDBSCAN_NO_ROOTS)) return fail(GSIM_ERR_INVALID, "hdbscan: unknown flags");
    return GSIM_OK;
}

// the checks the three device calls share, gsim_db_mst's with min_pts
int check_call(const gsim_db* db, const char* name, uint32_t min_pts, float cutoff, int metric, float alpha, float beta)
{
    const std::string n(name);
    if (min_pts < 1 || min_pts > GSIM_KNN_MAX_K + 1) return fail(GSIM_ERR_INVALID, n + ": min_pts must be in [1, GSIM_KNN_MAX_K + 1 = 129]");
    if (const int rc = check_cutoff(name, cutoff)) return rc;
    if (const int rc = check_symmetric_metric((n + " needs").c_str(), name, metric, alpha, beta)) return rc;
    return check_tile_table(db, name);
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_core_scores(gsim_db* db, uint32_t min_pts, float cutoff, int metric, float alpha, float beta, float* core, gsim_knn_stats* stats)
{
    if (stats) *stats = gsim_knn_stats{};
    if (!db) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_call(db, "core scores", min_pts, cutoff, metric, alpha, beta)) return rc;
    if (db->nrows && !core) return fail(GSIM_ERR_INVALID, "NULL core");
    if (db->nrows == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "core scores", true)) return rc;
    return on_one_shard(db, "host memory for the core scores",
                        [&](Shard& s) { return core_scores(db, s, min_pts, cutoff, metric, alpha, beta, core, stats); });
}

int gsim_db_mreach_mst(gsim_db* db, uint32_t min_pts, float cutoff, int metric, float alpha, float beta, gsim_mst_edge* edges, uint64_t* nedges,
                       float* core, gsim_mreach_stats* stats)
{
    if (stats) *stats = gsim_mreach_stats{};
    if (nedges) *nedges = 0;
    if (!db || !nedges) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_call(db, "mreach mst", min_pts, cutoff, metric, alpha, beta)) return rc;
    if (db->nrows > 1 && !edges) return fail(GSIM_ERR_INVALID, "NULL edges");
    if (db->nrows == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "mreach mst", false)) return rc;
    return on_one_shard(db, "host memory for the spanning forest", [&](Shard& s) {
        return mreach_forest(db, s, min_pts, cutoff, metric, alpha, beta, db->row_base, edges, nedges, core, stats);
    });
}

int gsim_db_hdbscan(gsim_db* db, uint32_t min_pts, uint32_t min_cluster_size, float cutoff, int metric, float alpha, float beta, uint32_t flags,
                    uint32_t* label_of, uint64_t* nclusters, float* leave, uint32_t* first_row, uint32_t* sizes, float* birth, double* stability,
                    gsim_hdbscan_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (stats) *stats = gsim_hdbscan_stats{};
    if (nclusters) *nclusters = 0;
    if (!db || !nclusters || (db->nrows && !label_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_call(db, "hdbscan", min_pts, cutoff, metric, alpha, beta)) return rc;
    if (const int rc = check_selection(min_cluster_size, flags)) return rc;
    const uint64_t N = db->nrows;
    if (N == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "hdbscan", false)) return rc;
    return on_one_shard(db, "host memory for hdbscan", [&](Shard& s) {
        // the forest without the row base: the selection works on table rows
        std::vector<gsim_mst_edge> edges(N - 1);
        uint64_t nedges = 0;
        gsim_mreach_stats fs{};
        if (const int rc = mreach_forest(db, s, min_pts, cutoff, metric, alpha, beta, 0, edges.data(), &nedges, nullptr, &fs)) return rc;
        const auto t1 = std::chrono::steady_clock::now();
        if (const int rc = hdbscan_select(edges.data(), nedges, N, cutoff, min_cluster_size, flags, label_of, nclusters, leave, first_row, sizes,
                                          birth, stability))
            return rc;
        for (uint64_t c = 0; first_row && c < *nclusters; c++) first_row[c] += db->row_base;
        if (stats) {
            stats->forest = fs;
            stats->clusters = *nclusters;
            for (uint64_t r = 0; r < N; r++) stats->noise += label_of[r] == GSIM_HDBSCAN_NOISE;
            stats->select_ms = ms_since(t1);
            stats->wall_ms = ms_since(t0);
        }
        return static_cast<int>(GSIM_OK);
    });
}

int gsim_mreach_mst(const uint64_t* indptr, const uint32_t* indices, const float* scores, uint64_t nrows, uint32_t min_pts, gsim_mst_edge* edges,
                    uint64_t* nedges, float* core)
{
    if (nedges) *nedges = 0;
    if (!indptr || !nedges) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (min_pts == 0) return fail(GSIM_ERR_INVALID, "mreach mst: min_pts must be at least 1");
    uint64_t nnz = 0;
    if (const int rc = check_scored_csr(indptr, indices, scores, nrows, edges, &nnz)) return rc;
    try {
        // core: the (min_pts - 1)-th largest score of the row's list without its self edges; `dense`: the list is that long
        const uint64_t k = min_pts - 1;
        std::vector<float> own(nrows), list;
        std::vector<uint8_t> dense(nrows);
        for (uint64_t r = 0; r < nrows; r++) {
            list.clear();
            for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++)
                if (indices[e] != r) list.push_back(scores[e]);
            dense[r] = list.size() >= k;
            own[r] = 1.0f;
            if (k && dense[r]) {
                std::nth_element(list.begin(), list.begin() + static_cast<std::ptrdiff_t>(k - 1), list.end(), std::greater<float>());
                own[r] = list[k - 1];
            }
            if (!dense[r]) own[r] = 0.0f;
            if (core) core[r] = own[r];
        }
        std::vector<gsim_mst_edge> all;
        all.reserve(nnz);
        for (uint64_t r = 0; r < nrows; r++)
            for (uint64_t e = indptr[r]; dense[r] && e < indptr[r + 1]; e++) {
                const uint32_t i = static_cast<uint32_t>(r), j = indices[e];
                // (min_pts == 1 caps nothing, whatever the caller's scores are: gsim_mst's edges)
                const float m = k ? std::min(scores[e], std::min(own[i], own[j])) : scores[e];
                if (i != j && dense[j]) all.push_back({std::min(i, j), std::max(i, j), m});
            }
        *nedges = kruskal_in_e(all, nrows, edges);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "mreach mst");
    }
    return GSIM_OK;
}

int gsim_mst_hdbscan(const gsim_mst_edge* edges, uint64_t nedges, uint64_t nrows, float floor, uint32_t min_cluster_size, uint32_t flags,
                     uint32_t* label_of, uint64_t* nclusters, float* leave, uint32_t* first_row, uint32_t* sizes, float* birth, double* stability)
{
    if (nclusters) *nclusters = 0;
    if (!nclusters || (nrows && !label_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_edges(edges, nedges, nrows)) return rc;
    if (nedges && nedges >= nrows) return fail(GSIM_ERR_INVALID, "hdbscan: a forest over nrows rows has fewer than nrows edges");
    if (std::isnan(floor)) return fail(GSIM_ERR_INVALID, "hdbscan: a NaN floor");
    if (const int rc = check_selection(min_cluster_size, flags)) return rc;
    try {
        return hdbscan_select(edges, nedges, nrows, floor, min_cluster_size, flags, label_of, nclusters, leave, first_row, sizes, birth, stability);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "hdbscan");
    }
}

} // extern "C"
