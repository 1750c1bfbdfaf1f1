// capi_components.cpp -- gsim_db_components (single-linkage clustering: the connected components of the threshold graph at up to
// eight cutoffs, in one pass over the pairs; the labelling tail is ForestLabels, capi_front.h) and gsim_components (the same rule on a
// symmetric CSR graph, host code).  The device side is gsim_components.hip.  The rule is stated in include/gpusim_hip.h.
#include "capi_front.h"

#include <cmath>

namespace gsim_host
{
namespace
{

int components(gsim_db* db, Shard& s, const float* cutoffs, uint32_t nlevels, int metric, float alpha, float beta, uint32_t* component_of,
               uint32_t* ncomponents, uint32_t* first_row, uint32_t* sizes, gsim_components_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;

    const uint64_t nt = (N + gsim::kNbrTile - 1) / gsim::kNbrTile;
    const std::vector<NbrLaunch> plan =
        N < 2 ? std::vector<NbrLaunch>() : plan_launches(nt, nt, true, WP, static_cast<uint64_t>(db->knobs.components_launch_pairs));
    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::scan_u32_bytes(N, &tmp_bytes));
    PaddedRows table;
    DevBuf<uint32_t> parent;
    ForestLabels labels;
    DevBuf<unsigned long long> ctl; // the counters, then 4 clock stamps per launch
    DevBuf<> tmp;
    if (const int rc = table.alloc(N, s.W, WP, "components (popcounts)", "components (the padded rows)")) return rc;
    GSIM_ALLOC(parent, static_cast<size_t>(N) * 4 * nlevels, "components (the forests)");
    if (const int rc = labels.alloc(N, nlevels, first_row, sizes, "components", "component_of")) return rc;
    GSIM_ALLOC(ctl, (gsim::kCompCounters + 4 * plan.size()) * 8, "components (control block)");
    GSIM_ALLOC(tmp, tmp_bytes, "components (scan scratch)");
    LaunchClocks clocks;
    clocks.view(ctl + gsim::kCompCounters);

    gsim::CompArgs a{};
    a.nrows = N;
    a.WP = WP;
    a.nlevels = nlevels;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    for (uint32_t l = 0; l < gsim::kCompMaxLevels; l++) a.cutoffs[l] = cutoffs[l < nlevels ? l : nlevels - 1];
    a.parent = parent;
    a.counters = ctl;

    EventPair ev_kernel;
    GSIM_HIP(ev_kernel.create());
    GSIM_HIP(hipMemsetAsync(ctl, 0, (gsim::kCompCounters + 4 * plan.size()) * 8, stream));
    if (const int rc = table.prepare(s.d_rows, N, stream)) return rc;
    a.rows = table.rows();
    a.pop = table.pop();
    GSIM_HIP(gsim::launch_comp_init(parent, N, nlevels, stream));
    // the pass: every launch is followed by the flatten (all path shortening is there; after the last launch it leaves
    // parent[x] = the smallest row of x's component)
    GSIM_HIP(hipEventRecord(ev_kernel.a, stream));
    for (size_t l = 0; l < plan.size(); l++) {
        gsim::CompArgs al = a;
        al.clk = clocks.at(l);
        GSIM_HIP(gsim::launch_comp_tiles(al, plan[l].rt0, plan[l].nrt, plan[l].ct0, plan[l].nct, stream));
        GSIM_HIP(gsim::launch_comp_flatten(parent, N, nlevels, stream));
    }
    GSIM_HIP(hipEventRecord(ev_kernel.b, stream));
    if (const int rc = labels.run(parent, N, nlevels, db->row_base, tmp, tmp_bytes, ctl, gsim::kCompCounters + 4 * plan.size(), component_of,
                                  first_row, sizes, stream, "components"))
        return rc;
    const unsigned long long* h_ctl = labels.ctl.data();
    if (h_ctl[gsim::kCompUnions] != labels.unions) return fail(GSIM_ERR_STATE, "components: the hooks and the component counts do not add up");
    for (uint32_t l = 0; l < nlevels; l++) ncomponents[l] = labels.ncomp[l];
    if (st) {
        st->rows = N;
        st->levels = nlevels;
        st->launches = plan.size();
        st->pairs = N * (N - 1) / 2;
        st->kept = h_ctl[gsim::kCompKept];
        st->unions = labels.unions;
        st->cas_failed = h_ctl[gsim::kCompCasFailed];
        st->kernel_ms = ev_kernel.ms();
        st->label_ms = labels.ev_label.ms();
        st->d2h_ms = labels.ev_d2h.ms();
        clocks.add(h_ctl + gsim::kCompCounters, plan.size()); // (read with the counters, in one copy)
        st->clock_mhz = clocks.mhz();
        st->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_components(gsim_db* db, const float* cutoffs, uint32_t nlevels, int metric, float alpha, float beta, uint32_t* component_of,
                       uint32_t* ncomponents, uint32_t* first_row, uint32_t* sizes, gsim_components_stats* stats)
{
    if (stats) *stats = gsim_components_stats{};
    if (!db || !cutoffs || !component_of || !ncomponents) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nlevels < 1 || nlevels > GSIM_COMPONENTS_MAX_LEVELS) return fail(GSIM_ERR_INVALID, "components: between 1 and 8 cutoff levels");
    for (uint32_t l = 0; l < nlevels; l++) {
        if (!(cutoffs[l] > 0.0f && cutoffs[l] <= 1.0f)) return fail(GSIM_ERR_INVALID, "components: every cutoff must be in (0, 1]");
        if (l && !(cutoffs[l - 1] < cutoffs[l])) return fail(GSIM_ERR_INVALID, "components: the cutoffs must be strictly ascending");
    }
    if (const int rc = check_symmetric_metric("components need", "components", metric, alpha, beta)) return rc;
    if (const int rc = check_tile_table(db, "components")) return rc;
    const uint64_t N = db->nrows;
    for (uint32_t l = 0; l < nlevels; l++) ncomponents[l] = 0;
    if (N == 0) return GSIM_OK;
    if (const int rc = check_table_state(db, "components", true)) return rc;
    return on_one_shard(db, "host memory for components", [&](Shard& s) {
        return components(db, s, cutoffs, nlevels, metric, alpha, beta, component_of, ncomponents, first_row, sizes, stats);
    });
}

int gsim_components(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, uint32_t* component_of, uint32_t* first_row,
                    uint32_t* sizes, uint64_t* ncomponents)
{
    if (!indptr || !ncomponents || (nrows && !component_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    uint64_t nnz = 0;
    if (const int rc = check_csr_offsets(indptr, nrows, &nnz)) return rc;
    if (const int rc = check_csr_indices(indices, nnz, nrows)) return rc;
    try {
        Forest f(nrows);
        for (uint64_t r = 0; r < nrows; r++)
            for (uint64_t e = indptr[r]; e < indptr[r + 1]; e++) f.unite(static_cast<uint32_t>(r), indices[e]);
        *ncomponents = number_components(f, nrows, component_of, first_row, sizes);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "components");
    }
    return GSIM_OK;
}

} // extern "C"
