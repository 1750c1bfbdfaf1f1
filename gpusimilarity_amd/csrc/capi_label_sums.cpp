// capi_label_sums.cpp -- gsim_db_label_sums: for every labelled row of a range the quantised sum of its scores against its own
// cluster and against the other cluster of the greatest mean.  The argument checks, the plan and the launches of a call; the label
// sort is gsim_db_label_counts' (LabelSort, capi_labels.cpp), the device side is gsim_label_sums.hip, the host functions on the sums
// are capi_label_sums_host.cpp.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 29.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

struct LsumLaunch {
    uint32_t ot0, not_; // owner tiles
    uint64_t c0, c1;    // candidates (sorted positions)
};

// The fold launches over n labelled rows of WP words whose segments start at first[0 .. nlabels].
// An owner tile's SPAN is what its waves walk: every candidate, or with own_only the segments of the labels its owners have.
// Consecutive tiles share a group while the pairs of the group -- each tile's owners x its span -- stay within the budget.  A group
// within the budget is one launch over its span: with own_only and clusters of moderate size that is many tiles at once, each walking
// its own short span.  Where tiles that are each worth a good part of a budget walk the SAME span -- every tile of a full pass, the
// tiles inside one giant cluster -- the group goes on past the budget while it is below `fill` tiles (eight workgroups per compute
// unit: the waves a SIMD holds) and one column tile of it fits, so that a launch fills the device; such a group is cut into column
// pieces of budget / owners candidates (whole column tiles, at least one, and never more than the budget gives one lane of 65 536), in
// ascending order without gaps, and every piece keeps all of its tiles busy.  `pairs` > 0 is the budget instead of the tile kernel's
// (launch_tile_budget: priced by the width).
std::vector<LsumLaunch> plan_label_sums(uint64_t n, const std::vector<uint32_t>& first, uint32_t WP, bool own_only, uint64_t pairs, uint64_t fill)
{
    const uint64_t tile = gsim::kLsumTile, ctile = gsim::kLsumColTile;
    const uint64_t budget = pairs ? pairs : launch_tile_budget(WP) * tile * ctile;
    const uint64_t ntiles = (n + tile - 1) / tile;
    // the label of a sorted position: the last l with first[l] <= p
    auto label_at = [&](uint64_t p) { return static_cast<size_t>(std::upper_bound(first.begin(), first.end(), static_cast<uint32_t>(p)) - first.begin()) - 1; };
    std::vector<LsumLaunch> out;
    uint64_t t0 = 0;
    while (t0 < ntiles) {
        uint64_t nt = 0, owners = 0, work = 0, lo = 0, hi = 0;
        for (uint64_t t = t0; t < ntiles && nt < (1u << 30); t++) {
            const uint64_t o0 = t * tile, o1 = std::min(o0 + tile, n);
            const uint64_t s0 = own_only ? first[label_at(o0)] : 0, s1 = own_only ? first[label_at(o1 - 1) + 1] : n;
            const uint64_t w = (o1 - o0) * (s1 - s0);
            if (nt && work + w > budget && !(nt < fill && s0 == lo && s1 == hi && (owners + o1 - o0) * ctile <= budget)) break;
            if (nt == 0) lo = s0;
            hi = s1;
            owners += o1 - o0;
            work += w;
            nt++;
        }
        uint64_t cols = hi - lo;
        if (work > budget) cols = std::max(std::min(budget / owners, budget / 65536u) / ctile * ctile, ctile);
        for (uint64_t c = lo; c < hi; c += cols) out.push_back({static_cast<uint32_t>(t0), static_cast<uint32_t>(nt), c, std::min(c + cols, hi)});
        t0 += nt;
    }
    return out;
}

struct LsumCall {
    uint64_t rb, n; // the table rows [rb, rb + n), n > 0
    uint32_t nlabels;
    int metric;
    float alpha, beta;
    bool own_only;
    uint64_t launch_pairs;
};

int label_sums(gsim_db* db, Shard& s, const uint32_t* labels, const LsumCall& c, uint64_t* own_q, uint32_t* other_label, uint64_t* other_q, uint32_t* sizes,
               gsim_label_sums_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    gsim_label_sums_stats ss{};
    ss.rows = c.n;
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const uint32_t WP = gsim::nbr_padded_words(s.W);
    auto drain = [&](int rc) { // (nothing of the call is still running when its buffers go)
        (void) hipStreamSynchronize(st);
        return rc;
    };

    // the outputs in row order, as a GSIM_LABEL_NONE row has them; the labels; the sort
    DevBuf<uint32_t> d_labels, d_other;
    DevBuf<unsigned long long> d_own, d_otherq;
    LabelSort sort;
    GSIM_ALLOC(d_labels, c.n * 4, "the label sums (labels)");
    if (const int rc = sort.alloc(c.n, c.nlabels, "the label sums")) return rc;
    GSIM_ALLOC(d_own, c.n * 8, "the label sums (own sums)");
    if (!c.own_only) {
        GSIM_ALLOC(d_other, c.n * 4, "the label sums (other labels)");
        GSIM_ALLOC(d_otherq, c.n * 8, "the label sums (other sums)");
    }
    EventPair ev_sort, ev_gather, ev_fold, ev_d2h;
    GSIM_HIP(ev_sort.create());
    GSIM_HIP(ev_gather.create());
    GSIM_HIP(ev_fold.create());
    GSIM_HIP(ev_d2h.create());

    GSIM_HIP(hipEventRecord(ev_sort.a, st));
    if (const int rc = sort.enqueue(labels, d_labels, c.n, c.nlabels, c.rb, st)) return drain(rc);
    GSIM_HIP(hipMemsetAsync(d_own, 0, c.n * 8, st));
    if (!c.own_only) {
        GSIM_HIP(hipMemsetAsync(d_other, 0xFF, c.n * 4, st));
        GSIM_HIP(hipMemsetAsync(d_otherq, 0, c.n * 8, st));
    }
    GSIM_HIP(hipEventRecord(ev_sort.b, st));
    GSIM_HIP(hipStreamSynchronize(st));
    ss.sort_ms = ev_sort.ms();
    const std::vector<uint32_t>& first = sort.h_first;
    const uint64_t nlab = first[c.nlabels]; // (GSIM_LABEL_NONE sorts behind every label)
    ss.rows_labelled = nlab;
    uint64_t in_cluster = 0;
    for (uint32_t l = 0; l < c.nlabels; l++) {
        const uint64_t nl = first[l + 1] - first[l];
        if (sizes) sizes[l] = static_cast<uint32_t>(nl);
        ss.labels_nonempty += nl ? 1 : 0;
        in_cluster += nl * nl;
    }
    ss.pairs = (c.own_only ? in_cluster : nlab * nlab) - nlab;

    size_t nlaunch = 0;
    if (nlab) {
        // the labelled rows in label order, zero-padded; their popcounts; the carried state
        const std::vector<LsumLaunch> plan =
            plan_label_sums(nlab, first, WP, c.own_only, c.launch_pairs, 8u * static_cast<uint64_t>(std::max(s.num_cus, 1)));
        nlaunch = plan.size();
        DevBuf<uint32_t> sorted;
        DevBuf<gsim::LsumState> state;
        PaddedRows pops;
        LaunchClocks clocks;
        GSIM_ALLOC(sorted, nlab * WP * 4, "the label sums (the sorted rows)");
        if (const int rc = pops.alloc(nlab, WP, WP, "the label sums (popcounts)", "the label sums (popcounts)")) return rc;
        GSIM_ALLOC(state, nlab * sizeof(gsim::LsumState), "the label sums (carried state)");
        if (const int rc = clocks.own(nlaunch, "the label sums (clock stamps)")) return rc;
        GSIM_HIP(hipEventRecord(ev_gather.a, st));
        GSIM_HIP(clocks.zero(nlaunch, st));
        GSIM_HIP(gsim::launch_lsum_gather(static_cast<const uint32_t*>(s.d_rows), s.W, WP, sort.vals2, nlab, sorted, st));
        if (const int rc = pops.prepare(sorted, nlab, st)) return drain(rc);
        GSIM_HIP(gsim::launch_lsum_init(state, nlab, st));
        GSIM_HIP(hipEventRecord(ev_gather.b, st));

        gsim::LsumArgs a{};
        a.rows = sorted;
        a.pop = pops.pop();
        a.keys = sort.keys2;
        a.first = sort.first;
        a.n = nlab;
        a.WP = WP;
        a.metric = c.metric;
        a.alpha = c.alpha;
        a.beta = c.beta;
        a.state = state;
        GSIM_HIP(hipEventRecord(ev_fold.a, st));
        for (size_t l = 0; l < nlaunch; l++) {
            a.clk = clocks.at(l);
            const hipError_t e = gsim::launch_lsum_fold(a, c.own_only, plan[l].ot0, plan[l].not_, plan[l].c0, plan[l].c1, st);
            if (e != hipSuccess) return drain(fail_hip(e, "launch_lsum_fold"));
        }
        GSIM_HIP(hipEventRecord(ev_fold.b, st));

        GSIM_HIP(hipEventRecord(ev_d2h.a, st));
        hipError_t e = gsim::launch_lsum_scatter(state, sort.vals2, nlab, static_cast<uint32_t>(c.rb), d_own, c.own_only ? nullptr : d_other.as<uint32_t>(),
                                                 c.own_only ? nullptr : d_otherq.as<unsigned long long>(), st);
        if (e == hipSuccess) e = clocks.fetch(nlaunch, st);
        if (e != hipSuccess) return drain(fail_hip(e, "launch_lsum_scatter"));
        // (the temporaries of this block are freed below, behind the wait)
        GSIM_HIP(hipMemcpyAsync(own_q, d_own, c.n * 8, hipMemcpyDeviceToHost, st));
        if (!c.own_only) {
            GSIM_HIP(hipMemcpyAsync(other_label, d_other, c.n * 4, hipMemcpyDeviceToHost, st));
            GSIM_HIP(hipMemcpyAsync(other_q, d_otherq, c.n * 8, hipMemcpyDeviceToHost, st));
        }
        GSIM_HIP(hipEventRecord(ev_d2h.b, st));
        const hipError_t w = hipStreamSynchronize(st);
        if (w != hipSuccess) return fail_hip(w, "hipStreamSynchronize");
        clocks.add();
        ss.gather_ms = ev_gather.ms();
        ss.kernel_ms = ev_fold.ms();
        ss.d2h_ms = ev_d2h.ms();
        ss.clock_mhz = clocks.mhz();
    } else { // every row is GSIM_LABEL_NONE
        GSIM_HIP(hipMemcpyAsync(own_q, d_own, c.n * 8, hipMemcpyDeviceToHost, st));
        if (!c.own_only) {
            GSIM_HIP(hipMemcpyAsync(other_label, d_other, c.n * 4, hipMemcpyDeviceToHost, st));
            GSIM_HIP(hipMemcpyAsync(other_q, d_otherq, c.n * 8, hipMemcpyDeviceToHost, st));
        }
        GSIM_HIP(hipStreamSynchronize(st));
    }
    ss.launches = nlaunch;
    ss.wall_ms = ms_since(t0);
    if (stats) *stats = ss;
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_label_sums(gsim_db* db, const uint32_t* labels, uint32_t nlabels, uint64_t row_begin, uint64_t row_end, int metric, float alpha, float beta,
                       uint32_t flags, uint64_t launch_pairs, uint64_t* own_q, uint32_t* other_label, uint64_t* other_q, uint32_t* sizes,
                       gsim_label_sums_stats* stats)
{
    if (!db || !own_q) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (flags & ~GSIM_LABEL_SUMS_OWN_ONLY) return fail(GSIM_ERR_INVALID, "label sums: unknown flag bits");
    const bool own_only = (flags & GSIM_LABEL_SUMS_OWN_ONLY) != 0;
    if (!own_only && (!other_label || !other_q)) return fail(GSIM_ERR_INVALID, "label sums: NULL other_label or other_q without GSIM_LABEL_SUMS_OWN_ONLY");
    if (nlabels == 0) return fail(GSIM_ERR_INVALID, "label sums: nlabels == 0");
    if (const int rc = check_row_range(db, row_begin, row_end)) return rc;
    if (const int rc = check_metric("label sums", metric, alpha, beta)) return rc;
    if (const int rc = check_tile_table(db, "label sums")) return rc; // (width first: the shared order)
    const uint64_t n = row_end - row_begin;
    if (n && !labels) return fail(GSIM_ERR_INVALID, "label sums: NULL labels");
    for (uint64_t i = 0; i < n; i++)
        if (labels[i] >= nlabels && labels[i] != GSIM_LABEL_NONE)
            return fail(GSIM_ERR_INVALID, "label sums: the label of row " + std::to_string(row_begin + i) + " is not below nlabels");
    if (const int rc = check_table_state(db, "label sums", true)) return rc;
    if (stats) *stats = gsim_label_sums_stats{};
    if (n == 0) {
        if (sizes) std::fill(sizes, sizes + nlabels, 0u);
        return GSIM_OK;
    }
    const LsumCall call{row_begin, n, nlabels, metric, alpha, beta, own_only, launch_pairs};
    return on_one_shard(db, "host memory for the label sums",
                        [&](Shard& s) { return label_sums(db, s, labels, call, own_q, other_label, other_q, sizes, stats); });
}

} // extern "C"
