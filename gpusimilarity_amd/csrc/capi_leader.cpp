// capi_leader.cpp -- gsim_db_leader: leader (sphere-exclusion) clustering in rounds of candidates.  The argument checks and the
// launch sequence of a call; the device side is gsim_leader.hip (resolve, pass, compaction).  The rule is stated in
// include/gpusim_hip.h.
#include "capi_front.h"

#include <cmath>

namespace gsim_host
{
namespace
{

// Row x leader pairs of one launch of a pass where GSIM_LEADER_LAUNCH_PAIRS is not set: the group scan's arithmetic (capi_group.cpp
// group_launch_pairs) -- the leader loop is that scan's loop, and the early exits only shorten it.
constexpr uint64_t kLeaderLaunchWork = 45000000000ull;
constexpr uint64_t kLeaderPairOverhead = 14;
constexpr uint64_t kLeaderWordLoopCost = 20;
// A pass whose rows take more than this many bytes reads them with non-temporal loads: they do not fit the Infinity Cache, and
// the next round's pass would not find them there
constexpr uint64_t kLeaderCachedBytes = 192ull << 20;

uint64_t leader_launch_pairs(const gsim_db* db, uint32_t W, bool word_loop)
{
    if (db->knobs.leader_launch_pairs > 0) return static_cast<uint64_t>(db->knobs.leader_launch_pairs);
    return kLeaderLaunchWork / (W + kLeaderPairOverhead) / (word_loop ? kLeaderWordLoopCost : 1u);
}

int leader(gsim_db* db, Shard& s, float cutoff, const uint32_t* seeds, uint32_t nseeds, uint32_t max_leaders, int metric, float alpha, float beta,
           uint32_t* leaders, uint32_t* nleaders, uint32_t* leader_of, float* row_score, gsim_leader_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t N = s.nrows;
    GSIM_HIP(set_device(s.device));
    const hipStream_t stream = s.stream;
    const uint32_t B = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(db->knobs.leader_round), N));
    const uint32_t cover_words = (B + 63u) / 64u;

    size_t tmp_bytes = 0;
    GSIM_HIP(gsim::leader_select_bytes(N, &tmp_bytes));
    DevBuf<uint32_t> d_leader_of, d_list[2], d_leaders, d_round_fp, d_round_pop, d_ctl;
    DevBuf<float> d_row_score;
    DevBuf<unsigned long long> d_cover;
    DevBuf<> d_tmp;
    GSIM_ALLOC(d_leader_of, N * 4, "leader clustering (leader_of)");
    GSIM_ALLOC(d_list[0], N * 4, "leader clustering (the active list)");
    GSIM_ALLOC(d_list[1], N * 4, "leader clustering (the active list)");
    if (row_score) GSIM_ALLOC(d_row_score, N * 4, "leader clustering (row_score)");
    GSIM_ALLOC(d_leaders, static_cast<size_t>(max_leaders) * 4, "leader clustering (leaders)");
    GSIM_ALLOC(d_round_fp, static_cast<size_t>(B) * s.W * 4, "leader clustering (the round buffer)");
    GSIM_ALLOC(d_round_pop, static_cast<size_t>(B) * 4, "leader clustering (the round buffer)");
    GSIM_ALLOC(d_cover, static_cast<size_t>(B) * cover_words * 8, "leader clustering (the resolve)");
    GSIM_ALLOC(d_ctl, gsim::kLdrCtlWords * 4, "leader clustering (control block)");
    GSIM_ALLOC(d_tmp, tmp_bytes, "leader clustering (compaction scratch)");
    HostBuf<uint32_t> h_ctl(hipHostMallocDefault); // the control block as every round left it
    GSIM_HIP(h_ctl.grow(gsim::kLdrCtlWords * 4));

    gsim::LeaderArgs a{};
    a.rows = s.d_rows;
    a.W = s.W;
    a.metric = metric;
    a.alpha = alpha;
    a.beta = beta;
    a.cutoff = cutoff;
    a.leaders = d_leaders;
    a.leader_of = d_leader_of;
    a.row_score = d_row_score;
    a.round_fp = d_round_fp;
    a.round_pop = d_round_pop;
    a.cover = d_cover;
    a.ctl = d_ctl;
    a.max_leaders = max_leaders;

    // initial state: nobody has a leader but the seeds; the list holds every other row
    std::vector<uint32_t> ctl0(gsim::kLdrCtlWords, 0u);
    ctl0[gsim::kLdrAssigned] = nseeds;
    std::vector<uint32_t> seed_rows(nseeds);
    for (uint32_t j = 0; j < nseeds; j++) seed_rows[j] = seeds[j] - db->row_base;
    GSIM_HIP(hipMemsetD32Async(static_cast<hipDeviceptr_t>(d_leader_of), static_cast<int>(GSIM_LEADER_NONE), N, stream));
    if (row_score) GSIM_HIP(hipMemsetD32Async(static_cast<hipDeviceptr_t>(d_row_score), 0, N, stream));
    GSIM_HIP(hipMemcpyAsync(d_ctl, ctl0.data(), ctl0.size() * 4, hipMemcpyHostToDevice, stream));
    if (nseeds) GSIM_HIP(hipMemcpyAsync(d_leaders, seed_rows.data(), static_cast<size_t>(nseeds) * 4, hipMemcpyHostToDevice, stream));
    uint64_t launches = 0, rounds = 0;
    GSIM_HIP(gsim::launch_leader_first_list(a, d_tmp, tmp_bytes, N, nseeds, d_list[0], stream));
    launches += nseeds ? 2 : 1;
    GSIM_HIP(hipMemcpyAsync(h_ctl, d_ctl, gsim::kLdrCtlWords * 4, hipMemcpyDeviceToHost, stream));
    GSIM_HIP(hipStreamSynchronize(stream));
    uint64_t nactive = h_ctl[gsim::kLdrActive];
    if (nactive != N - nseeds) return fail(GSIM_ERR_STATE, "leader: the device reported an impossible list length");

    Event ev[4];
    if (st)
        for (auto& e : ev) GSIM_HIP(e.create());
    double kernel_ms = 0.0, resolve_ms = 0.0, compact_ms = 0.0;
    const bool specialised = s.W == 4 || s.W == 8 || s.W == 16 || s.W == 32 || s.W == 64; // (launch_leader_pass's switch)
    const uint64_t pairs_per_launch = leader_launch_pairs(db, s.W, !specialised);
    const uint64_t chunk_rows = gsim::leader_chunk_rows(s.W);
    const uint64_t row_bytes = static_cast<uint64_t>(s.W) * 4u;
    uint32_t made = 0, seeded = 0;
    int cur = 0;
    // One round: its leaders (seeds as they are, or the resolve of the first B entries), the pass over the rest of the list cut into
    // launches, the compaction into the other buffer, and ONE look at the control block.
    while (seeded < nseeds || (nactive > 0 && made < max_leaders)) {
        const bool seed_round = seeded < nseeds;
        const uint32_t nc = seed_round ? std::min(B, nseeds - seeded) : static_cast<uint32_t>(std::min<uint64_t>(B, nactive));
        const uint64_t first = seed_round ? 0 : nc; // candidates leave the list with the round
        if (st) GSIM_HIP(hipEventRecord(ev[0], stream));
        if (seed_round) {
            GSIM_HIP(gsim::launch_leader_seed_round(a, seeded, nc, stream));
            launches += 1;
        } else {
            GSIM_HIP(gsim::launch_leader_resolve(a, d_list[cur], nc, stream));
            launches += 2;
        }
        if (st) GSIM_HIP(hipEventRecord(ev[1], stream));
        if (nactive > first) {
            // (the round's leaders are at most nc: the host sizes the launches without knowing how many the resolve made)
            const uint64_t per = std::max<uint64_t>(pairs_per_launch / nc / chunk_rows, 1u) * chunk_rows;
            const bool nt = (nactive - first) * row_bytes > kLeaderCachedBytes;
            for (uint64_t e0 = first; e0 < nactive; e0 += per) {
                GSIM_HIP(gsim::launch_leader_pass(a, d_list[cur], e0, std::min(e0 + per, nactive), s.num_cus, nt, stream));
                launches++;
            }
            if (st) GSIM_HIP(hipEventRecord(ev[2], stream));
            GSIM_HIP(gsim::launch_leader_compact(a, d_tmp, tmp_bytes, d_list[cur] + first, nactive - first, d_list[cur ^ 1], stream));
            launches++;
        } else if (st) {
            GSIM_HIP(hipEventRecord(ev[2], stream));
        }
        if (st) GSIM_HIP(hipEventRecord(ev[3], stream));
        GSIM_HIP(hipMemcpyAsync(h_ctl, d_ctl, gsim::kLdrCtlWords * 4, hipMemcpyDeviceToHost, stream));
        GSIM_HIP(hipStreamSynchronize(stream));
        const uint64_t left = nactive > first ? h_ctl[gsim::kLdrActive] : 0u;
        const uint32_t now = h_ctl[gsim::kLdrLeaders];
        if (left > nactive - first || now > max_leaders || now < made || (!seed_round && now == made))
            return fail(GSIM_ERR_STATE, "leader: the device reported an impossible round");
        if (nactive > first) cur ^= 1;
        nactive = left;
        made = now;
        if (seed_round) seeded += nc;
        rounds++;
        if (st) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[0], ev[3]) == hipSuccess) kernel_ms += ms;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) resolve_ms += ms;
            if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) compact_ms += ms;
        }
    }

    EventPair ev_d2h;
    if (st) {
        GSIM_HIP(ev_d2h.create());
        GSIM_HIP(hipEventRecord(ev_d2h.a, stream));
    }
    GSIM_HIP(hipMemcpyAsync(leaders, d_leaders, static_cast<size_t>(made) * 4, hipMemcpyDeviceToHost, stream));
    if (leader_of) GSIM_HIP(hipMemcpyAsync(leader_of, d_leader_of, N * 4, hipMemcpyDeviceToHost, stream));
    if (row_score) GSIM_HIP(hipMemcpyAsync(row_score, d_row_score, N * 4, hipMemcpyDeviceToHost, stream));
    if (st) GSIM_HIP(hipEventRecord(ev_d2h.b, stream));
    GSIM_HIP(hipStreamSynchronize(stream));
    for (uint32_t j = 0; j < made; j++) leaders[j] += db->row_base;
    *nleaders = made;
    if (st) {
        st->leaders = made;
        st->rounds = rounds;
        st->launches = launches;
        std::memcpy(&st->pairs, h_ctl + gsim::kLdrPairs, 8);
        std::memcpy(&st->assigned, h_ctl + gsim::kLdrAssigned, 8);
        st->kernel_ms = kernel_ms;
        st->resolve_ms = resolve_ms;
        st->compact_ms = compact_ms;
        st->d2h_ms = ev_d2h.ms();
        st->wall_ms = ms_since(t0);
    }
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_leader(gsim_db* db, float cutoff, const uint32_t* seeds, uint32_t nseeds, uint32_t max_leaders, int metric, float alpha, float beta,
                   uint32_t* leaders, uint32_t* nleaders, uint32_t* leader_of, float* row_score, gsim_leader_stats* stats)
{
    if (stats) *stats = gsim_leader_stats{};
    if (!db || !leaders || !nleaders) return fail(GSIM_ERR_INVALID, "NULL argument");
    *nleaders = 0;
    if (const int rc = check_cutoff("leader", cutoff)) return rc;
    if (const int rc = check_symmetric_metric("leader needs", "leader", metric, alpha, beta)) return rc;
    const uint64_t N = db->nrows;
    if (N > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "leader: tables of 2^32 rows or more");
    if (db->fp_bits > 4096) return fail(GSIM_ERR_INVALID, "leader: rows wider than 4096 bits");
    if (N == 0 && nseeds == 0) return GSIM_OK;
    if (max_leaders < 1 || max_leaders < nseeds || max_leaders > N)
        return fail(GSIM_ERR_INVALID, "leader: max_leaders must be at least 1, at least the number of seeds and at most the number of rows");
    if (const int rc = check_seeds(db, seeds, nseeds, "leader seeds")) return rc;
    if (const int rc = check_table_state(db, "leader clustering", false)) return rc;
    return on_one_shard(db, "host memory for leader clustering", [&](Shard& s) {
        return leader(db, s, cutoff, seeds, nseeds, max_leaders, metric, alpha, beta, leaders, nleaders, leader_of, row_score, stats);
    });
}

} // extern "C"
