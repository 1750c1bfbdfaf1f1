// knn_join_plan_check.cpp -- plan_knn_join (capi_knn_join.cpp, a pure host function) over a grid of left sizes, table sizes,
// row widths, device sizes and knob values: a stand-alone program, built and run by tests/test_knn_join_host.py.  It replays each
// plan the way the fold kernel reads it (gsim::knn_join_seg_begin, a launch's rows [r0, r1) of every segment) and checks that
//   * the segment cuts start at 0, end at N, are multiples of 256 and ascend strictly (no segment is empty, segment 0 is the longest);
//   * every (owner tile, segment) gets its segment's columns exactly once, in ascending order, launch after launch;
//   * S is 1 when the owner tiles give two workgroups per CU, else ceil(2 x CUs / owner tiles); a forced S is taken; either is
//     clamped to the table's column tiles and to kKnnJoinMaxSegments;
//   * under the automatic rule the partial lists stay below 2 x (2 x CUs) x 256 x k x 8 bytes;
//   * no launch walks more columns than gsim_db_knn's per-lane bound, a launch prices within the tile budget (or is one column
//     tile per segment), a pair budget is kept (or the launch is one column tile per segment);
//   * with S == 1 the launches are plan_knn's;
//   * plan_knn, which is plan_knn_join with one segment, gives launch for launch what its own loop gave before the two were one
//     (restated here as plan_knn_before).
#include "../../gpusimilarity_amd/csrc/capi_pairs.h"

#include <cstdio>

using namespace gsim_host;

namespace
{

int failures = 0;
#define CHECK(cond)                                                                                                                  \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            if (failures < 40)                                                                                                       \
                std::fprintf(stderr, "%s:%d: %s  [nl %llu N %llu WP %u cus %d segments %d pairs %lld]\n", __FILE__, __LINE__, #cond, \
                             (unsigned long long) g_nl, (unsigned long long) g_N, g_WP, g_cus, g_seg, g_pairs);                      \
            failures++;                                                                                                              \
        }                                                                                                                            \
    } while (0)

uint64_t g_nl, g_N;
uint32_t g_WP;
int g_cus, g_seg;
long long g_pairs;

// gsim_db_knn's plan as it was written out before it became plan_knn_join with one segment: the oracle of plan_knn
std::vector<KnnLaunch> plan_knn_before(uint64_t nout, uint64_t N, uint32_t WP, long long pairs)
{
    const uint64_t tile = gsim::kKnnTile, ctile = gsim::kKnnColTile;
    const uint64_t not_total = (nout + tile - 1) / tile;
    const uint64_t max_tiles = launch_tile_budget(WP);
    const uint64_t group = std::min<uint64_t>(std::min(not_total, max_tiles), 1u << 30);
    std::vector<KnnLaunch> out;
    for (uint64_t t0 = 0; t0 < not_total; t0 += group) {
        const uint64_t nt = std::min(group, not_total - t0);
        uint64_t cols;
        if (pairs > 0) {
            const uint64_t owners = std::min(nt * tile, nout - t0 * tile);
            cols = static_cast<uint64_t>(pairs) / owners / ctile * ctile;
        } else {
            cols = std::min(max_tiles / nt * ctile, max_tiles / ctile * ctile);
        }
        cols = std::max(cols, ctile);
        for (uint64_t c0 = 0; c0 < N; c0 += cols)
            out.push_back({static_cast<uint32_t>(t0), static_cast<uint32_t>(nt), c0, std::min(c0 + cols, N)});
    }
    return out;
}

void check_one(uint64_t nl, uint64_t N, uint32_t WP, int cus, int segments, long long pairs)
{
    g_nl = nl, g_N = N, g_WP = WP, g_cus = cus, g_seg = segments, g_pairs = pairs;
    const uint64_t tile = gsim::kKnnTile, ctile = gsim::kKnnColTile;
    const uint64_t ot = (nl + tile - 1) / tile, nct = (N + ctile - 1) / ctile;
    const KnnJoinPlan plan = plan_knn_join(nl, N, WP, cus, segments, pairs);
    const uint64_t S = plan.segments;

    // S: the rule and the clamp
    uint64_t want = segments > 0 ? static_cast<uint64_t>(segments) : ot >= 2u * static_cast<uint64_t>(cus) ? 1 : (2u * cus + ot - 1) / ot;
    want = std::max<uint64_t>(std::min(std::min(want, nct), static_cast<uint64_t>(gsim::kKnnJoinMaxSegments)), 1);
    CHECK(S == want);
    if (segments == 0) {
        CHECK(S * ot >= std::min<uint64_t>(2u * cus, ot * nct)); // two workgroups per CU, where the table has the tiles for it
        CHECK(static_cast<double>(nl) * S * 128 * 8 < 2.0 * (2.0 * cus) * 256 * 128 * 8 || S == 1);
    }

    // the cuts
    CHECK(gsim::knn_join_seg_begin(0, S, N) == 0 && gsim::knn_join_seg_begin(S, S, N) == N);
    uint64_t longest = 0;
    for (uint64_t s = 0; s < S; s++) {
        const uint64_t b = gsim::knn_join_seg_begin(s, S, N), e = gsim::knn_join_seg_begin(s + 1, S, N);
        CHECK(b % ctile == 0 && (e % ctile == 0 || e == N) && b < e);
        longest = std::max(longest, e - b);
    }
    CHECK(longest == gsim::knn_join_seg_begin(1, S, N));

    // the launches, replayed
    const uint64_t max_tiles = launch_tile_budget(WP);
    const uint64_t lane_cols = std::max(max_tiles / ctile * ctile, ctile);
    std::vector<uint64_t> done(ot * S, 0); // columns of segment s folded so far by owner tile t
    uint32_t last_ot0 = 0;
    uint64_t last_r1 = 0;
    for (const KnnJoinLaunch& l : plan.launches) {
        CHECK(l.not_ >= 1 && static_cast<uint64_t>(l.ot0) + l.not_ <= ot && l.r0 < l.r1 && l.r0 % ctile == 0 && l.r1 <= longest);
        CHECK(l.r1 % ctile == 0 || l.r1 == longest);
        const uint64_t cols = l.r1 - l.r0;
        const uint64_t owners = std::min<uint64_t>(l.not_ * tile, nl - l.ot0 * tile);
        if (pairs > 0) CHECK(owners * S * cols <= static_cast<uint64_t>(pairs) || cols <= ctile);
        else {
            CHECK(cols <= lane_cols);
            CHECK(l.not_ * S * ((cols + ctile - 1) / ctile) <= max_tiles || cols <= ctile);
        }
        // the pieces of a group of owner tiles follow each other in ascending order; groups ascend
        if (l.ot0 == last_ot0 && &l != &plan.launches.front()) CHECK(l.r0 == last_r1);
        else CHECK(l.r0 == 0 && (l.ot0 > last_ot0 || &l == &plan.launches.front()));
        last_ot0 = l.ot0, last_r1 = l.r1;
        for (uint64_t t = l.ot0; t < static_cast<uint64_t>(l.ot0) + l.not_ && t < ot; t++)
            for (uint64_t s = 0; s < S; s++) {
                const uint64_t b = gsim::knn_join_seg_begin(s, S, N), e = gsim::knn_join_seg_begin(s + 1, S, N);
                const uint64_t c0 = b + l.r0, c1 = e - b < l.r1 ? e : b + l.r1; // (the kernel's lines)
                if (c0 >= c1) continue;
                CHECK(done[t * S + s] == l.r0); // exactly once, in ascending order
                done[t * S + s] = c1 - b;
            }
    }
    for (uint64_t t = 0; t < ot; t++)
        for (uint64_t s = 0; s < S; s++) CHECK(done[t * S + s] == gsim::knn_join_seg_begin(s + 1, S, N) - gsim::knn_join_seg_begin(s, S, N));

    const std::vector<KnnLaunch> ref = plan_knn(nl, N, WP, pairs), before = plan_knn_before(nl, N, WP, pairs);
    CHECK(ref.size() == before.size()); // (whatever this call's S, CUs and `segments` are)
    for (size_t i = 0; i < ref.size() && i < before.size(); i++)
        CHECK(ref[i].ot0 == before[i].ot0 && ref[i].not_ == before[i].not_ && ref[i].c0 == before[i].c0 && ref[i].c1 == before[i].c1);
    if (S == 1) {
        CHECK(ref.size() == plan.launches.size());
        for (size_t i = 0; i < ref.size() && i < plan.launches.size(); i++)
            CHECK(ref[i].ot0 == plan.launches[i].ot0 && ref[i].not_ == plan.launches[i].not_ && ref[i].c0 == plan.launches[i].r0 &&
                  ref[i].c1 == plan.launches[i].r1);
    }
}

} // namespace

int main()
{
    const uint64_t nls[] = {1, 63, 64, 65, 255, 256, 257, 300, 512, 1000, 4096, 70000, 131072, 140000};
    const uint64_t Ns[] = {1, 40, 255, 256, 257, 1200, 1280, 4097, 100000, 1000000};
    const uint32_t WPs[] = {4, 8, 32, 128};
    const int cuss[] = {1, 64, 256, 304};
    const int segs[] = {0, 1, 2, 3, 5, 99, 512, 70000};
    const long long pairss[] = {0, 1, 300 * 256, 1200 * 512, 1ll << 24, 1ll << 40};
    unsigned long long n = 0;
    for (uint64_t nl : nls)
        for (uint64_t N : Ns)
            for (uint32_t WP : WPs)
                for (int cus : cuss)
                    for (int seg : segs)
                        for (long long pairs : pairss) {
                            // (replaying costs owner tiles x segments x launches: the largest left sizes only at the extremes of the knobs)
                            if (nl > 4096 && ((seg != 0 && seg != 1 && seg != 5) || (pairs != 0 && pairs != 1ll << 40) || (WP != 32 && WP != 128))) continue;
                            if (pairs == 1 && static_cast<uint64_t>(seg) > 99 && N > 100000) continue;
                            check_one(nl, N, WP, cus, seg, pairs);
                            n++;
                        }
    if (failures) {
        std::printf("knn_join_plan_check: %d failures in %llu plans\n", failures, n);
        return 1;
    }
    std::printf("ok %llu plans\n", n);
    return 0;
}
