// capi_profile.cpp -- the column-wise questions about a table: gsim_db_bit_counts (per-bit column counts of a row range or a row
// set), gsim_db_overlap_sums (every row's weighted popcount) and their host companions gsim_isim / gsim_isim_complement (the iSIM
// index of a set from its column counts, and of the set without each row).  The argument checks, the launch cuts and the copies of a
// call; the device side is gsim_profile.hip.  The rules are stated in include/gpusim_hip.h.
#include "capi_front.h"

namespace gsim_host
{
namespace
{

// Bytes of table rows one launch of either pass reads at most (GSIM_PROFILE_LAUNCH_ROWS = 0): as a histogram's streaming pass
constexpr uint64_t kProfileLaunchBytes = (256ull << 20) * 128ull;

uint64_t launch_rows(const gsim_db* db, uint32_t W)
{
    const uint64_t knob = static_cast<uint64_t>(db->knobs.profile_launch_rows);
    return std::max<uint64_t>(knob > 0 ? knob : kProfileLaunchBytes / (static_cast<uint64_t>(W) * 4u), 1);
}

// what both device calls check after their own arguments, in this order
int check_profile_handle(const gsim_db* db, uint64_t row_begin, uint64_t row_end)
{
    if (const int rc = check_row_range(db, row_begin, row_end)) return rc;
    if (db->nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "column counts: tables of 2^32 rows or more");
    if (db->fp_bits > 4096) return fail(GSIM_ERR_INVALID, "column counts support rows of up to 4096 bits");
    return GSIM_OK;
}

int check_profile_state(const gsim_db* db)
{
    return db->nrows == 0 ? GSIM_OK : check_table_state(db, "column counts", true); // (an empty table has nothing to read: zeros)
}

int bit_counts(gsim_db* db, Shard& s, const gsim_rowset* rs, uint64_t rb, uint64_t re, uint64_t* counts, uint64_t* counted, gsim_profile_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t F = db->fp_bits;
    gsim_profile_stats ps{};
    std::vector<unsigned long long> h(static_cast<size_t>(F) + 1, 0); // the counters, then the rows counted
    if (rb < re && !(rs && rs->count == 0)) {
        GSIM_HIP(set_device(s.device));
        const hipStream_t stream = s.stream;
        DevBuf<unsigned long long> d_counts;
        DevBuf<uint32_t> d_range, d_partial;
        GSIM_ALLOC(d_counts, h.size() * 8, "the column counters");
        GSIM_ALLOC(d_partial, static_cast<size_t>(gsim::profile_count_blocks(s.num_cus)) * h.size() * 4, "the column counters (the workgroups' partials)");
        GSIM_HIP(hipMemsetAsync(d_counts, 0, h.size() * 8, stream));
        const bool gather = rs && subset_gather_applies(db, s, rs->count);
        uint64_t i0 = rb, i1 = re;
        if (gather) { // the entries of the set's list inside the range
            uint32_t range[2] = {0, 0};
            GSIM_ALLOC(d_range, sizeof range, "the row set's range");
            GSIM_HIP(gsim::launch_profile_list_range(rs->d_list, static_cast<uint32_t>(rs->count), rb, re, d_range, stream));
            GSIM_HIP(hipMemcpyAsync(range, d_range, sizeof range, hipMemcpyDeviceToHost, stream));
            GSIM_HIP(hipStreamSynchronize(stream));
            i0 = range[0];
            i1 = range[1];
        }
        gsim::ProfileCountArgs a{};
        a.rows = static_cast<const uint32_t*>(s.d_rows);
        a.W = s.W;
        a.bits = rs && !gather ? rs->d_bits.as<uint32_t>() : nullptr;
        a.list = gather ? rs->d_list.as<uint32_t>() : nullptr;
        a.counts = d_counts;
        a.partial = d_partial;
        EventPair ev_run, ev_d2h;
        GSIM_HIP(ev_run.create());
        GSIM_HIP(ev_d2h.create());
        const uint64_t per = launch_rows(db, s.W);
        GSIM_HIP(hipEventRecord(ev_run.a, stream));
        for (uint64_t i = i0; i < i1; i += per) {
            GSIM_HIP(gsim::launch_profile_count(a, i, std::min(i + per, i1), s.num_cus, stream));
            ps.launches++;
        }
        GSIM_HIP(hipEventRecord(ev_run.b, stream));
        GSIM_HIP(hipEventRecord(ev_d2h.a, stream));
        GSIM_HIP(hipMemcpyAsync(h.data(), d_counts, h.size() * 8, hipMemcpyDeviceToHost, stream));
        GSIM_HIP(hipEventRecord(ev_d2h.b, stream));
        GSIM_HIP(hipStreamSynchronize(stream)); // (the temporaries are freed on return)
        ps.rows_read = i1 - i0;
        ps.route = gather ? GSIM_PROFILE_GATHERED : GSIM_PROFILE_STREAMED;
        ps.kernel_ms = ev_run.ms();
        ps.d2h_ms = ev_d2h.ms();
    }
    for (uint32_t k = 0; k < F; k++) counts[k] = h[k];
    if (counted) *counted = h[F];
    ps.rows_counted = h[F];
    ps.wall_ms = ms_since(t0);
    if (st) *st = ps;
    return GSIM_OK;
}

int overlap_sums(gsim_db* db, Shard& s, const uint32_t* weights, uint64_t rb, uint64_t re, uint64_t* sums, uint32_t* popc, gsim_profile_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    gsim_profile_stats ps{};
    const uint64_t n = re - rb;
    if (n > 0) {
        const uint32_t W = s.W, F = db->fp_bits;
        // the weights as bit planes: plane b is the fingerprint of the columns whose weight has bit b set
        std::vector<uint32_t> planes(static_cast<size_t>(32) * W, 0);
        uint32_t all = 0;
        for (uint32_t k = 0; k < F; k++) {
            all |= weights[k];
            for (uint32_t w = weights[k], b = 0; w; w >>= 1, b++)
                if (w & 1u) planes[static_cast<size_t>(b) * W + k / 32] |= 1u << (k % 32);
        }
        uint32_t nplanes = 1;
        while (nplanes < 32 && (all >> nplanes)) nplanes++;
        GSIM_HIP(set_device(s.device));
        const hipStream_t stream = s.stream;
        DevBuf<uint32_t> d_planes, d_popc;
        DevBuf<unsigned long long> d_sums;
        GSIM_ALLOC(d_planes, planes.size() * 4, "the weights' bit planes");
        GSIM_ALLOC(d_sums, n * 8, "the overlap sums");
        if (popc) GSIM_ALLOC(d_popc, n * 4, "the overlap sums (popcounts)");
        GSIM_HIP(hipMemcpyAsync(d_planes, planes.data(), planes.size() * 4, hipMemcpyHostToDevice, stream));
        bool matrix = gsim::profile_overlap_matrix(W);
#ifdef GSIM_TEST_HOOKS
        if (env_int("GSIM_TEST_PROFILE_VALU", 0)) matrix = false; // (the VALU kernel at the matrix kernel's widths: tests, and the crossover's timing)
#endif
        gsim::ProfileOverlapArgs a{};
        a.rows = static_cast<const uint32_t*>(s.d_rows);
        a.W = W;
        a.planes = d_planes;
        a.nplanes = nplanes;
        a.sums = d_sums;
        a.popc = popc ? d_popc.as<uint32_t>() : nullptr;
        a.out0 = rb;
        EventPair ev_run, ev_d2h;
        GSIM_HIP(ev_run.create());
        GSIM_HIP(ev_d2h.create());
        const uint64_t per = launch_rows(db, W);
        GSIM_HIP(hipEventRecord(ev_run.a, stream));
        for (uint64_t r = rb; r < re; r += per) {
            GSIM_HIP(gsim::launch_profile_overlap(a, r, std::min(r + per, re), matrix, s.num_cus, stream));
            ps.launches++;
        }
        GSIM_HIP(hipEventRecord(ev_run.b, stream));
        GSIM_HIP(hipEventRecord(ev_d2h.a, stream));
        GSIM_HIP(hipMemcpyAsync(sums, d_sums, n * 8, hipMemcpyDeviceToHost, stream));
        if (popc) GSIM_HIP(hipMemcpyAsync(popc, d_popc, n * 4, hipMemcpyDeviceToHost, stream));
        GSIM_HIP(hipEventRecord(ev_d2h.b, stream));
        GSIM_HIP(hipStreamSynchronize(stream)); // (the planes' host copy and the temporaries are freed on return)
        ps.rows_read = ps.rows_counted = n;
        ps.route = GSIM_PROFILE_STREAMED | (matrix ? GSIM_PROFILE_MATRIX : GSIM_PROFILE_VALU);
        ps.kernel_ms = ev_run.ms();
        ps.d2h_ms = ev_d2h.ms();
    }
    ps.wall_ms = ms_since(t0);
    if (st) *st = ps;
    return GSIM_OK;
}

// ---- the host companions ----
typedef unsigned __int128 u128;
typedef __int128 i128;

// one round-to-nearest(-even) conversion: the top 64 bits with a sticky bit (11 bits more than a double keeps), converted by the
// hardware, scaled exactly
double to_double(u128 v)
{
    const uint64_t hi = static_cast<uint64_t>(v >> 64);
    if (hi == 0) return static_cast<double>(static_cast<uint64_t>(v));
    const int sh = 64 - __builtin_clzll(hi);
    uint64_t top = static_cast<uint64_t>(v >> sh);
    if (v & ((static_cast<u128>(1) << sh) - 1)) top |= 1u;
    return std::ldexp(static_cast<double>(top), sh);
}

struct PairSums {
    u128 a = 0, d = 0, dis = 0, c = 0; // pairs of ones, pairs of zeros, mismatches, sum of the counts
};

int pair_sums(const uint64_t* counts, uint32_t fp_bits, uint64_t n, int index, PairSums* out)
{
    if (!counts) return fail(GSIM_ERR_INVALID, "NULL counts");
    if (fp_bits == 0) return fail(GSIM_ERR_INVALID, "isim: fp_bits == 0");
    if (n > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "isim: 2^32 rows or more");
    if (index != GSIM_ISIM_TANIMOTO && index != GSIM_ISIM_RUSSELL_RAO && index != GSIM_ISIM_SIMPLE_MATCHING)
        return fail(GSIM_ERR_INVALID, "isim: unknown index");
    PairSums p;
    for (uint32_t k = 0; k < fp_bits; k++) {
        const uint64_t c = counts[k];
        if (c > n) return fail(GSIM_ERR_INVALID, "isim: a column count above the number of rows");
        const uint64_t z = n - c; // (c, z < 2^32: every product fits 64 bits)
        p.a += c * (c - (c ? 1u : 0u)) / 2;
        p.d += z * (z - (z ? 1u : 0u)) / 2;
        p.dis += c * z;
        p.c += c;
    }
    *out = p;
    return GSIM_OK;
}

double isim_value(int index, u128 a, u128 d, u128 dis)
{
    const u128 num = index == GSIM_ISIM_SIMPLE_MATCHING ? a + d : a;
    const u128 den = index == GSIM_ISIM_TANIMOTO ? a + dis : a + d + dis;
    return den == 0 ? 0.0 : to_double(num) / to_double(den);
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_db_bit_counts(gsim_db* db, const gsim_rowset* rs, uint64_t row_begin, uint64_t row_end, uint64_t* counts, uint64_t* counted,
                       gsim_profile_stats* stats)
{
    if (stats) *stats = gsim_profile_stats{};
    if (counted) *counted = 0;
    if (!db || !counts) return fail(GSIM_ERR_INVALID, "NULL argument");
    int rc = check_profile_handle(db, row_begin, row_end);
    if (rc != GSIM_OK) return rc;
    if (rs && rs->owner != db) return fail(GSIM_ERR_INVALID, "the row set was made for another handle");
    rc = check_profile_state(db);
    if (rc != GSIM_OK) return rc;
    if (rs && rs->nrows != db->nrows) return fail(GSIM_ERR_STATE, "the table changed after the row set was made");
    if (db->nrows == 0) {
        std::fill(counts, counts + db->fp_bits, uint64_t{0});
        return GSIM_OK;
    }
    return on_one_shard(db, "host memory for the column counts",
                        [&](Shard& s) { return bit_counts(db, s, rs, row_begin, row_end, counts, counted, stats); });
}

int gsim_db_overlap_sums(gsim_db* db, const uint32_t* weights, uint64_t row_begin, uint64_t row_end, uint64_t* sums, uint32_t* popc,
                         gsim_profile_stats* stats)
{
    if (stats) *stats = gsim_profile_stats{};
    if (!db || !weights) return fail(GSIM_ERR_INVALID, "NULL argument");
    int rc = check_profile_handle(db, row_begin, row_end);
    if (rc != GSIM_OK) return rc;
    if (row_begin < row_end && !sums) return fail(GSIM_ERR_INVALID, "NULL sums");
    rc = check_profile_state(db);
    if (rc != GSIM_OK) return rc;
    if (db->nrows == 0) return GSIM_OK;
    return on_one_shard(db, "host memory for the overlap sums",
                        [&](Shard& s) { return overlap_sums(db, s, weights, row_begin, row_end, sums, popc, stats); });
}

int gsim_isim(const uint64_t* counts, uint32_t fp_bits, uint64_t n, int index, double* value)
{
    if (!value) return fail(GSIM_ERR_INVALID, "NULL value");
    PairSums p;
    const int rc = pair_sums(counts, fp_bits, n, index, &p);
    if (rc != GSIM_OK) return rc;
    *value = isim_value(index, p.a, p.d, p.dis);
    return GSIM_OK;
}

int gsim_isim_complement(const uint64_t* counts, uint32_t fp_bits, uint64_t n, int index, const uint64_t* sums, const uint32_t* popc,
                         uint64_t m, double* out)
{
    PairSums p;
    const int rc = pair_sums(counts, fp_bits, n, index, &p);
    if (rc != GSIM_OK) return rc;
    if (m == 0) return GSIM_OK;
    if (!sums || !popc || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (n == 0) return fail(GSIM_ERR_INVALID, "isim: the rows of an empty set");
    const i128 a = static_cast<i128>(p.a), d = static_cast<i128>(p.d), dis = static_cast<i128>(p.dis), c = static_cast<i128>(p.c);
    for (uint64_t i = 0; i < m; i++) {
        if (popc[i] > fp_bits) return fail(GSIM_ERR_INVALID, "isim: a popcount above fp_bits");
        const i128 s = static_cast<i128>(sums[i]), pc = popc[i];
        const i128 ai = a - s + pc;
        const i128 disi = dis - static_cast<i128>(n) * pc - c + 2 * s;
        const i128 di = d - (static_cast<i128>(fp_bits) - pc) * static_cast<i128>(n - 1) + (c - s);
        if (ai < 0 || disi < 0 || di < 0) return fail(GSIM_ERR_INVALID, "isim: row " + std::to_string(i) + " is no member of the counted set");
        out[i] = isim_value(index, static_cast<u128>(ai), static_cast<u128>(di), static_cast<u128>(disi));
    }
    return GSIM_OK;
}

} // extern "C"
