// capi_rowhash.cpp -- row-hash indexes (gsim_rowhash_*): the duplicate groups of a table and the lookup of a fingerprint in it.  The
// index's lifecycle, the argument checks, the launch cuts and the copies of a call; the device side is gsim_rowhash.hip (the table,
// the inserting pass, the finish, the lookup), the row set of the representatives is capi_subset.cpp's.  The hash and the host
// functions are gsim_rowhash_hash.h and capi_rowhash_host.cpp.  The rule is stated in include/gpusim_hip.h; DESIGN.md section 35.
#include "capi_front.h"
#include "gsim_rowhash_hash.h"

namespace gsim_host
{
namespace
{

// Bytes of table rows one inserting launch reads at most: as the column counts' streaming pass
constexpr uint64_t kRowhashLaunchBytes = (256ull << 20) * 128ull;
// left rows of one lookup launch (8 bytes of answer each, staged through the host)
constexpr uint64_t kRowhashFindRows = 1ull << 22;

const char* const kImpossible = "row hash: the device reported an impossible count";

int build_rowhash(gsim_db* db, gsim_rowhash* ix)
{
    const auto t0 = std::chrono::steady_clock::now();
    Shard& s = db->shards[0];
    const uint64_t N = s.nrows;
    ix->owner = db;
    ix->device = s.device;
    ix->nrows = N;
    ix->fp_bits = db->fp_bits;
    ix->row_base = db->row_base;
    ix->nslots = gsim::rowhash_slots(N);
    ix->stats = gsim_rowhash_stats{};
    ix->stats.rows = N;
    ix->stats.slots = ix->nslots;
    if (N == 0) return GSIM_OK;
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const uint64_t nwords = gsim::rowset_words(N);
    ix->bits.assign(static_cast<size_t>(nwords), 0);
    DevBuf<uint32_t> d_bits, d_flag; // (the build's temporaries are freed on return)
    DevBuf<unsigned long long> d_counters;
    GSIM_ALLOC(ix->d_slots, static_cast<size_t>(ix->nslots) * 8, "the row hash's slots");
    GSIM_ALLOC(ix->d_groups, static_cast<size_t>(N) * 8, "the row hash's groups");
    GSIM_ALLOC(d_bits, static_cast<size_t>(nwords) * 4, "the row hash's bitmap");
    GSIM_ALLOC(d_counters, 4 * 8, "the row hash's counters");
    GSIM_ALLOC(d_flag, 4, "the row hash's flag");
    EventPair ev_insert, ev_finish;
    GSIM_HIP(ev_insert.create());
    GSIM_HIP(ev_finish.create());
    GSIM_HIP(hipMemsetAsync(d_counters, 0, 4 * 8, st));
    GSIM_HIP(hipMemsetAsync(d_flag, 0, 4, st));
    GSIM_HIP(gsim::launch_rowhash_init(ix->d_slots, ix->nslots, s.num_cus, st));
    uint64_t launches = 1;
    const uint64_t cut = std::max<uint64_t>(kRowhashLaunchBytes / (static_cast<uint64_t>(s.W) * 4u), 1);
    GSIM_HIP(hipEventRecord(ev_insert.a, st));
    for (uint64_t r0 = 0; r0 < N; r0 += cut, launches++)
        GSIM_HIP(gsim::launch_rowhash_insert(s.d_rows, r0, std::min(N, r0 + cut), s.W, ix->d_slots, ix->nslots, d_flag, ix->d_groups, s.num_cus, st));
    GSIM_HIP(hipEventRecord(ev_insert.b, st));
    GSIM_HIP(hipEventRecord(ev_finish.a, st));
    GSIM_HIP(gsim::launch_rowhash_finish(ix->d_groups, N, ix->d_slots, ix->nslots, d_flag, d_bits, nwords, d_counters, s.num_cus, st));
    launches++;
    GSIM_HIP(hipEventRecord(ev_finish.b, st));
    unsigned long long counters[4] = {0, 0, 0, 0};
    uint32_t flag = 0;
    GSIM_HIP(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipMemcpyAsync(ix->bits.data(), d_bits, static_cast<size_t>(nwords) * 4, hipMemcpyDeviceToHost, st));
    GSIM_HIP(hipStreamSynchronize(st));
    if (flag != 0 || counters[0] < 1 || counters[0] > N || counters[1] > counters[0] || counters[2] < 1 || counters[2] > N || counters[3] != N)
        return fail(GSIM_ERR_STATE, kImpossible);
    ix->stats.groups = counters[0];
    ix->stats.repeated_groups = counters[1];
    ix->stats.largest_group = counters[2];
    ix->stats.launches = launches;
    ix->stats.kernel_ms = ev_insert.ms() + ev_finish.ms();
    ix->stats.wall_ms = ms_since(t0);
    return GSIM_OK;
}

// The answers for the nl left rows at d_left (the table's W words each, on its device), in launches of at most kRowhashFindRows rows.
// `upload`: host rows that go through a device buffer of this call, launch by launch.
int find_rows(Shard& s, const gsim_rowhash* ix, const uint32_t* d_left, const uint32_t* upload, uint64_t nl, uint32_t* row, uint32_t* size)
{
    if (nl == 0) return GSIM_OK;
    if (ix->nrows == 0) { // an empty table holds no row: no launch
        for (uint64_t q = 0; q < nl; q++) {
            row[q] = GSIM_ROW_NONE;
            if (size) size[q] = 0;
        }
        return GSIM_OK;
    }
    GSIM_HIP(set_device(s.device));
    const hipStream_t st = s.stream;
    const uint64_t per = std::min(nl, kRowhashFindRows);
    DevBuf<uint32_t> d_up, d_flag;
    DevBuf<unsigned long long> d_found;
    std::vector<unsigned long long> found(static_cast<size_t>(per));
    if (upload) GSIM_ALLOC(d_up, static_cast<size_t>(per) * s.W * 4, "the row hash's queries");
    GSIM_ALLOC(d_found, static_cast<size_t>(per) * 8, "the row hash's answers");
    GSIM_ALLOC(d_flag, 4, "the row hash's flag");
    GSIM_HIP(hipMemsetAsync(d_flag, 0, 4, st));
    for (uint64_t q0 = 0; q0 < nl; q0 += per) {
        const uint64_t n = std::min(per, nl - q0);
        if (upload) GSIM_HIP(hipMemcpyAsync(d_up, upload + q0 * s.W, static_cast<size_t>(n) * s.W * 4, hipMemcpyHostToDevice, st));
        const uint32_t* left = upload ? d_up.as<uint32_t>() : d_left + q0 * s.W;
        GSIM_HIP(gsim::launch_rowhash_find(left, n, s.d_rows, s.W, ix->d_slots, ix->nslots, d_flag, d_found, s.num_cus, st));
        uint32_t flag = 0;
        GSIM_HIP(hipMemcpyAsync(found.data(), d_found, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
        GSIM_HIP(hipStreamSynchronize(st));
        if (flag != 0) return fail(GSIM_ERR_STATE, kImpossible);
        for (uint64_t q = 0; q < n; q++) {
            const uint32_t r = static_cast<uint32_t>(found[q]);
            if (r != GSIM_ROW_NONE && r >= ix->nrows) return fail(GSIM_ERR_STATE, kImpossible);
            row[q0 + q] = r == GSIM_ROW_NONE ? GSIM_ROW_NONE : r + ix->row_base;
            if (size) size[q0 + q] = static_cast<uint32_t>(found[q] >> 32);
        }
    }
    return GSIM_OK;
}

// what every call on an index and its handle checks after its own arguments, in this order
int check_index_state(const gsim_rowhash* ix)
{
    if (const int rc = check_table_state(ix->owner, "row hashes", true)) return rc;
    if (ix->nrows != ix->owner->nrows || ix->row_base != ix->owner->row_base) return fail(GSIM_ERR_STATE, "the table changed after the row hash was made");
    return GSIM_OK;
}

} // namespace
} // namespace gsim_host

using namespace gsim_host;

extern "C" {

int gsim_rowhash_create(gsim_db* db, uint32_t flags, gsim_rowhash** out)
{
    if (out) *out = nullptr;
    if (!db || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (flags != 0) return fail(GSIM_ERR_INVALID, "unknown row-hash flags");
    if (db->nrows + db->row_base > GSIM_ROW_NONE) return fail(GSIM_ERR_INVALID, "row hashes: the table's last row number would be GSIM_ROW_NONE or beyond");
    if (const int rc = check_table_state(db, "row hashes", true)) return rc;
    return on_one_shard(db, "host memory for a row hash", [&](Shard&) {
        std::unique_ptr<gsim_rowhash> ix(new (std::nothrow) gsim_rowhash);
        if (!ix) return fail(GSIM_ERR_NOMEM, "row hash");
        const int rc = build_rowhash(db, ix.get());
        if (rc == GSIM_OK) *out = ix.release();
        return rc;
    });
}

int gsim_rowhash_get_stats(const gsim_rowhash* ix, gsim_rowhash_stats* out)
{
    if (!ix || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    *out = ix->stats;
    return GSIM_OK;
}

int gsim_rowhash_groups(const gsim_rowhash* ix, uint32_t* first, uint32_t* size)
{
    if (!ix) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (!first && !size) return fail(GSIM_ERR_INVALID, "row hash: both first and size are NULL");
    if (ix->nrows == 0) return GSIM_OK;
    try {
        std::vector<unsigned long long> g(static_cast<size_t>(ix->nrows));
        GSIM_HIP(set_device(ix->device));
        GSIM_HIP(hipMemcpy(g.data(), ix->d_groups, g.size() * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < ix->nrows; i++) {
            if (first) first[i] = static_cast<uint32_t>(g[i]) + ix->row_base;
            if (size) size[i] = static_cast<uint32_t>(g[i] >> 32);
        }
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "host memory for the row hash's groups");
    }
    return GSIM_OK;
}

int gsim_rowhash_rowset(const gsim_rowhash* ix, uint32_t flags, gsim_rowset** out)
{
    if (out) *out = nullptr;
    if (!ix || !out) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (flags & ~GSIM_ROWHASH_REPEATS) return fail(GSIM_ERR_INVALID, "unknown row-hash flags");
    if (const int rc = check_index_state(ix)) return rc;
    const uint32_t none = 0; // (an empty table's bitmap has no words)
    return gsim_rowset_from_bitmap(ix->owner, ix->bits.empty() ? &none : ix->bits.data(), (flags & GSIM_ROWHASH_REPEATS) ? GSIM_ROWSET_EXCLUDE : 0u, out);
}

int gsim_rowhash_find(const gsim_rowhash* ix, const uint32_t* queries, uint64_t nq, uint32_t* row, uint32_t* size)
{
    if (!ix || (nq && !row)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (nq && !queries) return fail(GSIM_ERR_INVALID, "NULL queries");
    if (const int rc = check_index_state(ix)) return rc;
    return on_one_shard(ix->owner, "host memory for a row-hash lookup", [&](Shard& s) { return find_rows(s, ix, nullptr, queries, nq, row, size); });
}

int gsim_rowhash_find_db(const gsim_rowhash* ix, gsim_db* left, uint64_t lrow_begin, uint64_t lrow_end, uint32_t* row, uint32_t* size)
{
    if (!ix) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (const int rc = check_left_handle(ix->owner, left, lrow_end)) return rc;
    if (lrow_begin > lrow_end) return fail(GSIM_ERR_INVALID, "left row range: begin past end");
    if (lrow_begin < lrow_end && !row) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (ix->nrows != ix->owner->nrows || ix->row_base != ix->owner->row_base) {
        if (const int rc = check_table_state(ix->owner, "row hashes", true)) return rc;
        return fail(GSIM_ERR_STATE, "the table changed after the row hash was made");
    }
    LeftSide ls;
    if (const int rc = ls.from_handle(ix->owner, left, lrow_begin, lrow_end, "row-hash lookups")) return rc;
    Shard& s = ix->owner->shards[0];
    int rc;
    try {
        rc = find_rows(s, ix, ls.rows, nullptr, ls.nl, row, size);
    } catch (const std::bad_alloc&) {
        rc = fail(GSIM_ERR_NOMEM, "host memory for a row-hash lookup");
    }
    if (rc != GSIM_OK) s.state_dirty = true;
    return rc;
}

int gsim_rowhash_destroy(gsim_rowhash* ix)
{
    if (!ix) return GSIM_OK;
    (void) set_device(ix->device);
    delete ix;
    return GSIM_OK;
}

} // extern "C"
