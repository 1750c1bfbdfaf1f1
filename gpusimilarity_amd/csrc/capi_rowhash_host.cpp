// capi_rowhash_host.cpp -- gsim_row_hash and gsim_duplicates: the row hash and the duplicate groups of gsim_rowhash_* on the host.
// No device, no handle, no HIP: the file depends on the public header, on gsim_rowhash_hash.h (the hash, <stdint.h> alone) and on
// fail() (as capi_popindex_host.cpp), so that tests/cpp/rowhash_host_check.cpp can be built with it under the sanitizers.  The rule is
// stated in include/gpusim_hip.h; gsim_rowhash.hip computes the same on the device.
#include "../../include/gpusim_hip.h"

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "gsim_rowhash_hash.h"

namespace gsim_host
{
int fail(int code, const std::string& msg);
}

using gsim_host::fail;

namespace
{

int check_rows(const uint32_t* rows, uint64_t nrows, uint32_t fp_bits)
{
    if (fp_bits == 0 || fp_bits % 32 != 0 || fp_bits > 32768) return fail(GSIM_ERR_INVALID, "fp_bits must be a positive multiple of 32, <= 32768");
    if (nrows && !rows) return fail(GSIM_ERR_INVALID, "NULL rows");
    if (nrows >= GSIM_ROW_NONE) return fail(GSIM_ERR_INVALID, "row hashes: 2^32 - 1 rows or more");
    return GSIM_OK;
}

uint64_t hash_row(const uint32_t* r, uint32_t W)
{
    uint32_t A = 0, B = 0;
    for (uint32_t i = 0; i < W; i++) gsim::rowhash_word(r[i], gsim::rowhash_key(i), A, B);
    return gsim::rowhash_final(A, B);
}

} // namespace

extern "C" int gsim_row_hash(const uint32_t* rows, uint64_t nrows, uint32_t fp_bits, uint64_t* hash)
{
    if (const int rc = check_rows(rows, nrows, fp_bits)) return rc;
    if (nrows && !hash) return fail(GSIM_ERR_INVALID, "NULL argument");
    const uint32_t W = fp_bits / 32;
    for (uint64_t i = 0; i < nrows; i++) hash[i] = hash_row(rows + i * W, W);
    return GSIM_OK;
}

// The device's table on the host: rows enter in ascending order, so the occupant of a slot is its group's first row from the start.
extern "C" int gsim_duplicates(const uint32_t* rows, uint64_t nrows, uint32_t fp_bits, uint32_t* first, uint32_t* size, uint64_t* ngroups)
{
    if (const int rc = check_rows(rows, nrows, fp_bits)) return rc;
    const uint32_t W = fp_bits / 32;
    const uint64_t nslots = gsim::rowhash_slots(nrows);
    uint64_t groups = 0;
    try {
        std::vector<uint32_t> slot(static_cast<size_t>(nslots), GSIM_ROW_NONE);
        std::vector<uint32_t> first_of(first ? 0 : static_cast<size_t>(nrows)), count(static_cast<size_t>(nrows), 0);
        uint32_t* f = first ? first : first_of.data();
        for (uint64_t i = 0; i < nrows; i++) {
            const uint32_t* r = rows + i * W;
            uint64_t s = hash_row(r, W) & (nslots - 1);
            while (slot[s] != GSIM_ROW_NONE && std::memcmp(rows + static_cast<uint64_t>(slot[s]) * W, r, static_cast<size_t>(W) * 4) != 0)
                s = (s + 1) & (nslots - 1); // (ends: at most half the slots are taken)
            if (slot[s] == GSIM_ROW_NONE) {
                slot[s] = static_cast<uint32_t>(i);
                groups++;
            }
            f[i] = slot[s];
            count[slot[s]]++;
        }
        if (size)
            for (uint64_t i = 0; i < nrows; i++) size[i] = count[f[i]];
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "host memory for the duplicate groups");
    }
    if (ngroups) *ngroups = groups;
    return GSIM_OK;
}
