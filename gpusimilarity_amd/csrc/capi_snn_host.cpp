// capi_snn_host.cpp -- gsim_snn and gsim_jarvis_patrick: shared-nearest-neighbour counts and Jarvis-Patrick clustering of any CSR of
// lists, on the host.  No device, no handle, no HIP: the file depends on the public header and on fail() alone (as
// capi_label_sums_host.cpp), so that tests/cpp/snn_host_check.cpp can be built with it under the sanitizers.  The rule is stated in
// include/gpusim_hip.h; gsim_db_snn and gsim_db_jarvis_patrick (capi_snn.cpp, gsim_snn.hip) apply it to gsim_db_knn's lists.
#include "../../include/gpusim_hip.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace gsim_host
{
int fail(int code, const std::string& msg);
}

using gsim_host::fail;

namespace
{

// The lists of a graph with their rows ascending, the owner of every entry, and the shared count of every entry.
struct Lists {
    std::vector<uint32_t> sorted, owner;

    // gsim_butina's checks of a graph (the messages of capi_pairs.cpp), then "snn: list r names its own row / names a row twice"
    int take(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows)
    {
        if (nrows > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "more than 2^32-1 rows");
        if (indptr[0] != 0) return fail(GSIM_ERR_INVALID, "indptr[0] must be 0");
        for (uint64_t r = 0; r < nrows; r++)
            if (indptr[r + 1] < indptr[r]) return fail(GSIM_ERR_INVALID, "indptr must not decrease");
        const uint64_t nnz = indptr[nrows];
        if (nnz && !indices) return fail(GSIM_ERR_INVALID, "NULL indices");
        for (uint64_t e = 0; e < nnz; e++)
            if (indices[e] >= nrows) return fail(GSIM_ERR_INVALID, "column index outside the graph");
        sorted.assign(indices, indices + nnz);
        owner.resize(nnz);
        for (uint64_t r = 0; r < nrows; r++) {
            const auto b = sorted.begin() + static_cast<std::ptrdiff_t>(indptr[r]), e = sorted.begin() + static_cast<std::ptrdiff_t>(indptr[r + 1]);
            std::sort(b, e);
            if (std::binary_search(b, e, static_cast<uint32_t>(r)))
                return fail(GSIM_ERR_INVALID, "snn: list " + std::to_string(r) + " names its own row");
            if (std::adjacent_find(b, e) != e) return fail(GSIM_ERR_INVALID, "snn: list " + std::to_string(r) + " names a row twice");
            std::fill(owner.begin() + static_cast<std::ptrdiff_t>(indptr[r]), owner.begin() + static_cast<std::ptrdiff_t>(indptr[r + 1]),
                      static_cast<uint32_t>(r));
        }
        return GSIM_OK;
    }

    // shared(i, j) | the mutual bit for the entry j of list i
    uint32_t shared(const uint64_t* indptr, uint32_t i, uint32_t j, bool closed) const
    {
        const uint32_t *a = sorted.data() + indptr[i], *ae = sorted.data() + indptr[i + 1];
        const uint32_t *b = sorted.data() + indptr[j], *be = sorted.data() + indptr[j + 1];
        const bool mutual = std::binary_search(b, be, i);
        uint32_t n = 0;
        while (a != ae && b != be) {
            if (*a < *b) a++;
            else if (*b < *a) b++;
            else {
                n++;
                a++;
                b++;
            }
        }
        if (closed) n += 1u + (mutual ? 1u : 0u);
        return n | (mutual ? GSIM_SNN_MUTUAL_BIT : 0u);
    }
};

// union-find over rows: the smaller index wins every hook, so a tree's root is its smallest row (as gsim_components)
uint32_t root_of(std::vector<uint32_t>& parent, uint32_t x)
{
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

} // namespace

extern "C" {

int gsim_snn(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, uint32_t flags, uint32_t* shared)
{
    if (!indptr) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (flags & ~GSIM_SNN_CLOSED) return fail(GSIM_ERR_INVALID, "snn: unknown flags");
    try {
        Lists l;
        if (const int rc = l.take(indptr, indices, nrows)) return rc;
        const uint64_t nnz = indptr[nrows];
        if (nnz && !shared) return fail(GSIM_ERR_INVALID, "NULL shared");
        for (uint64_t e = 0; e < nnz; e++) shared[e] = l.shared(indptr, l.owner[e], indices[e], (flags & GSIM_SNN_CLOSED) != 0);
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "host memory for snn");
    }
    return GSIM_OK;
}

int gsim_jarvis_patrick(const uint64_t* indptr, const uint32_t* indices, uint64_t nrows, const uint32_t* kmins, uint32_t nlevels,
                        uint32_t flags, uint32_t* cluster_of, uint32_t* first_row, uint32_t* sizes, uint32_t* nclusters)
{
    if (!indptr || !kmins || !nclusters || (nrows && !cluster_of)) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (flags & ~(GSIM_SNN_CLOSED | GSIM_SNN_EITHER)) return fail(GSIM_ERR_INVALID, "jarvis-patrick: unknown flags");
    if (nlevels < 1 || nlevels > GSIM_COMPONENTS_MAX_LEVELS) return fail(GSIM_ERR_INVALID, "jarvis-patrick: between 1 and 8 levels");
    for (uint32_t l = 1; l < nlevels; l++)
        if (!(kmins[l - 1] < kmins[l])) return fail(GSIM_ERR_INVALID, "jarvis-patrick: kmins must be strictly ascending");
    try {
        Lists ls;
        if (const int rc = ls.take(indptr, indices, nrows)) return rc;
        const uint64_t nnz = indptr[nrows];
        const bool closed = (flags & GSIM_SNN_CLOSED) != 0, either = (flags & GSIM_SNN_EITHER) != 0;
        std::vector<std::vector<uint32_t>> forests(nlevels, std::vector<uint32_t>(nrows));
        for (std::vector<uint32_t>& f : forests)
            for (uint64_t r = 0; r < nrows; r++) f[r] = static_cast<uint32_t>(r);
        for (uint64_t e = 0; e < nnz; e++) {
            const uint32_t i = ls.owner[e], j = indices[e];
            const uint32_t s = ls.shared(indptr, i, j, closed);
            if (!either && !(s & GSIM_SNN_MUTUAL_BIT)) continue;
            for (uint32_t l = 0; l < nlevels && (s & ~GSIM_SNN_MUTUAL_BIT) >= kmins[l]; l++) {
                const uint32_t x = root_of(forests[l], i), y = root_of(forests[l], j);
                if (x != y) forests[l][std::max(x, y)] = std::min(x, y);
            }
        }
        // rows ascending: a root comes before every other row of its cluster and takes the next number
        for (uint32_t l = 0; l < nlevels; l++) {
            std::vector<uint32_t>& forest = forests[l];
            uint32_t* out = cluster_of + l * nrows;
            uint32_t nc = 0;
            for (uint64_t r = 0; r < nrows; r++) {
                const uint32_t root = root_of(forest, static_cast<uint32_t>(r));
                if (root == r) {
                    out[r] = nc;
                    if (first_row) first_row[l * nrows + nc] = static_cast<uint32_t>(r);
                    if (sizes) sizes[l * nrows + nc] = 1;
                    nc++;
                } else {
                    out[r] = out[root];
                    if (sizes) sizes[l * nrows + out[root]]++;
                }
            }
            nclusters[l] = nc;
        }
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "host memory for jarvis-patrick");
    }
    return GSIM_OK;
}

} // extern "C"
