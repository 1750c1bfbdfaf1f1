// capi_label_sums_host.cpp -- gsim_label_silhouette and gsim_label_medoids: what a caller makes of gsim_db_label_sums' integers on
// the host.  No device, no handle, no HIP: the file depends on the public header and on fail() alone, so that
// tests/cpp/label_sums_host_check.cpp can be built with it under the sanitizers.  The operations are stated in include/gpusim_hip.h
// and made in exactly that order; the file is compiled with -ffp-contract=off (as all of the library), so nothing is fused.
#include "../../include/gpusim_hip.h"

#include <cmath>
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

// INVALID "<what>: the label of row i is not below nlabels"; counts the rows of every label
int count_labels(const char* what, const uint32_t* labels, uint64_t n, uint32_t nlabels, std::vector<uint32_t>* count)
{
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t l = labels[i];
        if (l == GSIM_LABEL_NONE) continue;
        if (l >= nlabels) return fail(GSIM_ERR_INVALID, std::string(what) + ": the label of row " + std::to_string(i) + " is not below nlabels");
        if (count) (*count)[l]++;
    }
    return GSIM_OK;
}

} // namespace

extern "C" {

int gsim_label_silhouette(const uint32_t* labels, const uint64_t* own_q, const uint32_t* other_label, const uint64_t* other_q, const uint32_t* sizes,
                          uint64_t n, uint32_t nlabels, double* sil, double* label_mean, double* mean)
{
    if (nlabels == 0) return fail(GSIM_ERR_INVALID, "label silhouette: nlabels == 0");
    if (!sizes) return fail(GSIM_ERR_INVALID, "label silhouette: NULL sizes");
    if (n && (!labels || !own_q || !other_label || !other_q || !sil)) return fail(GSIM_ERR_INVALID, "label silhouette: NULL argument");
    if (n > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "label silhouette: 2^32 rows or more");
    try {
        std::vector<uint32_t> count(nlabels, 0u);
        if (const int rc = count_labels("label silhouette", labels, n, nlabels, &count)) return rc;
        for (uint32_t l = 0; l < nlabels; l++)
            if (count[l] != sizes[l]) return fail(GSIM_ERR_INVALID, "label silhouette: sizes[" + std::to_string(l) + "] disagrees with the labels");
        for (uint64_t i = 0; i < n; i++) { // (nothing is written when anything is refused)
            const uint32_t o = other_label[i];
            if (o == GSIM_LABEL_NONE) continue;
            if (labels[i] == GSIM_LABEL_NONE || o >= nlabels || o == labels[i] || sizes[o] == 0)
                return fail(GSIM_ERR_INVALID, "label silhouette: the other label of row " + std::to_string(i) +
                                                  " is the row's own, not below nlabels, without rows, or that of an unlabelled row");
        }
        std::vector<double> sum(label_mean ? nlabels : 0u, 0.0);
        double total = 0.0;
        uint64_t labelled = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t L = labels[i];
            double v = 0.0;
            if (L != GSIM_LABEL_NONE && sizes[L] >= 2 && other_label[i] != GSIM_LABEL_NONE) {
                const double a = static_cast<double>(own_q[i]) / static_cast<double>(sizes[L] - 1u) * 0x1p-31;
                const double b = static_cast<double>(other_q[i]) / static_cast<double>(sizes[other_label[i]]) * 0x1p-31;
                const double d = 1.0 - std::fmin(a, b);
                v = d > 0 ? (a - b) / d : 0.0;
            }
            sil[i] = v;
            if (L == GSIM_LABEL_NONE) continue;
            if (label_mean) sum[L] += v;
            total += v;
            labelled++;
        }
        if (label_mean)
            for (uint32_t l = 0; l < nlabels; l++) label_mean[l] = sizes[l] ? sum[l] / static_cast<double>(sizes[l]) : 0.0;
        if (mean) *mean = labelled ? total / static_cast<double>(labelled) : 0.0;
    } catch (const std::bad_alloc&) {
        return fail(GSIM_ERR_NOMEM, "host memory for the label silhouette");
    }
    return GSIM_OK;
}

int gsim_label_medoids(const uint32_t* labels, const uint64_t* own_q, uint64_t n, uint32_t nlabels, uint32_t* medoid)
{
    if (nlabels == 0) return fail(GSIM_ERR_INVALID, "label medoids: nlabels == 0");
    if (!medoid) return fail(GSIM_ERR_INVALID, "label medoids: NULL medoid");
    if (n && (!labels || !own_q)) return fail(GSIM_ERR_INVALID, "label medoids: NULL argument");
    if (n > 0xFFFFFFFFull) return fail(GSIM_ERR_INVALID, "label medoids: 2^32 rows or more");
    if (const int rc = count_labels("label medoids", labels, n, nlabels, nullptr)) return rc;
    for (uint32_t l = 0; l < nlabels; l++) medoid[l] = GSIM_LABEL_NONE;
    for (uint64_t i = 0; i < n; i++) { // ascending rows: only a strictly greater sum replaces the holder
        const uint32_t l = labels[i];
        if (l == GSIM_LABEL_NONE) continue;
        if (medoid[l] == GSIM_LABEL_NONE || own_q[i] > own_q[medoid[l]]) medoid[l] = static_cast<uint32_t>(i);
    }
    return GSIM_OK;
}

} // extern "C"
