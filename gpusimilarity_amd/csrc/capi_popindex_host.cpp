// capi_popindex_host.cpp -- gsim_popcount_bounds: the popcount bound of gsim_db_search_bounded on the host.  No device, no handle,
// no HIP: the file depends on the public header and on fail() alone (as capi_snn_host.cpp), so that tests/cpp/popindex_host_check.cpp
// can be built with it under the sanitizers.  The rule is stated in include/gpusim_hip.h; popindex_bounds_kernel (gsim_popindex.hip)
// computes the same table on the device.
#include "../../include/gpusim_hip.h"

#include <limits>
#include <string>

namespace gsim_host
{
int fail(int code, const std::string& msg);
}

using gsim_host::fail;

namespace
{

// score_of (gsim_device_common.h) on the host: one rounding per operation, in its order (the file is built with -ffp-contract=off)
float score_host(int metric, float alpha, float beta, uint32_t a, uint32_t b, uint32_t c)
{
    if (metric == GSIM_METRIC_TVERSKY) {
        const float t1 = alpha * static_cast<float>(static_cast<int>(a - c));
        const float t2 = beta * static_cast<float>(static_cast<int>(b - c));
        const float den = (t1 + t2) + static_cast<float>(c);
        return static_cast<float>(c) / den;
    }
    const int total = static_cast<int>(a + b);
    return static_cast<float>(static_cast<int>(c)) / static_cast<float>(total - static_cast<int>(c));
}

} // namespace

extern "C" int gsim_popcount_bounds(uint32_t fp_bits, uint32_t popc_query, int metric, float alpha, float beta, float* ub)
{
    if (!ub) return fail(GSIM_ERR_INVALID, "NULL argument");
    if (fp_bits == 0 || fp_bits % 32 != 0 || fp_bits > 32768) return fail(GSIM_ERR_INVALID, "fp_bits must be a positive multiple of 32, <= 32768");
    if (popc_query > fp_bits) return fail(GSIM_ERR_INVALID, "popcount bounds: the query's popcount exceeds fp_bits");
    if (metric != GSIM_METRIC_TANIMOTO && metric != GSIM_METRIC_TVERSKY) return fail(GSIM_ERR_INVALID, "unknown metric");
    const uint32_t a = popc_query;
    for (uint32_t b = 0; b <= fp_bits; b++) {
        const uint32_t c0 = a + b > fp_bits ? a + b - fp_bits : 0u;
        const uint32_t c1 = a < b ? a : b;
        float m = -std::numeric_limits<float>::infinity();
        for (uint32_t c = c0; c <= c1; c++) {
            float s = score_host(metric, alpha, beta, a, b, c);
            s = s == s ? s : 0.0f; // (NaN, 0 / 0: taken as 0)
            m = s > m ? s : m;
        }
        ub[b] = m;
    }
    return GSIM_OK;
}
