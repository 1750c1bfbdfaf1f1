// gsim_prims.hip -- device-wide primitives that more than one file uses, instantiated once: the exclusive prefix sum over 32-bit
// words (rocPRIM) behind the component and cluster numbering (gsim_components.hip, gsim_dbscan.hip), a row set's list offsets
// (capi_subset.cpp) and a popcount index's bucket starts (capi_popindex.cpp).  The u32 -> u64 scan of the k-NN lists, the radix
// sorts and the selects have one user each and stay in their files.
#include "gsim_device.h"

#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

namespace gsim
{

hipError_t scan_u32_bytes(uint64_t n, size_t* bytes)
{
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u,
                                   static_cast<size_t>(n), rocprim::plus<uint32_t>());
}

hipError_t launch_scan_u32(void* tmp, size_t tmp_bytes, const uint32_t* in, uint32_t* out, uint64_t n, hipStream_t s)
{
    size_t bytes = tmp_bytes;
    return rocprim::exclusive_scan(tmp, bytes, in, out, 0u, static_cast<size_t>(n), rocprim::plus<uint32_t>(), s);
}

} // namespace gsim
