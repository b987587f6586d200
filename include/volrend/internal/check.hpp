// The host layer's throwing checks: a failed C ABI call or HIP call becomes
// std::runtime_error("<what>: <reason>").  hip_check exists in the translation units that are
// built against the HIP runtime (-D__HIP_PLATFORM_AMD__); vr_check everywhere.
#pragma once
#include <stdexcept>
#include <string>

#include "volrend_hip.h"

#ifdef __HIP_PLATFORM_AMD__
#include <hip/hip_runtime_api.h>
#endif

namespace volrend {
namespace internal {

inline void vr_check(int rc, const char* what) {
    if (rc != VR_OK) throw std::runtime_error(std::string(what) + ": " + vr_last_error());
}

#ifdef __HIP_PLATFORM_AMD__
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#endif

}  // namespace internal
}  // namespace volrend
