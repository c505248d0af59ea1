// Host side of a launch that claims a large dynamic-LDS allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <utility>

namespace kjarni {

// A launch whose dynamic LDS exceeds the default limit needs hipFuncAttributeMaxDynamicSharedMemorySize raised on its kernel,
// per device.  allow_dynamic_lds raises it once per (kernel, device) -- again only when a later launch claims more -- under
// one lock, so concurrent host threads may call it, and returns the HIP error to the caller.  The attribute is host state,
// not a stream operation: a first call inside a stream capture (a captured decode step) sets it just as outside one.
inline hipError_t allow_dynamic_lds(const void* kernel, size_t bytes)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> allowed;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = allowed[{kernel, dev}];
    if (bytes <= have) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

template <typename F>
inline hipError_t allow_dynamic_lds(F* kernel, size_t bytes)
{
    return allow_dynamic_lds(reinterpret_cast<const void*>(kernel), bytes);
}

}  // namespace kjarni
