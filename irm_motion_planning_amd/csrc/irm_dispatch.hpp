// irm_dispatch.hpp — host-side launch helpers: run-time D and workgroup size to a template argument
// (dispatch_d, dispatch_t) and a launch with its dynamic LDS request (launch_lds).  Host code only.
// Included by every unit that launches a kernel: irm_kernels.hip, irm_dense.hip, irm_clearance.hip,
// irm_self_clearance.hip, irm_fit.hip, irm_kernels_impl.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace irm {

template <class Fn>
inline hipError_t dispatch_d(int D, Fn&& fn) {
    switch (D) {
        case 1: return fn(std::integral_constant<int, 1>{});
        case 2: return fn(std::integral_constant<int, 2>{});
        case 3: return fn(std::integral_constant<int, 3>{});
        case 4: return fn(std::integral_constant<int, 4>{});
        case 5: return fn(std::integral_constant<int, 5>{});
        case 6: return fn(std::integral_constant<int, 6>{});
        case 7: return fn(std::integral_constant<int, 7>{});
        case 8: return fn(std::integral_constant<int, 8>{});
        default: return hipErrorInvalidValue;
    }
}

template <class Fn>
inline hipError_t dispatch_t(int BT, Fn&& fn) {
    if (BT <= 256) return fn(std::integral_constant<int, 256>{});
    if (BT <= 512) return fn(std::integral_constant<int, 512>{});
    if (BT <= 1024) return fn(std::integral_constant<int, 1024>{});
    return hipErrorInvalidValue;
}

template <class K, class... Args>
inline hipError_t launch_lds(K kernel, int grid, int threads, size_t lds, hipStream_t s, Args... args) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, args...);
    return hipGetLastError();
}

template <class T>
struct type_tag {
    using type = T;
};

}  // namespace irm
