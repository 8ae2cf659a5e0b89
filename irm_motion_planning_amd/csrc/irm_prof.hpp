// irm_prof.hpp — the phase profiler of the optimiser kernels (IRM_PHASE_PROFILE builds) and the
// IRM_STAMP / IRM_COUNT macros the kernels mark their phases with (IRM_ISA_MARKS: markers in the assembly).
// Included by irm_kernels_impl.hpp, whose kernels stamp phases.
#pragma once
#include <hip/hip_runtime.h>

#include "irm_kernels.hpp"

namespace irm {

// ---------------------------------------------------- phase profiler (diag)
// Built with -DIRM_PHASE_PROFILE: thread 0 of each workgroup accumulates the
// shader-clock cycles (s_memtime) between consecutive stamps per phase into
// P.prof[block][phase].  In the shipped build every stamp is empty.
struct Prof {
#ifdef IRM_PHASE_PROFILE
    unsigned long long last, acc[kProfPhases];
    __device__ __forceinline__ void init() {
        last = __builtin_amdgcn_s_memtime();
#pragma unroll
        for (int i = 0; i < kProfPhases; ++i) acc[i] = 0;
    }
    __device__ __forceinline__ void stamp(int ph) {
        unsigned long long now = __builtin_amdgcn_s_memtime();
        acc[ph] += now - last;
        last = now;
    }
    __device__ __forceinline__ void count(int ph, bool c) {
        if (c) acc[ph] += 1;
    }
    __device__ __forceinline__ void flush(unsigned long long* out) {
        if (out)
            for (int i = 0; i < kProfPhases; ++i) out[(size_t)blockIdx.x * kProfPhases + i] = acc[i];
    }
#else
    __device__ __forceinline__ void init() {}
    __device__ __forceinline__ void stamp(int) {}
    __device__ __forceinline__ void count(int, bool) {}
    __device__ __forceinline__ void flush(unsigned long long*) {}
#endif
};
#ifdef IRM_ISA_MARKS  // analysis builds: phase markers in the emitted assembly
#define IRM_STAMP(ph) asm volatile("; IRM_PHASE " #ph)
#define IRM_COUNT(ph, c)
#else
#define IRM_STAMP(ph)                         \
    do {                                      \
        if (threadIdx.x == 0) prof.stamp(ph); \
    } while (0)
#define IRM_COUNT(ph, c)                          \
    do {                                          \
        if (threadIdx.x == 0) prof.count(ph, c);  \
    } while (0)
#endif

}  // namespace irm
