// irm_dense_sample.hpp — what the kernels that evaluate a trajectory at the context's evaluation times share:
// the workgroup shape, the staging of a problem's α into LDS and one lane's sample q(t_eval[i]), v(t_eval[i]) in
// irm_eval_any's arithmetic.  Included by irm_dense.hip (k_eval_any, k_dense_check), irm_clearance.hip
// (k_clearance) and irm_self_clearance.hip (k_self_clearance).
#pragma once
#include <hip/hip_runtime.h>

#include "irm_kernels.hpp"

namespace irm {

constexpr int kDenseT = 256;  // threads per workgroup = evaluation times per chunk
constexpr int kDenseU = 8;    // query-matrix rows per software-pipelined batch (eval_exact's U)

// Evaluation time i (lane) of the problem whose α is Al (LDS, [N][D]): q = fp32(fp32(Kq·α)[i]·J) and, with
// BOTH, v from dKq the same way.  kqT / dkqT: [N][M].
template <int D, bool BOTH>
__device__ __forceinline__ void dense_sample(const KParams& P, const float* __restrict__ Al,
                                             const float* __restrict__ kqT, const float* __restrict__ dkqT,
                                             unsigned M, unsigned i, float (&q)[D], float (&v)[D]) {
    constexpr int U = kDenseU;
    const int N = P.N;
    double aq[D], av[D];
#pragma unroll
    for (int d = 0; d < D; ++d) aq[d] = av[d] = 0.0;
    const int nb = N / U;
    const int m0 = nb * U;
    if (nb > 0) {
        float kq[U], kv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kq[u] = kqT[(unsigned)u * M + i];
            kv[u] = BOTH ? dkqT[(unsigned)u * M + i] : 0.f;
        }
        for (int bi = 0; bi < nb; ++bi) {
            const int mb = bi * U;
            float nq[U], nv[U];
            const int mn = (bi + 1 < nb) ? mb + U : mb;  // (the last batch re-reads itself: no branch)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                nq[u] = kqT[(unsigned)(mn + u) * M + i];
                nv[u] = BOTH ? dkqT[(unsigned)(mn + u) * M + i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float* xr = Al + (mb + u) * D;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double x = (double)xr[d];
                    aq[d] = fma((double)kq[u], x, aq[d]);
                    if constexpr (BOTH) av[d] = fma((double)kv[u], x, av[d]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                kq[u] = nq[u];
                kv[u] = nv[u];
            }
        }
    }
    for (int m = m0; m < N; ++m) {
        const double kq = (double)kqT[(unsigned)m * M + i];
        const double kv = BOTH ? (double)dkqT[(unsigned)m * M + i] : 0.0;
        const float* xr = Al + m * D;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double x = (double)xr[d];
            aq[d] = fma(kq, x, aq[d]);
            if constexpr (BOTH) av[d] = fma(kv, x, av[d]);
        }
    }
    float tq[D], tv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        tq[d] = (float)aq[d];
        tv[d] = (float)av[d];
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double sq = 0.0, sv = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            sq = fma((double)tq[d], (double)P.J[d * D + k], sq);
            if constexpr (BOTH) sv = fma((double)tv[d], (double)P.J[d * D + k], sv);
        }
        q[k] = (float)sq;
        v[k] = (float)sv;
    }
}

// α of problem b into LDS ([N][D], as it lies in memory).
template <int D>
__device__ __forceinline__ void dense_stage_alpha(const KParams& P, int b, float* Al) {
    const int nd = P.N * D;
    const float* src = P.alpha0 + (size_t)b * nd;
    for (int e = threadIdx.x; e < nd; e += kDenseT) Al[e] = src[e];
}

}  // namespace irm
