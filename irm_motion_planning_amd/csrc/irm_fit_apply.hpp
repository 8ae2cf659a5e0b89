// irm_fit_apply.hpp — what the kernels that apply a host-built fp64 fit operator share (irm_fit.hip: fit_alpha,
// transfer_alpha; irm_multistart.hip: the seed ensemble, whose α is fit_alpha's arithmetic on waypoints the kernel
// forms itself): the workgroup shape and the FMA chain of one output waypoint.  See irm_fit.hip for the layout.
#pragma once
#include <hip/hip_runtime.h>

namespace irm {

constexpr int kFitT = 256;  // threads per workgroup at most (N ≤ 192 runs ⌈N/64⌉ waves)
constexpr int kFitU = 4;    // operator rows per software-pipelined batch
// problems per workgroup: kFitP·D ≤ 16 fp64 accumulators per lane, at most 64 KiB of staged rows (n_src = 512)
template <int D>
constexpr int fit_problems() { return D <= 4 ? 4 : 2; }

static int fit_threads(int N) { return N >= kFitT ? kFitT : (N + 63) / 64 * 64; }

// acc[c] = Σ_m opT[m][n]·X[m][c] for the C = problems·D columns of waypoint n (lane), m ascending.
template <int C>
__device__ __forceinline__ void fit_apply(const double* __restrict__ opT, unsigned N, int M, unsigned n,
                                          const double* __restrict__ X, double (&acc)[C]) {
    constexpr int U = kFitU;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    const int nb = M / U;
    const int m0 = nb * U;
    if (nb > 0) {
        double w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) w[u] = opT[(unsigned)u * N + n];
        for (int bi = 0; bi < nb; ++bi) {
            const int mb = bi * U;
            double nw[U];
            const int mn = (bi + 1 < nb) ? mb + U : mb;  // (the last batch re-reads itself: no branch)
#pragma unroll
            for (int u = 0; u < U; ++u) nw[u] = opT[(unsigned)(mn + u) * N + n];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double* xr = X + (mb + u) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = fma(w[u], xr[c], acc[c]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) w[u] = nw[u];
        }
    }
    for (int m = m0; m < M; ++m) {
        const double w = opT[(unsigned)m * N + n];
        const double* xr = X + m * C;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = fma(w, xr[c], acc[c]);
    }
}

template <int D>
static size_t fit_lds(int M) {
    constexpr int C = fit_problems<D>() * D;
    return (size_t)M * C * sizeof(double) + 16 * sizeof(float);
}

}  // namespace irm
