// irm_alpha_exact.hpp — the correctly rounded α-space maps (eval_exact, eval_exact_loop, grad_exact): fp64
// sums rounded once, bit-identical to the CPU oracle.  Off the hot loop: prologue, resyncs, k_forward.
// Included by irm_kernels_impl.hpp (k_optimize, k_lean) and irm_k_forward.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "irm_kernels.hpp"  // KParams, kLd

namespace irm {

// ------------------------------------------- correctly rounded α-space maps
// The reference's K@α@J (trajectory.py:63-65) contracts over N waypoints with
// |α| ≈ 1e3 (singular K): a plain fp32 sum carries ~1e-4 (positions) and
// ~1e-3 (velocities) of order-dependent noise.  Here every product of two
// fp32 values is exact in fp64 and the N-term sum accumulates in fp64 (same
// sequential order as oracle/irm_oracle.c), then rounds once — the result is
// the correctly rounded fp32 value, bit-identical to the CPU oracle.  Used off
// the hot loop: host-API evaluation and the optimiser's prologue / resyncs.
//
// Lane n of trajectory column block Xa (LDS, rows m = 0..N-1, stride kLd):
//   q = fp32(fp32(K·α)[n]·J), v = fp32(fp32(dK·α)[n]·J).
// (rs, cs: row / column strides of Xa — [row][16] LDS buffers by default, the lean kernel's
// column-major buffers with rs = 1, cs = column stride)
// U: K / dK rows per software-pipelined batch (8 in the prologue / epilogue; the optimiser loop's resync
// rounds use 2, which keeps the register peak of the dual-loop / BLS instantiations low — spill-free —
// at the cost of less latency hiding in a round that runs once per outer iteration)
// JL: J (D×D) from Jm, an LDS copy (inside the optimiser loop, whose reads are not hoisted: the D² fp64
// conversions of P.J hoisted out of the round loop held 2·D² VGPRs), else from P.J.  A compile-time
// choice: a run-time select between &P.J and an LDS address takes the kernel argument's address, and the
// compiler then copies all of KParams into scratch and reads every parameter from there (1.8 KB of
// scratch and ≈60 scratch loads in the dual-loop / BLS rounds, round 4)
template <int D, int U = 8, bool JL = false>
__device__ void eval_exact(const KParams& P, const float* __restrict__ Xa, int n, float (&q)[D], float (&v)[D],
                           const float* Kt = nullptr, const float* dKt = nullptr, int rs = kLd, int cs = 1,
                           const float* Jm = nullptr) {
    const float* J;
    if constexpr (JL) J = Jm;
    else J = P.J;
    const int N = P.N;
    double aq[D], av[D];
#pragma unroll
    for (int d = 0; d < D; ++d) aq[d] = av[d] = 0.0;
    // wave-uniform bases and 32-bit element offsets (global loads with an SGPR base and a VGPR
    // offset): inside the optimiser loop a per-lane 64-bit pointer would be hoisted out of the loop
    // and held (or spilled) across every round
    const float* kt = Kt ? Kt : P.Kt;
    const float* dkt = dKt ? dKt : P.dKt;
    const unsigned un = (unsigned)n, uN = (unsigned)N;
    // K / dK rows come from L2 / HBM: software-pipelined batches of U rows (the next batch's 2U
    // loads are in flight while this one is summed; the sum stays in the sequential order
    // m = 0, 1, …, N−1 of the oracle)
    const int nb = N / U;
    int m0 = nb * U;
    if (nb > 0) {
        float kq[U], kv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kq[u] = kt[(unsigned)u * uN + un];
            kv[u] = dkt[(unsigned)u * uN + un];
        }
        for (int bi = 0; bi < nb; ++bi) {
            const int mb = bi * U;
            float nq[U], nv[U];
            const int mn = (bi + 1 < nb) ? mb + U : mb;  // (the last batch re-reads itself: no branch)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                nq[u] = kt[(unsigned)(mn + u) * uN + un];   // K[n][m]
                nv[u] = dkt[(unsigned)(mn + u) * uN + un];  // dK[n][m]
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float* xr = Xa + (mb + u) * rs;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double x = (double)xr[d * cs];
                    aq[d] = fma((double)kq[u], x, aq[d]);
                    av[d] = fma((double)kv[u], x, av[d]);
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
        const double kq = (double)kt[(unsigned)m * uN + un], kv = (double)dkt[(unsigned)m * uN + un];
        const float* xr = Xa + m * rs;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double x = (double)xr[d * cs];
            aq[d] = fma(kq, x, aq[d]);
            av[d] = fma(kv, x, av[d]);
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
            sq = fma((double)tq[d], (double)J[d * D + k], sq);
            sv = fma((double)tv[d], (double)J[d * D + k], sv);
        }
        q[k] = (float)sq;
        v[k] = (float)sv;
    }
}

// eval_exact for one lane inside the optimiser loop (the lean kernel's resyncs at D > 3): the same sums
// in the same order, as one loop over m whose K / dK loads run PF rows ahead, J read from LDS (Jl).
// eval_exact's batched form kept ~80 more VGPRs live around the resync at D = 7 (its fp64 J products
// hoisted out of the round loop, and the batch's addressing): the 7-DoF dual-loop / BLS kernels spilled.
template <int D, int PF>
__device__ __forceinline__ void eval_exact_loop(const KParams& P, const float* __restrict__ Xc, int ldc, int n, int N,
                                                const float* Jl, float (&q)[D], float (&v)[D]) {
    const unsigned un = (unsigned)n, uN = (unsigned)N;
    double aq[D], av[D];
#pragma unroll
    for (int d = 0; d < D; ++d) aq[d] = av[d] = 0.0;
    float kq = P.Kt[un], kv = P.dKt[un];
#pragma unroll 1
    for (int m = 0; m < N; m += PF) {
        float nq[PF], nv[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) {  // rows m+1 … m+PF (clamped: the last rows re-read row N − 1)
            const unsigned mn = (unsigned)min(m + 1 + u, N - 1);
            nq[u] = P.Kt[mn * uN + un];
            nv[u] = P.dKt[mn * uN + un];
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if (PF == 1 || m + u < N) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double x = (double)Xc[d * ldc + m + u];
                    aq[d] = fma((double)kq, x, aq[d]);
                    av[d] = fma((double)kv, x, av[d]);
                }
            }
            kq = nq[u];
            kv = nv[u];
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
        // one column of J at a time: without the barrier the scheduler hoists all D² LDS reads and their fp64
        // conversions (2·D² = 98 VGPRs at D = 7) ahead of the first product — the resync's register peak
        __builtin_amdgcn_sched_barrier(0);
        double sq = 0.0, sv = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            sq = fma((double)tq[d], (double)Jl[d * D + k], sq);
            sv = fma((double)tv[d], (double)Jl[d * D + k], sv);
        }
        q[k] = (float)sq;
        v[k] = (float)sv;
    }
}

// G[n] = (fp32(Kᵀa)[n] + fp32(dKᵀb)[n])·Jᵀ  (trajectory.py:295), the N-sums
// in fp64 as above, the fp32 add and the D-term J product unfused in fp32
// (the oracle's order).  Xa: a in rows 0..N-1, b in rows N..2N-1.
template <int D>
__device__ void grad_exact(const KParams& P, const float* __restrict__ Xa, int n, float (&G)[D]) {
    const int N = P.N;
    double ga[D], gb[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ga[d] = gb[d] = 0.0;
    const float* km = P.Km + n;
    const float* dkm = P.dKm + n;
    for (int m = 0; m < N; ++m) {
        const double ka = (double)km[(size_t)m * N], kb = (double)dkm[(size_t)m * N];  // K[m][n], dK[m][n]
        const float* xa = Xa + m * kLd;
        const float* xb = Xa + (N + m) * kLd;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            ga[d] = fma(ka, (double)xa[d], ga[d]);
            gb[d] = fma(kb, (double)xb[d], gb[d]);
        }
    }
    float tmp[D];
#pragma unroll
    for (int d = 0; d < D; ++d) tmp[d] = __fadd_rn((float)ga[d], (float)gb[d]);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        float u = 0.f;
#pragma unroll
        for (int l = 0; l < D; ++l) u = __fadd_rn(u, __fmul_rn(tmp[l], P.J[k * D + l]));
        G[k] = u;
    }
}

}  // namespace irm
