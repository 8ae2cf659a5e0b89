// irm_k_forward.hpp — k_forward, the α-space evaluation kernel of the host API (evaluate, cost, cost + grad,
// constraints) of one D.  Included by irm_kernels_impl.hpp; launched by launch_forward_dim (irm_launch.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "irm_alpha_exact.hpp"  // eval_exact, grad_exact
#include "irm_kernels.hpp"
#include "irm_physics.hpp"      // per-waypoint physics and its reductions

namespace irm {

// --------------------------------------------------- α-space eval kernels
// mode 0: evaluate (K or dK)·α·J; 1: cost; 2: cost + grad; 3: constraints.
// trajectory.py:63-65, 271-297, 129-180; same lane mapping as k_optimize.
template <int D, int MAXT>
__global__ __launch_bounds__(MAXT) void k_forward(KParams P, int mode) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Plan L = plan_lds(P, false, false, false, P.moving != 0, P.via != 0);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = P.N, NW = P.NW, TB = P.TB, MP = P.MP;
    const int WPT = NW >> 6;
    const int t = wave / WPT;
    const int n = tid - t * NW;
    const int tb0 = blockIdx.x * TB;
    const int ntb = min(TB, P.B - tb0);
    if (ntb <= 0) return;
    const bool tvalid = t < ntb;
    const bool valid = tvalid && n < N;
    const size_t b = (size_t)(tb0 + (tvalid ? t : 0));
    float* XG = smem + L.X;
    float* red = smem + L.red;
    float* sg = smem + L.sg;
    float* obsL = smem + L.obs;
    float* viaw = smem + L.via;  // (a via launch: L.via is a region of its own)

    stage_obstacles<true>(P, tb0, ntb, obsL);
    stage_alpha<D>(P, tb0, ntb, XG, MP);
    __syncthreads();
    float q[D], v[D], s[D], g[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        q[k] = v[k] = 0.f;
        s[k] = tvalid ? P.start[b * D + k] : 0.f;
        g[k] = tvalid ? P.goal[b * D + k] : 0.f;
    }
    if (valid) eval_exact<D>(P, XG + t * D, n, q, v);
    __syncthreads();
    if (mode == 0) {
        if (valid) {
#pragma unroll
            for (int k = 0; k < D; ++k) P.out0[(b * N + n) * D + k] = P.which ? v[k] : q[k];
        }
        return;
    }
    WP<D> w;
    const bool task_row = P.task && valid && n == N - 1;
    float task_r2 = 0.f;
    // via-points: the lane of row m_v (rows lie in 1 … N−2, so never a start / goal row)
    const int via = (P.via && valid) ? via_code(P, n) : -1;
    if (tvalid) {
        // (obstacles: shared only here, obs_stride 0 — the velocity table follows the one position table)
        EE<D> ee;
        if (valid) eval_waypoint_rt<D, true>(P, q, v, obsL, w, obsL + obs_vel_offset(P), P.moving ? P.tsup[n] : 0.f, &ee);
        // end-effector goal: ge = J_eeᵀ·(f − p) replaces this lane's copy of the joint goal
        if (task_row) task_end_row<D>(ee, P.goal_xy[b * 2], P.goal_xy[b * 2 + 1], g, task_r2);
        // via row: ge_v replaces this lane's copy of the joint goal (an interior row never reads it) and r_v²
        // goes to the trajectory's via words
        if (via >= 0) {
            float r2 = 0.f;
            via_row_terms<D, false>(P, b, via, q, ee, g, r2);
            viaw[t * IRM_MAX_VIA + (via & 3)] = r2;
        }
        eval_partials<D>(P, valid, w, n, wave, q, v, s, g, red, sg, t, task_row, task_r2);
    }
    __syncthreads();
    EvalOut E{};
    const int nvia = P.via ? P.n_via : 0;
    if (tvalid) E = eval_finalize(P, red, sg, t, t * WPT, WPT, P.lam_sg, P.lam_jl, viaw, nvia);
    if (tvalid && n == 0) {
        if (mode == 1 || mode == 2) {
            if (P.out0) P.out0[b] = E.loss;
        } else if (mode == 3) {
            const bool f0 = E.ds < P.eps_p && E.dg < P.eps_p;
            const bool f1 = E.vs < P.eps_v && E.vg < P.eps_v;
            const bool f2 = E.tmax <= P.pmax && E.tmin >= P.pmin;
            const bool f3 = E.vabs <= P.vmax;
            bool fv = true;  // every via distance below eps_position (the 11-float report stays as it is)
            for (int i = 0; i < nvia; ++i) {
                const float dv = sqrtf(viaw[t * IRM_MAX_VIA + i]);
                fv = fv && dv < P.eps_p;
                if (P.out1) P.out1[b * nvia + i] = dv;
            }
            if (P.out_ok) P.out_ok[b] = (f0 && f1 && f2 && f3 && fv) ? 1 : 0;
            if (P.out0) {
                float* r = P.out0 + b * 11;
                r[0] = E.ds; r[1] = E.dg; r[2] = E.vs; r[3] = E.vg;
                r[4] = E.tmax; r[5] = E.tmin; r[6] = E.vabs;
                r[7] = f0; r[8] = f1; r[9] = f2; r[10] = f3;
            }
        }
    }
    if (mode != 2) return;
    if (valid) {
        float a[D], bb[D];
        grad_waypoint<D>(P, w, q, v, n, E.idx, P.lam_sg, P.lam_jl, s, g, a, bb, task_row, via >= 0);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            XG[n * kLd + t * D + k] = a[k];
            XG[(N + n) * kLd + t * D + k] = bb[k];
        }
    }
    __syncthreads();
    // G = (Kᵀa + dKᵀb)·Jᵀ  (trajectory.py:295)
    if (valid) {
        float G[D];
        grad_exact<D>(P, XG + t * D, n, G);
#pragma unroll
        for (int k = 0; k < D; ++k) P.out1[(b * N + n) * D + k] = G[k];
    }
}

}  // namespace irm
