// irm_kernels.hip — gfx950 host-API kernels (fk, fk_joints, compute_cost_vg,
// initTrajectory) and the launch dispatch.  The optimiser / α-space kernels are
// templates in irm_kernels_impl.hpp, instantiated per shape in irm_opt_inst.hip; this unit
// sees their launchers' declarations only.
#include "irm_dispatch.hpp"
#include "irm_launch_decl.hpp"
#include "irm_opt_common.hpp"  // FixShape, DenseShape, DynShape
#include "irm_physics.hpp"     // sincos_fast

namespace irm {

IRM_FIX_SHAPES(IRM_EXTERN_FIX)
IRM_DENSE_SHAPES(IRM_EXTERN_DENSE)
IRM_DYN_DIMS(IRM_EXTERN_DYN)

// ------------------------------------------- per-waypoint utility kernels
// robot.py:29-36 + 75-87 for B×N waypoints.
template <int D>
__global__ void k_fk(KParams P, const float* traj, float* pos, float* jac) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = P.N;
    if (i >= P.B * N) return;
    const int b = i / N, n = i - b * N;
    const float* q = traj + (size_t)i * D;
    float cum = 0.f, fx = 0.f, fy = 0.f, Sx = 0.f, Sy = 0.f, xs[D], ys[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        cum += q[d];
        float sn, cs;
        sincos_fast(cum, sn, cs);
        fx += P.link[d] * cs;
        fy += P.link[d] * sn;
        xs[d] = -(P.link[d] * sn);
        ys[d] = P.link[d] * cs;
        Sx += xs[d];
        Sy += ys[d];
    }
    pos[(size_t)b * 2 * N + n] = fx;
    pos[(size_t)b * 2 * N + N + n] = fy;
    if (!jac) return;
    float Cx = 0.f, Cy = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        Cx += xs[d];
        Cy += ys[d];
        jac[(((size_t)b * 2 + 0) * N + n) * D + d] = (xs[d] + Sx) - Cx;
        jac[(((size_t)b * 2 + 1) * N + n) * D + d] = (ys[d] + Sy) - Cy;
    }
}

// robot.py:39-72 (fk_joint_j, generalised to j = 1..D) for B×N waypoints:
// pos[b][j−1] = (Σ_{l<j} L_l cos c_l, Σ_{l<j} L_l sin c_l), B×D×2×N.
template <int D>
__global__ void k_fk_joints(KParams P, const float* traj, float* pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = P.N;
    if (i >= P.B * N) return;
    const int b = i / N, n = i - b * N;
    const float* q = traj + (size_t)i * D;
    float cum = 0.f, fx = 0.f, fy = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        cum += q[d];
        float sn, cs;
        sincos_fast(cum, sn, cs);
        fx += P.link[d] * cs;
        fy += P.link[d] * sn;
        float* o = pos + (((size_t)b * D + d) * 2) * N + n;
        o[0] = fx;
        o[N] = fy;
    }
}

// environment.py:32-58 for B×N points (shared obstacles).  Each obstacle's term and the three sums are formed in
// fp64 from the fp32 inputs and rounded once: the gradient of a point among many obstacles is a sum of terms of
// magnitude up to 1 that cancel, and an fp32 sum of them (half an ulp of 1 per addition, 3 ulp per term through
// v_rcp_f32) misses the host API's elementwise bound rtol 1e-5 + atol 1e-7 from 8 obstacles on
// (tests/test_gpu_physics.py, test_obstacle_counts_cost_vg).  Not a hot path: one launch per host call.
__global__ void k_cost_vg(KParams P, const float* f, float* cv_out, float* cg_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = P.N;
    if (i >= P.B * N) return;
    const int b = i / N, n = i - b * N;
    const double fx = f[(size_t)b * 2 * N + n], fy = f[(size_t)b * 2 * N + N + n];
    double cv = 0.0, ax = 0.0, ay = 0.0;
    for (int o = 0; o < P.O; ++o) {
        const double dx = fx - (double)P.obstacles[2 * o], dy = fy - (double)P.obstacles[2 * o + 1];
        const double r2 = dx * dx + dy * dy;
        const double inv = 1.0 / (0.5 + 0.5 * r2);
        cv += 0.8 * inv;
        const double i2 = inv * inv;
        ax += (-0.8 * dx) * i2;
        ay += (-0.8 * dy) * i2;
    }
    cv_out[i] = (float)cv;
    if (cg_out) {
        cg_out[(size_t)b * 2 * N + n] = (float)ax;
        cg_out[(size_t)b * 2 * N + N + n] = (float)ay;
    }
}

// trajectory.py:73-78 batched: α0 = u⊗(s·J⁻¹) + w⊗(g·J⁻¹).
__global__ void k_init_alpha(KParams P, float* alpha_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = P.N, D = P.D;
    if (e >= P.B * N * D) return;
    const int b = e / (N * D), r = e - b * N * D, n = r / D, d = r - n * D;
    float sj = 0.f, gj = 0.f;
    for (int k = 0; k < D; ++k) {
        sj += P.start[(size_t)b * D + k] * P.Jinv[k * D + d];
        gj += P.goal[(size_t)b * D + k] * P.Jinv[k * D + d];
    }
    alpha_out[e] = P.uvec[n] * sj + P.wvec[n] * gj;
}

// IK seed of an end-effector goal (irm_ik_seed, include/irm.h): damped least squares from `start`, one lane
// per problem, fp32.  kIkIters iterations of
//   e = f(q) − p,  dq = −J_eeᵀ·(J_ee·J_eeᵀ + μ²I)⁻¹·e  (μ = kIkMu, the 2×2 system in closed form),
//   dq scaled to max|dq| ≤ kIkStep,  q ← clamp(q + dq, lo, hi)
// then the residual ‖f(q) − p‖ of the returned q.  FK and Jacobian as k_fk forms them.
constexpr int kIkIters = 32;
constexpr float kIkMu = 0.1f, kIkStep = 0.5f;
template <int D>
__global__ void k_ik_seed(KParams P, const float* __restrict__ start, const float* __restrict__ goal_xy, float lo,
                          float hi, float* __restrict__ q_out, float* __restrict__ res_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const float px = goal_xy[(size_t)b * 2], py = goal_xy[(size_t)b * 2 + 1];
    float q[D], jx[D], jy[D];
#pragma unroll
    for (int d = 0; d < D; ++d) q[d] = start[(size_t)b * D + d];
    float ex = 0.f, ey = 0.f;
    // e = f(q) − p and, with `jac`, J_ee at q
    auto fk = [&](bool jac) {
        float cum = 0.f, fx = 0.f, fy = 0.f, Sx = 0.f, Sy = 0.f, xs[D], ys[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            cum += q[d];
            float sn, cs;
            sincos_fast(cum, sn, cs);
            fx = fmaf(P.link[d], cs, fx);
            fy = fmaf(P.link[d], sn, fy);
            xs[d] = -(P.link[d] * sn);
            ys[d] = P.link[d] * cs;
            Sx += xs[d];
            Sy += ys[d];
        }
        ex = fx - px;
        ey = fy - py;
        if (!jac) return;
        float Cx = 0.f, Cy = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            Cx += xs[d];
            Cy += ys[d];
            jx[d] = (xs[d] + Sx) - Cx;
            jy[d] = (ys[d] + Sy) - Cy;
        }
    };
    for (int it = 0; it < kIkIters; ++it) {
        fk(true);
        float a11 = kIkMu * kIkMu, a12 = 0.f, a22 = kIkMu * kIkMu;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            a11 = fmaf(jx[d], jx[d], a11);
            a12 = fmaf(jx[d], jy[d], a12);
            a22 = fmaf(jy[d], jy[d], a22);
        }
        // y = A⁻¹·e; det ≥ μ⁴ > 0 (A = J·Jᵀ + μ²I is positive definite)
        const float det = fmaf(a11, a22, -(a12 * a12));
        const float y0 = fmaf(a22, ex, -(a12 * ey)) / det;
        const float y1 = fmaf(a11, ey, -(a12 * ex)) / det;
        float dq[D], m = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            dq[d] = -fmaf(jx[d], y0, jy[d] * y1);
            m = fmaxf(m, fabsf(dq[d]));
        }
        const float sc = m > kIkStep ? kIkStep / m : 1.f;
#pragma unroll
        for (int d = 0; d < D; ++d) q[d] = fminf(fmaxf(fmaf(sc, dq[d], q[d]), lo), hi);
    }
    fk(false);
#pragma unroll
    for (int d = 0; d < D; ++d) q_out[(size_t)b * D + d] = q[d];
    if (res_out) res_out[b] = sqrtf(fmaf(ey, ey, ex * ex));
}

hipError_t launch_ik_seed(const KParams& p, const float* start, const float* goal_xy, float lo, float hi, float* q_out,
                          float* res_out, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        hipLaunchKernelGGL(k_ik_seed<DD>, dim3((p.B + 63) / 64), dim3(64), 0, s, p, start, goal_xy, lo, hi, q_out, res_out);
        return hipGetLastError();
    });
}

hipError_t launch_optimize(const KParams& p, hipStream_t s, LaunchDesc* desc) {
    // the dense operator (--operator-rank -1) of BASELINE configs[4]'s shape (7-DoF, N = 256): k_lean's GD
    // single loop over DenseShape (the other flows, workgroup sizes: the general kernel below)
    // (a moving launch runs k_optimize<DynShape<D>>, as a whole-robot launch does: the shape-specialised
    // kernels have no moving variant, and k_optimize has no work queue; an end-effector-goal launch, p.task,
    // and a via launch, p.via, likewise)
    if (p.v_ident && p.RP == p.NK && !p.whole_robot && !p.moving && !p.task && !p.via && p.lean_ok) {
#define IRM_TRY_DENSE(D_, N_)                                                                         \
        if (p.D == D_ && p.N == N_) {                                                                 \
            bool served = false;                                                                      \
            const hipError_t e = launch_dense_shape<DenseShape<D_, N_>>(p, s, desc, &served); \
            if (served) return e;                                                                     \
        }
        IRM_DENSE_SHAPES(IRM_TRY_DENSE)
#undef IRM_TRY_DENSE
    }
    // shape-specialised kernels for the common configurations (auto rank R = 32)
    if (p.RP == 32 && p.nsplit == stage1_splits(p.NK) && !p.whole_robot && !p.moving && !p.task && !p.via) {
#define IRM_TRY_FIX(D_, N_) \
        if (p.D == D_ && p.N == N_) return launch_optimize_shape<FixShape<D_, N_, 32>>(p, s, desc);
        IRM_FIX_SHAPES(IRM_TRY_FIX)
#undef IRM_TRY_FIX
    }
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        return launch_optimize_shape<DynShape<DD>>(p, s, desc);
    });
}

hipError_t launch_forward(const KParams& p, int mode, hipStream_t s) {
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        return launch_forward_dim<DD>(p, mode, s);
    });
}

hipError_t launch_fk(const KParams& p, const float* traj, float* pos, float* jac, hipStream_t s) {
    const int n = p.B * p.N;
    if (n <= 0) return hipSuccess;
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        hipLaunchKernelGGL(k_fk<DD>, dim3((n + 255) / 256), dim3(256), 0, s, p, traj, pos, jac);
        return hipGetLastError();
    });
}

hipError_t launch_fk_joints(const KParams& p, const float* traj, float* pos, hipStream_t s) {
    const int n = p.B * p.N;
    if (n <= 0) return hipSuccess;
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        hipLaunchKernelGGL(k_fk_joints<DD>, dim3((n + 255) / 256), dim3(256), 0, s, p, traj, pos);
        return hipGetLastError();
    });
}

hipError_t launch_cost_vg(const KParams& p, const float* f, float* cv, float* cg, hipStream_t s) {
    const int n = p.B * p.N;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_cost_vg, dim3((n + 255) / 256), dim3(256), 0, s, p, f, cv, cg);
    return hipGetLastError();
}

hipError_t launch_init_alpha(const KParams& p, float* alpha_out, hipStream_t s) {
    const int n = p.B * p.N * p.D;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_alpha, dim3((n + 255) / 256), dim3(256), 0, s, p, alpha_out);
    return hipGetLastError();
}

}  // namespace irm
