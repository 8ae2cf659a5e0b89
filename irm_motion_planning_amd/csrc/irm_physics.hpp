// irm_physics.hpp — what one lane computes for one waypoint: sin/cos, FK, the obstacle potential, the
// end-effector and via rows, the joint-limit penalties, their gradients, the evaluation's reductions and the
// staging of obstacles and α into LDS.  Included by irm_kernels_impl.hpp (every optimiser kernel), by
// irm_dense.hip (eval_waypoint_rt, stage_obstacles), by irm_clearance.hip (stage_obstacles), by irm_fk_prefix.hpp
// (sincos_fast / sincos_poly: the clearance kernels' FK) and by irm_kernels.hip (sincos_fast).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "irm_kernels.hpp"
#include "irm_wave.hpp"

namespace irm {

// ------------------------------------------------ per-waypoint physics
// sin/cos for robot.py's joint angles: Cody-Waite reduction by π/2 (3-part
// split, fma) and the cephes single-precision minimax polynomials on
// [−π/4, π/4]; branch-free.  Measured against double for |x| ≤ 1e4 (tests/test_physics_host.py, 1.1e8
// angles): at most 1.56 ulp of the correctly rounded result, for sin and for cos, next to odd multiples of
// π/4 (1.3 / 1.4 ulp next to multiples of π/2); asserted < 2 ulp.  |x| > 1e4 rad falls back to sincosf.
__device__ __forceinline__ void sincos_poly(float x, float& sn, float& cs) {
    // k = round(x·2/π) by the 1.5·2²³ shifter: one fma rounds the exact product to an integer (ties to
    // even), whose low bits are k's two's-complement bits in t's mantissa (|k| < 2²² here); kf = k as a
    // float.  (rintf(fl(x·2/π)) differs only where x·2/π lies within an ulp of a half-integer — then r
    // sits at ±π/4 either way, inside the polynomials' accurate range.)
    const float t = fmaf(x, 0.636619772f, 12582912.0f);
    const float kf = t - 12582912.0f;
    float r = fmaf(kf, -1.57079637050628662109375f, x);
    r = fmaf(kf, 4.371138828673793e-08f, r);
    r = fmaf(kf, 1.7151245100058819e-15f, r);
    const float z = r * r;
    const float sp = fmaf(r * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), r);
    const float cp = fmaf(z * z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f),
                          fmaf(-0.5f, z, 1.0f));
    // quadrant q = kf mod 4: swap on odd q, sin negated for q ∈ {2, 3}, cos for q ∈ {1, 2} — the sign
    // flips as bit 1 of q (resp. q + 1) moved to the sign bit (an xor; −x and the flip agree bit for bit)
    const int qi = __float_as_int(t);  // k mod 4 in the low bits
    const float s0 = (qi & 1) ? cp : sp;
    const float c0 = (qi & 1) ? sp : cp;
    sn = __uint_as_float(__float_as_uint(s0) ^ (((unsigned)qi << 30) & 0x80000000u));
    cs = __uint_as_float(__float_as_uint(c0) ^ (((unsigned)(qi + 1) << 30) & 0x80000000u));
}
__device__ __forceinline__ void sincos_fast(float x, float& sn, float& cs) {
    if (__builtin_expect(fabsf(x) > 1.0e4f, 0)) {
        sincosf(x, &sn, &cs);
        return;
    }
    sincos_poly(x, sn, cs);
}

template <int D>
struct WP {
    float cv, gx, gy;        // obstacle potential and its gradient at the end effector
    float jp, jv;            // masked joint-position / joint-velocity penalty terms (LEAN: Σ zm², Σ zvm²)
    float tx, tn, va;        // max/min joint position, max |joint velocity|
    float jx[D], jy[D];      // end-effector Jacobian row
    float fx, fy;            // end-effector position (eval_waypoint<…, POT = false>: potential not yet added)
    float zm[D], zvm[D];     // LEAN: masked (q − μ)/σ_q and v/v_max (0 where the limit mask is off)
};

// End-effector goal (P.task, include/irm.h): what the end row's terms need of a waypoint's evaluation — the
// end-effector position f the evaluation itself formed and the end effector's Jacobian J_ee (with WHOLE,
// WP::jx holds the whole-robot gradient instead).
template <int D>
struct EE {
    float fx, fy;
    float jx[D], jy[D];
};

// The end row's terms of an end-effector goal from its evaluation, in the fp32 order include/irm.h defines:
//   e = f − p,  r² = fmaf(e_y, e_y, e_x·e_x),  ge[d] = fmaf(J_y[d], e_y, J_x[d]·e_x)  (= J_eeᵀ·e)
// r² takes the place of ‖T[N−1] − g‖² (loss, constraint) and ge that of T[N−1] − g (gradient input a).
template <int D>
__device__ __forceinline__ void task_end_row(const EE<D>& ee, float px, float py, float (&ge)[D], float& r2) {
    const float ex = ee.fx - px, ey = ee.fy - py;
    r2 = fmaf(ey, ey, ex * ex);
#pragma unroll
    for (int d = 0; d < D; ++d) ge[d] = fmaf(ee.jy[d], ey, ee.jx[d] * ex);
}

// Via-points (P.via, include/irm.h): the via-point this lane's row n carries — −1 none, else v + 4·cartesian[v]
// (rows are strictly increasing: at most one matches).  Unrolled over the table, so every read of the
// kernel-argument arrays has a constant index.
__device__ __forceinline__ int via_code(const KParams& P, int n) {
    int code = -1;
#pragma unroll
    for (int i = 0; i < IRM_MAX_VIA; ++i)
        if (i < P.n_via && n == P.via_row[i]) code = i + 4 * (P.via_cart[i] != 0 ? 1 : 0);
    return code;
}
// The via row's terms (r², ge) of via-point `code` of problem b from the row's waypoint q and its evaluation's
// ee, in the fp32 order include/irm.h defines.  FMA: the joint distance accumulates as the calling kernel
// accumulates row N−1 against the joint goal — fmaf(e, e, a) in k_optimize, a += e·e in k_forward.
template <int D, bool FMA>
__device__ __forceinline__ void via_row_terms(const KParams& P, size_t b, int code, const float (&q)[D],
                                              const EE<D>& ee, float (&ge)[D], float& r2) {
    const float* c = P.via_target + (b * (size_t)P.n_via + (size_t)(code & 3)) * D;
    if (code & 4) {
        if constexpr (D >= 2) task_end_row<D>(ee, c[0], c[1], ge, r2);  // (D = 1: refused by the host)
        return;
    }
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float e = q[d] - c[d];
        ge[d] = e;
        if constexpr (FMA) a = fmaf(e, e, a);
        else a += e * e;
    }
    r2 = a;
}

// robot.py:29-36 (fk), 75-87 (jacobian); environment.py:46-58
// (compute_cost_vg); trajectory.py:215-227, 245-255 (penalty elements).
// WHOLE: the potential is summed over every joint position p_j = fk_joint_j
// (robot.py:39-72; DevBlog-Theme/blog-post.html:491-498) instead of the end
// effector only.  Its gradient w.r.t. angle k is Σ_{l≥k} (X_l·GX_l + Y_l·GY_l)
// with (X_l, Y_l) = L_l·(−sin c_l, cos c_l) and GX_l = Σ_{j≥l} ∂cost/∂p_j; it is
// returned as w.jx (with w.gx = 1, w.jy = w.gy = 0) so grad_waypoint is shared.
// POT = false (end-effector cost only): everything but the obstacle potential, whose inputs are left
// in w.fx / w.fy (potential_pair evaluates two waypoints' potentials in one pass over the obstacles).
// LEAN evaluations keep zm / zvm for the gradient inputs where kLeanKeep<D> (irm_layout.hpp); elsewhere the
// gradient inputs recompute them (lean_pen: the same arithmetic, the same values)
template <int D>
__device__ __forceinline__ void lean_pen(const KParams& P, const float (&q)[D], const float (&v)[D], float (&zm)[D],
                                         float (&zvm)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float z = (q[d] - P.mean_pos) * P.inv_std_pos;
        const bool m = (q[d] > P.thr_hi) || (q[d] < P.thr_lo);
        const float zv = v[d] * P.inv_vmax;
        const bool mv = fabsf(v[d]) > P.thr_v;
        zm[d] = m ? z : 0.f;  // (cvdl off: the host's thresholds make every mask true)
        zvm[d] = mv ? zv : 0.f;
    }
}

// LEAN (the optimiser kernels): the penalty terms in the form the loss and the gradient inputs share —
// zm = mask·(q − μ)/σ_q and zvm = mask·v/v_max per joint, w.jp = Σ zm², w.jv = Σ zvm² (the ½ and the
// 1/N of trajectory.py:215-227, 245-255 go into the per-trajectory weights, grad_waypoint_lean); the
// host-API kernels keep the reference's element order (½·z² per element, summed).
// MOVING: every obstacle drifts at a constant velocity over the plan; the lane's waypoint lies at plan time
// tau and sees obstacle o at fmaf(tau, w_o, p_o) per coordinate — one packed FMA per coordinate pair of an
// obstacle pair, from the velocity table `vel` (LDS, stage_obstacles' layout; sentinel velocity 0, so the
// padding stays at 1e20 and adds exactly 0).  From there on the arithmetic is the static one's; a zero
// velocity gives the static result to the bit (fmaf(tau, 0, p) = p).
// TASK: *ee receives f and J_ee as formed here (no second FK); nothing else changes.
template <int D, bool WHOLE = false, bool POT = true, bool LEAN = false, bool MOVING = false, bool TASK = false>
__device__ __forceinline__ void eval_waypoint(const KParams& P, const float (&q)[D], const float (&v)[D],
                                              const float* __restrict__ ob, WP<D>& w,
                                              const f32x4* oreg = nullptr,  // oreg: the 12-obstacle
                                                                            // table held in VGPRs
                                              const float* __restrict__ vel = nullptr, float tau = 0.f,
                                              EE<D>* ee = nullptr) {
    float fx = 0.f, fy = 0.f, Sx = 0.f, Sy = 0.f;
    float xs[D], ys[D], px[D], py[D], cum[D], snv[D], csv[D];
    bool big = false;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        cum[d] = d ? cum[d - 1] + q[d] : q[d];
        big |= fabsf(cum[d]) > 1.0e4f;
    }
    // One wave-uniform branch for all joints: the D polynomial chains share a basic block (the
    // scheduler interleaves them); a wave with any |angle| > 1e4 takes the per-lane form, whose
    // small-angle lanes compute the same polynomial, so every lane's value is that of sincos_fast.
    if (__builtin_expect(__ballot(big) != 0ull, 0)) {
#pragma unroll
        for (int d = 0; d < D; ++d) sincos_fast(cum[d], snv[d], csv[d]);
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) sincos_poly(cum[d], snv[d], csv[d]);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float sn = snv[d], cs = csv[d];
        fx = fmaf(P.link[d], cs, fx);
        fy = fmaf(P.link[d], sn, fy);
        px[d] = fx;
        py[d] = fy;
        xs[d] = -(P.link[d] * sn);
        ys[d] = P.link[d] * cs;
        Sx = d ? Sx + xs[d] : xs[d];
        Sy = d ? Sy + ys[d] : ys[d];
    }
    // Obstacles are staged in LDS in pairs (x_a, x_b, y_a, y_b), padded to a multiple of 4
    // with sentinels at (1e20, 1e20): r² overflows to +inf, rcp → 0, so a sentinel adds
    // exactly 0.  Two obstacles per packed-fp32 instruction; the even- and odd-numbered
    // obstacles accumulate separately and are added at the end.
    const f32x4* o4 = reinterpret_cast<const f32x4*>(ob);
    const int nq = (P.O + 3) >> 2;
    // obstacle pair i (x_a, x_b, y_a, y_b) at this lane's time
    auto pair_at = [&](int i) -> f32x4 {
        f32x4 p = o4[i];
        if constexpr (MOVING) {
            const f32x4 wv = reinterpret_cast<const f32x4*>(vel)[i];
            const f32x2 t2 = {tau, tau};
            p.xy = pkfma(t2, wv.xy, p.xy);
            p.zw = pkfma(t2, wv.zw, p.zw);
        }
        return p;
    };
    // Per pair of obstacles: e = 1 + dx² + dy² (= 2·den), u = rcp(e); the potential's constants are
    // applied once at the end: cost = 0.8/den = 1.6·Σu, ∂cost/∂f = −0.8·d/den² = −3.2·Σ d·u².
    auto potential = [&](float x, float y, float& cv, float& ax, float& ay) {
        f32x2 cv2 = {0.f, 0.f}, ax2 = {0.f, 0.f}, ay2 = {0.f, 0.f};
        const f32x2 fx2 = {x, x}, fy2 = {y, y}, one = {1.f, 1.f};
        auto pair2 = [&](f32x2 ox, f32x2 oy) {
            const f32x2 dx = fx2 - ox, dy = fy2 - oy;
            const f32x2 e = pkfma(dy, dy, pkfma(dx, dx, one));
            const f32x2 u = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
            cv2 += u;
            const f32x2 u2 = u * u;
            ax2 = pkfma(dx, u2, ax2);
            ay2 = pkfma(dy, u2, ay2);
        };
        if (nq == 3) {  // 9-12 obstacles (the reference's 11): one straight-line block, all 12 rcps
                        // issued back to back, then the sums in pair2's order
            f32x2 dx[6], dy[6], u[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                f32x4 p;
                if constexpr (MOVING) p = pair_at(i);
                else p = oreg ? oreg[i] : o4[i];
                dx[i] = fx2 - p.xy;
                dy[i] = fy2 - p.zw;
                const f32x2 e = pkfma(dy[i], dy[i], pkfma(dx[i], dx[i], one));
                u[i] = f32x2{__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
            }
            // (the sums start from the first pair, not from +0: the same values, two instructions fewer)
            cv2 = u[0];
            ax2 = dx[0] * (u[0] * u[0]);
            ay2 = dy[0] * (u[0] * u[0]);
#pragma unroll
            for (int i = 1; i < 6; ++i) {
                cv2 += u[i];
                const f32x2 u2 = u[i] * u[i];
                ax2 = pkfma(dx[i], u2, ax2);
                ay2 = pkfma(dy[i], u2, ay2);
            }
        } else {
            for (int c = 0; c < nq; ++c) {
                f32x4 p0, p1;
                if constexpr (MOVING) {
                    p0 = pair_at(2 * c);
                    p1 = pair_at(2 * c + 1);
                } else {
                    p0 = o4[2 * c];
                    p1 = o4[2 * c + 1];
                }
                pair2(p0.xy, p0.zw);
                pair2(p1.xy, p1.zw);
            }
        }
        cv = 1.6f * (cv2.x + cv2.y);
        ax = -3.2f * (ax2.x + ax2.y);
        ay = -3.2f * (ay2.x + ay2.y);
    };
    if constexpr (TASK) {
        ee->fx = fx;
        ee->fy = fy;
    }
    if constexpr (!WHOLE) {
        float Cx = 0.f, Cy = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            Cx = d ? Cx + xs[d] : xs[d];
            Cy = d ? Cy + ys[d] : ys[d];
            w.jx[d] = (xs[d] + Sx) - Cx;
            w.jy[d] = (ys[d] + Sy) - Cy;
            if constexpr (TASK) {
                ee->jx[d] = w.jx[d];
                ee->jy[d] = w.jy[d];
            }
        }
        if constexpr (POT) {
            potential(fx, fy, w.cv, w.gx, w.gy);
        } else {
            w.fx = fx;
            w.fy = fy;
        }
    } else {
        if constexpr (TASK) {  // J_ee in the order of the end-effector variant above
            float Cx = 0.f, Cy = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                Cx = d ? Cx + xs[d] : xs[d];
                Cy = d ? Cy + ys[d] : ys[d];
                ee->jx[d] = (xs[d] + Sx) - Cx;
                ee->jy[d] = (ys[d] + Sy) - Cy;
            }
        }
        float cvt = 0.f, gxj[D], gyj[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            float cvj;
            potential(px[j], py[j], cvj, gxj[j], gyj[j]);
            cvt += cvj;
        }
        float GX = 0.f, GY = 0.f, acc = 0.f;
#pragma unroll
        for (int l = D - 1; l >= 0; --l) {
            GX += gxj[l];
            GY += gyj[l];
            acc = fmaf(xs[l], GX, fmaf(ys[l], GY, acc));
            w.jx[l] = acc;
            w.jy[l] = 0.f;
        }
        w.cv = cvt;
        w.gx = 1.f;
        w.gy = 0.f;
    }
    float jp = 0.f, jv = 0.f, tx = -INFINITY, tn = INFINITY, va = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float z = (q[d] - P.mean_pos) * P.inv_std_pos;
        const bool m = (q[d] > P.thr_hi) || (q[d] < P.thr_lo);
        const float zv = v[d] * P.inv_vmax;
        const bool mv = fabsf(v[d]) > P.thr_v;
        if constexpr (LEAN) {
            const float zm = m ? z : 0.f, zvm = mv ? zv : 0.f;  // (cvdl: folded into the thresholds)
            if constexpr (kLeanKeep<D>) {
                w.zm[d] = zm;
                w.zvm[d] = zvm;
            }
            jp = fmaf(zm, zm, jp);
            jv = fmaf(zvm, zvm, jv);
        } else {
            jp += m ? 0.5f * (z * z) : 0.f;
            jv += mv ? 0.5f * (zv * zv) : 0.f;
        }
        tx = fmaxf(tx, q[d]);
        tn = fminf(tn, q[d]);
        va = fmaxf(va, fabsf(v[d]));
    }
    w.jp = jp;
    w.jv = jv;
    w.tx = tx;
    w.tn = tn;
    w.va = va;
}

// The obstacle potential of two waypoints (w0.fx/fy, w1.fx/fy) in one pass over the LDS obstacle table:
// each obstacle pair is loaded once and both waypoints' terms are formed from it (independent chains
// that interleave).  Per waypoint the arithmetic and the accumulation order are eval_waypoint's.
template <int D>
__device__ __forceinline__ void potential_pair(const KParams& P, const float* __restrict__ ob, WP<D>& w0, WP<D>& w1) {
    const f32x4* o4 = reinterpret_cast<const f32x4*>(ob);
    const int nq = (P.O + 3) >> 2;
    f32x2 cv0 = {0.f, 0.f}, ax0 = {0.f, 0.f}, ay0 = {0.f, 0.f}, cv1 = cv0, ax1 = cv0, ay1 = cv0;
    const f32x2 x0 = {w0.fx, w0.fx}, y0 = {w0.fy, w0.fy}, x1 = {w1.fx, w1.fx}, y1 = {w1.fy, w1.fy};
    const f32x2 one = {1.f, 1.f};
    auto pair2 = [&](const f32x2& fx2, const f32x2& fy2, f32x2 ox, f32x2 oy, f32x2& cv2, f32x2& ax2, f32x2& ay2) {
        const f32x2 dx = fx2 - ox, dy = fy2 - oy;
        const f32x2 e = pkfma(dy, dy, pkfma(dx, dx, one));
        const f32x2 u = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
        cv2 += u;
        const f32x2 u2 = u * u;
        ax2 = pkfma(dx, u2, ax2);
        ay2 = pkfma(dy, u2, ay2);
    };
    for (int c = 0; c < nq; ++c) {
        const f32x4 p0 = o4[2 * c], p1 = o4[2 * c + 1];
        pair2(x0, y0, p0.xy, p0.zw, cv0, ax0, ay0);
        pair2(x1, y1, p0.xy, p0.zw, cv1, ax1, ay1);
        pair2(x0, y0, p1.xy, p1.zw, cv0, ax0, ay0);
        pair2(x1, y1, p1.xy, p1.zw, cv1, ax1, ay1);
    }
    w0.cv = 1.6f * (cv0.x + cv0.y);
    w0.gx = -3.2f * (ax0.x + ax0.y);
    w0.gy = -3.2f * (ay0.x + ay0.y);
    w1.cv = 1.6f * (cv1.x + cv1.y);
    w1.gx = -3.2f * (ax1.x + ax1.y);
    w1.gy = -3.2f * (ay1.x + ay1.y);
}

// eval_waypoint with the cost variant chosen at run time (host-API kernels, DynShape optimiser).
// vel / tau: the moving variant (P.moving; vel the LDS velocity table behind ob's, tau the lane's time)
// TASK: *ee receives f and J_ee (eval_waypoint; the caller decides at run time whether it uses them)
template <int D, bool TASK = false>
__device__ __forceinline__ void eval_waypoint_rt(const KParams& P, const float (&q)[D], const float (&v)[D],
                                                 const float* __restrict__ ob, WP<D>& w,
                                                 const float* __restrict__ vel = nullptr, float tau = 0.f,
                                                 EE<D>* ee = nullptr) {
    if (P.moving) {
        if (P.whole_robot) eval_waypoint<D, true, true, false, true, TASK>(P, q, v, ob, w, nullptr, vel, tau, ee);
        else eval_waypoint<D, false, true, false, true, TASK>(P, q, v, ob, w, nullptr, vel, tau, ee);
        return;
    }
    if (P.whole_robot) eval_waypoint<D, true, true, false, false, TASK>(P, q, v, ob, w, nullptr, nullptr, 0.f, ee);
    else eval_waypoint<D, false, true, false, false, TASK>(P, q, v, ob, w, nullptr, nullptr, 0.f, ee);
}

// Gradient inputs a (→ Kᵀ) and b (→ dKᵀ) of one waypoint, trajectory.py:91-126
// (obstacle), 191-212 (start/goal), 231-242 / 259-268 (joint limits).
// task_row: this lane is row N−1 of an end-effector-goal call and g holds ge = J_eeᵀ·(f − p)
// (task_end_row), which takes the place of q − g.
template <int D>
__device__ __forceinline__ void grad_waypoint(const KParams& P, const WP<D>& w, const float (&q)[D],
                                              const float (&v)[D], int n, int idx, float lsg, float ljl,
                                              const float (&s)[D], const float (&g)[D], float (&a)[D],
                                              float (&b)[D], bool task_row = false, bool via_row = false) {
    // via_row: this lane's row (in 1 … N−2) carries a via-point and g holds its ge (via_row_terms); the position
    // term only — a via row's velocity is free
    const int N = P.N;
    const float wt = (n == idx ? P.lam_max : 0.f) + P.one_m_lmax * P.invN;
    const float wx = wt * w.gx, wy = wt * w.gy;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float sgp = 0.f, sgv = 0.f;
        if (n == 0) {
            sgp = q[d] - s[d];
            sgv = v[d];
        }
        if (n == N - 1) {
            sgp = task_row ? g[d] : q[d] - g[d];
            sgv = v[d];
        }
        if (via_row) sgp = g[d];
        float jpg = 0.f, jvg = 0.f;
        const bool m = (q[d] > P.thr_hi) || (q[d] < P.thr_lo);
        if (m) jpg = ((q[d] - P.mean_pos) * P.inv_std2) * P.invN;
        const bool mv = fabsf(v[d]) > P.thr_v;
        if (mv) jvg = (v[d] * P.inv_vmax2) * P.invN;
        a[d] = fmaf(ljl, jpg, fmaf(lsg, sgp, fmaf(wx, w.jx[d], wy * w.jy[d])));
        b[d] = fmaf(lsg, sgv, ljl * jvg);
    }
}

// Per-trajectory weights of the LEAN evaluation (uniform; ljl changes with the outer iteration):
// the loss's mean / penalty terms u = c_mean·cv + c_pen·(Σzm² + Σzvm²) (trajectory.py:85-87, 281 with
// ½ and 1/N folded), the gradient's penalty slopes k_pos = λjl/(σ_q·N), k_vel = λjl/(v_max·N)
// (trajectory.py:231-242, 259-268: (q − μ)/σ_q²/N = zm·(1/σ_q)/N).
struct LeanW {
    float c_mean, c_pen, k_pos, k_vel;
};
__device__ __forceinline__ LeanW lean_weights(const KParams& P, float ljl) {
    LeanW c;
    c.c_mean = P.one_m_lmax * P.invN;
    c.c_pen = (0.5f * ljl) * P.invN;
    c.k_pos = (ljl * P.inv_std_pos) * P.invN;
    c.k_vel = (ljl * P.inv_vmax) * P.invN;
    return c;
}

// Gradient inputs a, b of one waypoint from a LEAN evaluation (grad_waypoint's terms, the penalty
// masks and normalised deviations reused from the evaluation).  lsg_ep = λsg on rows 0 and N−1, else
// 0 (per lane); tg the row's start / goal.
// TASK (k_optimize<DynShape<D>>): on the lane with task_row — row N−1 of an end-effector-goal launch — tg
// holds ge = J_eeᵀ·(f − p) (task_end_row), which takes the place of q − tg.  lsg_pos: the weight of the position
// term — lsg_ep on every row but a via row (via_row_terms: task_row set, tg its ge), where it is λsg while
// lsg_ep, which also weighs v[d], stays 0: a via row's velocity is free.
template <int D, bool TASK = false>
__device__ __forceinline__ void grad_waypoint_lean(const KParams& P, const WP<D>& w, const float (&q)[D],
                                                   const float (&v)[D], bool isidx, float lsg_ep,
                                                   const LeanW& c, const float (&tg)[D], float (&a)[D],
                                                   float (&b)[D], bool task_row = false, float lsg_pos = 0.f) {
    const float wt = (isidx ? P.lam_max : 0.f) + c.c_mean;
    const float wx = wt * w.gx, wy = wt * w.gy;
    float zm[D], zvm[D];
    if constexpr (kLeanKeep<D>) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            zm[d] = w.zm[d];
            zvm[d] = w.zvm[d];
        }
    } else {
        lean_pen<D>(P, q, v, zm, zvm);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float sgp = q[d] - tg[d];
        float lp = lsg_ep;
        if constexpr (TASK) {
            sgp = task_row ? tg[d] : sgp;
            lp = lsg_pos;
        }
        a[d] = fmaf(c.k_pos, zm[d], fmaf(lp, sgp, fmaf(wx, w.jx[d], wy * w.jy[d])));
        b[d] = fmaf(lsg_ep, v[d], c.k_vel * zvm[d]);
    }
}

// Result of one cost evaluation of one trajectory (reduced over waypoints).
struct EvalOut {
    float loss, ds, dg, vs, vg, tmax, tmin, vabs;
    int idx;
};

// Wave-reduce this lane's waypoint terms; lane 0 of each wave stores the
// partials, the lanes of rows 0 / N−1 store the start/goal terms.  Must be
// reached by the whole wave (a wave never straddles two trajectories).
// kRedW: words per wave of `red`, the eight partials — plan_head gives the region kMaxWaves·8 words and `sg`
// follows it directly, so a wider stride would put the partials of a 1024-thread workgroup's last waves onto
// the start/goal words (four N = 256 or two N = 512 trajectories in one workgroup).
constexpr int kRedW = 8;
template <int D>
__device__ __forceinline__ void eval_partials(const KParams& P, bool live, const WP<D>& w, int n, int wave,
                                              const float (&q)[D], const float (&v)[D], const float (&s)[D],
                                              const float (&g)[D], float* red, float* sg, int t,
                                              bool task_row = false, float r2 = 0.f) {  // task_row: row N−1 of
                                              // an end-effector-goal call stores r² = ‖f − p‖² (task_end_row)
    float cmax = live ? w.cv : -INFINITY;
    int cidx = live ? n : 0x7fffffff;
    wred_argmax(cmax, cidx);
    const float csum = wred_sum(live ? w.cv : 0.f);
    const float jps = wred_sum(live ? w.jp : 0.f);
    const float jvs = wred_sum(live ? w.jv : 0.f);
    const float tx = wred_max(live ? w.tx : -INFINITY);
    const float tn = wred_min(live ? w.tn : INFINITY);
    const float va = wred_max(live ? w.va : 0.f);
    if ((threadIdx.x & 63) == 0) {
        float* r = red + wave * kRedW;
        r[0] = cmax;
        r[1] = __int_as_float(cidx);
        r[2] = csum;
        r[3] = jps;
        r[4] = jvs;
        r[5] = tx;
        r[6] = tn;
        r[7] = va;
    }
    if (live && (n == 0 || n == P.N - 1)) {  // trajectory.py:183-204 rows 0 and N−1
        float a = 0.f, bb = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float e = q[d] - (n == 0 ? s[d] : g[d]);
            a += e * e;
            bb += v[d] * v[d];
        }
        if (task_row) a = r2;
        sg[t * 4 + (n == 0 ? 0 : 2)] = a;
        sg[t * 4 + (n == 0 ? 1 : 3)] = bb;
    }
}

// Combine the trajectory's wave partials (fixed order) into loss + stats.
// viaw / nvia: the trajectory's via words r_v² (a via launch), which join the start/goal position sum in index
// order after its two terms (include/irm.h).
__device__ __forceinline__ EvalOut eval_finalize(const KParams& P, const float* red, const float* sg, int t,
                                                 int wave0, int nwt, float lsg, float ljl,
                                                 const float* viaw = nullptr, int nvia = 0) {
    const float* r = red + wave0 * kRedW;
    float cmax = r[0];
    int cidx = __float_as_int(r[1]);
    float csum = r[2], jps = r[3], jvs = r[4], tx = r[5], tn = r[6], va = r[7];
    for (int w = 1; w < nwt; ++w) {
        const float* q = red + (wave0 + w) * kRedW;
        amax_step(cmax, cidx, q[0], __float_as_int(q[1]));
        csum += q[2];
        jps += q[3];
        jvs += q[4];
        tx = fmaxf(tx, q[5]);
        tn = fminf(tn, q[6]);
        va = fmaxf(va, q[7]);
    }
    const float a0 = sg[t * 4 + 0], b0 = sg[t * 4 + 1], a1 = sg[t * 4 + 2], b1 = sg[t * 4 + 3];
    const float nN = (float)P.N;
    float sgpc = 0.5f * a0 + 0.5f * a1;                                // trajectory.py:187
    for (int i = 0; i < nvia; ++i) sgpc = sgpc + 0.5f * viaw[t * IRM_MAX_VIA + i];
    const float sgvc = 0.5f * b0 + 0.5f * b1;                          // trajectory.py:203
    const float toc = P.lam_max * cmax + P.one_m_lmax * (csum / nN);    // trajectory.py:85-87
    EvalOut e;
    e.loss = toc + lsg * (sgpc + sgvc) + ljl * (jps / nN + jvs / nN);  // trajectory.py:281
    e.idx = cidx;
    e.ds = sqrtf(a0);
    e.dg = sqrtf(a1);
    e.vs = sqrtf(b0);
    e.vg = sqrtf(b1);
    e.tmax = tx;
    e.tmin = tn;
    e.vabs = va;
    return e;
}

// Obstacles into LDS: one shared set (obs_stride 0) or one per trajectory,
// each padded to obs_pitch floats with zero-contribution sentinels.
__host__ __device__ inline int obs_pitch(int O) { return ((O + 3) & ~3) * 2; }
// MOVING (the kernels that have the moving variant): a moving launch (P.moving) stages the velocity table
// behind the positions (obs_vel_offset), in the same layout and from the same shared / per-problem indexing,
// sentinels at velocity 0.
__host__ __device__ inline int obs_vel_offset(const KParams& P) { return (P.obs_stride ? P.TB : 1) * obs_pitch(P.O); }
template <bool MOVING = false>
__device__ inline void stage_obstacles(const KParams& P, int tb0, int ntb, float* obsL) {
    const int pitch = obs_pitch(P.O), nsets = P.obs_stride ? P.TB : 1;
    for (int e = threadIdx.x; e < nsets * pitch; e += P.BT) {
        const int tt = e / pitch, r = e - tt * pitch;
        // r = 4·pair + 2·coord + j  →  obstacle 2·pair + j, coordinate coord
        const int o = 2 * (r >> 2) + (r & 1), coord = (r >> 1) & 1;
        float val = 1.0e20f;
        if (o < P.O) {
            const int src = 2 * o + coord;
            if (!P.obs_stride) val = P.obstacles[src];
            else if (tt < ntb) val = P.obstacles[(size_t)(tb0 + tt) * P.obs_stride + src];
        }
        obsL[e] = val;
    }
    if constexpr (!MOVING) return;
    if (!P.moving) return;
    float* velL = obsL + nsets * pitch;
    for (int e = threadIdx.x; e < nsets * pitch; e += P.BT) {
        const int tt = e / pitch, r = e - tt * pitch;
        const int o = 2 * (r >> 2) + (r & 1), coord = (r >> 1) & 1;
        float val = 0.f;
        if (o < P.O) {
            const int src = 2 * o + coord;
            if (!P.obs_stride) val = P.obs_vel[src];
            else if (tt < ntb) val = P.obs_vel[(size_t)(tb0 + tt) * P.obs_stride + src];
        }
        velL[e] = val;
    }
}

// α0 of the block's trajectories into X[n][tD+d] (rows ≥ N / unused columns 0).
template <int D>
__device__ void stage_alpha(const KParams& P, int tb0, int ntb, float* X, int xrows) {
    const int N = P.N;
    for (int e = threadIdx.x; e < xrows * 16; e += P.BT) {
        const int n = e >> 4, c = e & 15, t = c / D, d = c - t * D;
        float* dst = X + n * kLd + c;
        float val = 0.f;
        if (n < N && t < ntb) {
            const size_t b = (size_t)(tb0 + t);
            if (P.alpha0) {
                val = P.alpha0[(b * N + n) * D + d];
            } else {  // trajectory.py:73-78 via K⁻¹(1−c), K⁻¹c (linearity of solve)
                float sj = 0.f, gj = 0.f;
                for (int e2 = 0; e2 < D; ++e2) {
                    sj += P.start[b * D + e2] * P.Jinv[e2 * D + d];
                    gj += P.goal[b * D + e2] * P.Jinv[e2 * D + d];
                }
                val = P.uvec[n] * sj + P.wvec[n] * gj;
            }
        }
        *dst = val;
    }
}

}  // namespace irm
