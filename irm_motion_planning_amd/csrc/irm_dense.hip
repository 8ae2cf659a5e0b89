// irm_dense.hip — gfx950 kernels that evaluate and check trajectories at arbitrary times
// (irm_eval_any, irm_dense_check; DevBlog-Theme/blog-post.html:119-131, trajectory.py:68-70).
//
// The trajectory is the RKHS function q(t) = K(·, t)·α·J, v(t) = dK(·, t)·α·J.  The host builds the query
// matrices Kq, dKq (M×N) of the context's M evaluation times and keeps them on the device transposed
// ([N][M]).  One workgroup per problem, one lane per evaluation time, looping over M in chunks of the
// workgroup's threads: a problem's results do not depend on the rest of the batch.  α (N×D) is staged
// into LDS once per problem; every lane of a wave reads the same α element (a broadcast read) and
// consecutive floats of a query-matrix row.  The arithmetic is eval_exact's: the exact fp32×fp32
// products accumulate in fp64 in the order m = 0, 1, …, N−1, round once to fp32, then ·J the same way,
// so an evaluation on the support times is irm_evaluate's to the bit.
#include "irm_dense_sample.hpp"  // kDenseT, dense_sample, dense_stage_alpha
#include "irm_dispatch.hpp"
#include "irm_physics.hpp"  // WP, eval_waypoint_rt, stage_obstacles
#include "irm_wave.hpp"     // wred_*, amax_step

namespace irm {

// out (B×M×D) = mT's matrix · α · J (irm_eval_any: the host passes Kq or dKq).
template <int D>
__global__ __launch_bounds__(kDenseT) void k_eval_any(KParams P, const float* mT, int M, float* out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    dense_stage_alpha<D>(P, b, smem);
    __syncthreads();
    for (int base = wave * 64; base < M; base += kDenseT) {  // wave-uniform
        const int i = base + lane;
        const bool live = i < M;
        float q[D], v[D];
        dense_sample<D, false>(P, smem, mT, nullptr, (unsigned)M, (unsigned)(live ? i : M - 1), q, v);
        if (live) {
            float* o = out + ((size_t)b * M + i) * D;
#pragma unroll
            for (int k = 0; k < D; ++k) o[k] = q[k];
        }
    }
}

constexpr int kDenseRedW = 8;  // words per wave of the cross-wave combine

// irm_dense_check: q, v of every evaluation time, FK + obstacle potential on them (eval_waypoint_rt, the
// context's cost variant), the per-sample cost (optional) and the report.  Each wave reduces its 64
// samples of a chunk with the DPP trees and folds them into its running values in chunk order; the
// waves' values are combined from LDS in wave order.  Ties go to the lower index (amax_step).
// A moving launch (P.moving, irm_dense_check_moving): sample i sees the obstacle table at its own time
// t_eval[i] (P.tsup: the evaluation times on the device), from the velocity table staged behind the positions.
template <int D>
__global__ __launch_bounds__(kDenseT) void k_dense_check(KParams P, const float* kqT, const float* dkqT, int M,
                                                         irm_dense_report* rep, float* cost) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    float* Al = smem;
    float* obsL = smem + al4(P.N * D);
    float* red = obsL + (P.moving ? 2 : 1) * obs_pitch(P.O) + 4;
    const float* velL = obsL + obs_pitch(P.O);
    dense_stage_alpha<D>(P, b, Al);
    stage_obstacles<true>(P, b, 1, obsL);  // (the launch sets TB = 1, BT = kDenseT)
    __syncthreads();
    float cmax = -INFINITY, csum = 0.f, tx = -INFINITY, tn = INFINITY, va = -INFINITY;
    int cidx = 0x7fffffff, vidx = 0x7fffffff;
    for (int base = wave * 64; base < M; base += kDenseT) {  // wave-uniform
        const int i = base + lane;
        const bool live = i < M;
        float q[D], v[D];
        dense_sample<D, true>(P, Al, kqT, dkqT, (unsigned)M, (unsigned)(live ? i : M - 1), q, v);
        WP<D> w;
        eval_waypoint_rt<D>(P, q, v, obsL, w, velL, P.moving ? P.tsup[live ? i : M - 1] : 0.f);
        if (cost && live) cost[(size_t)b * M + i] = w.cv;
        float c = live ? w.cv : -INFINITY, a = live ? w.va : -INFINITY;
        int ci = live ? i : 0x7fffffff, ai = ci;
        wred_argmax(c, ci);
        wred_argmax(a, ai);
        const float s = wred_sum(live ? w.cv : 0.f);
        const float x = wred_max(live ? w.tx : -INFINITY);
        const float n = wred_min(live ? w.tn : INFINITY);
        amax_step(cmax, cidx, c, ci);
        amax_step(va, vidx, a, ai);
        csum += s;
        tx = fmaxf(tx, x);
        tn = fminf(tn, n);
    }
    if (lane == 0) {
        float* r = red + wave * kDenseRedW;
        r[0] = cmax;
        r[1] = __int_as_float(cidx);
        r[2] = csum;
        r[3] = tx;
        r[4] = tn;
        r[5] = va;
        r[6] = __int_as_float(vidx);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int wv = 1; wv < kDenseT / 64; ++wv) {
        const float* r = red + wv * kDenseRedW;
        amax_step(cmax, cidx, r[0], __float_as_int(r[1]));
        csum += r[2];
        tx = fmaxf(tx, r[3]);
        tn = fminf(tn, r[4]);
        amax_step(va, vidx, r[5], __float_as_int(r[6]));
    }
    irm_dense_report o;
    o.max_cost = cmax;
    o.avg_cost = csum / (float)M;
    o.argmax_cost = cidx;
    o.max_position = tx;
    o.min_position = tn;
    o.max_abs_velocity = va;
    o.argmax_abs_velocity = vidx;
    o.position_ok = (tx <= P.pmax && tn >= P.pmin) ? 1 : 0;  // robot.py:104-108
    o.velocity_ok = (va <= P.vmax) ? 1 : 0;                  // robot.py:111-113
    o.pad_ = 0;
    rep[b] = o;
}

static size_t dense_lds(const KParams& p, bool check) {
    int words = al4(p.N * p.D);
    if (check) words += (p.moving ? 2 : 1) * obs_pitch(p.O) + 4 + (kDenseT / 64) * kDenseRedW;
    return (size_t)words * 4;
}

hipError_t launch_eval_any(const KParams& p, const float* mT, int M, float* out, hipStream_t s) {
    if (p.B <= 0 || M <= 0) return hipSuccess;
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        return launch_lds(k_eval_any<DD>, p.B, kDenseT, dense_lds(p, false), s, p, mT, M, out);
    });
}

hipError_t launch_dense_check(const KParams& p, const float* kqT, const float* dkqT, int M, irm_dense_report* rep,
                              float* cost, hipStream_t s) {
    if (p.B <= 0 || M <= 0) return hipSuccess;
    KParams q = p;
    q.TB = 1;  // stage_obstacles: one table per workgroup, strided by kDenseT threads
    q.BT = kDenseT;
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        return launch_lds(k_dense_check<DD>, q.B, kDenseT, dense_lds(q, true), s, q, kqT, dkqT, M, rep, cost);
    });
}

}  // namespace irm
