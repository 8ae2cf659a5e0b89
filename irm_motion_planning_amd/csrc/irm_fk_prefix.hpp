// irm_fk_prefix.hpp — the FK prefix the clearance kernels share: from one lane's position sample q to the sines,
// cosines and joint positions of include/irm.h's clearance block (c_l, τ_l, sn, cs, p_l), operation for operation.
// Included by irm_clearance.hip (k_clearance) and irm_self_clearance.hip (k_self_clearance); both call it with the
// whole wave converged (the choice between the two sincos forms is a ballot over the wave).
#pragma once
#include <hip/hip_runtime.h>

#include "irm_physics.hpp"  // sincos_fast, sincos_poly

namespace irm {

// c_l, sincos_fast's values (the wave-uniform choice eval_waypoint makes), fmaf-accumulated joints, with the
// rounding of every prefix addition kept (two-sum): c_l + tail_l is the angle sum to second order
template <int D>
__device__ __forceinline__ void fk_prefix(const KParams& P, const float (&q)[D], float (&sn)[D], float (&cs)[D],
                                          float (&px)[D], float (&py)[D]) {
    float cum[D], tail[D];
    bool big = false;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        if (l == 0) {
            cum[0] = q[0];
            tail[0] = 0.f;
        } else {
            const float s = cum[l - 1] + q[l];
            const float bb = s - cum[l - 1];
            const float err = (cum[l - 1] - (s - bb)) + (q[l] - bb);  // exactly (c_{l−1} + q_l) − s
            cum[l] = s;
            tail[l] = tail[l - 1] + err;
        }
        big |= fabsf(cum[l]) > 1.0e4f;
    }
    if (__builtin_expect(__ballot(big) != 0ull, 0)) {
#pragma unroll
        for (int l = 0; l < D; ++l) sincos_fast(cum[l], sn[l], cs[l]);
    } else {
#pragma unroll
        for (int l = 0; l < D; ++l) sincos_poly(cum[l], sn[l], cs[l]);
    }
    // sin / cos of c_l + tail_l to first order in the tail (|tail| ≲ 1e-6: the second order is below 1e-12)
#pragma unroll
    for (int l = 0; l < D; ++l) {
        const float s0 = sn[l], c0 = cs[l];
        sn[l] = fmaf(tail[l], c0, s0);
        cs[l] = fmaf(-tail[l], s0, c0);
    }
    float fx = 0.f, fy = 0.f;
#pragma unroll
    for (int l = 0; l < D; ++l) {
        fx = fmaf(P.link[l], cs[l], fx);
        fy = fmaf(P.link[l], sn[l], fy);
        px[l] = fx;
        py[l] = fy;
    }
}

}  // namespace irm
