// irm_clearance.hip — gfx950 kernel of irm_clearance: the signed clearance between the arm's links (segments
// between consecutive joints) and disc obstacles on the context's evaluation times.  include/irm.h states the
// arithmetic; this file follows it operation for operation.
//
// The shape is k_dense_check's: one workgroup per problem, 256 threads, one lane per evaluation time, looping
// over M in chunks; α (N×D) and the obstacle table (stage_obstacles' pairs, the velocity table behind it on a
// moving launch) lie in LDS, the radius table behind them.  A lane forms q (dense_sample), the FK prefix
// (c_l, sin, cos, joint positions — kept in registers across the links) and then, per link, passes over the
// obstacle pairs two obstacles per packed-fp32 instruction, carrying a running (min, pair) per packed component;
// the link's two components, the links and then the samples combine with "lower value, then lower index".
#include "irm_dense_sample.hpp"  // kDenseT, dense_sample, dense_stage_alpha
#include "irm_dispatch.hpp"
#include "irm_fk_prefix.hpp"  // fk_prefix
#include "irm_physics.hpp"    // stage_obstacles
#include "irm_wave.hpp"     // wred_*, amax_step

namespace irm {

// What the launch adds to KParams (whose layout is every kernel's argument block and stays as it is).
struct ClearanceArgs {
    const float* radius;  // obstacle radii (nullable: 0): O shared, or one table per problem at radius_stride floats
    int32_t radius_stride;
    float link_radius;
    irm_clearance_report* rep;  // B
    float* clear;               // B×M, nullable
    float* link;                // B×D, nullable
    float* joints;              // B×M×D×2, nullable
};

constexpr int kClrRedW = 12;  // words per wave of the cross-wave combine: −min, index, count, first, D link minima
constexpr int kClrNone = 0x7fffffff;

__host__ __device__ inline int clr_rad_pitch(int O) { return (O + 3) & ~3; }

template <int D>
__global__ __launch_bounds__(kDenseT) void k_clearance(KParams P, const float* kqT, int M, ClearanceArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    float* Al = smem;
    float* obsL = smem + al4(P.N * D);
    const float* velL = obsL + obs_pitch(P.O);
    float* radL = obsL + (P.moving ? 2 : 1) * obs_pitch(P.O);
    float* red = radL + clr_rad_pitch(P.O) + 4;
    dense_stage_alpha<D>(P, b, Al);
    stage_obstacles<true>(P, b, 1, obsL);  // (the launch sets TB = 1, BT = kDenseT)
    for (int e = threadIdx.x; e < clr_rad_pitch(P.O); e += kDenseT)  // padded radii: 0
        radL[e] = (A.radius && e < P.O) ? A.radius[(size_t)b * A.radius_stride + e] : 0.f;
    __syncthreads();

    const f32x4* o4 = reinterpret_cast<const f32x4*>(obsL);
    const f32x4* w4 = reinterpret_cast<const f32x4*>(velL);
    const f32x2* r2 = reinterpret_cast<const f32x2*>(radL);
    const int npair = ((P.O + 3) >> 2) * 2;
    const f32x2 lr2 = {A.link_radius, A.link_radius};

    float nbest = -INFINITY;  // −(running minimum) of this wave, with its packed (i, l, o)
    int ibest = kClrNone;
    int ncoll = 0, first = kClrNone;
    float lmin[D];
#pragma unroll
    for (int l = 0; l < D; ++l) lmin[l] = INFINITY;

    for (int base = wave * 64; base < M; base += kDenseT) {  // wave-uniform
        const int i = base + lane;
        const bool live = i < M;
        const int ii = live ? i : M - 1;
        float q[D], v[D];
        dense_sample<D, false>(P, Al, kqT, nullptr, (unsigned)M, (unsigned)ii, q, v);
        // FK prefix (irm_fk_prefix.hpp): sines, cosines and the fmaf-accumulated joints of c_l + tail_l
        float sn[D], cs[D], px[D], py[D];
        fk_prefix<D>(P, q, sn, cs, px, py);
        if (A.joints && live) {
            float* jo = A.joints + ((size_t)b * M + i) * (2 * D);
#pragma unroll
            for (int l = 0; l < D; ++l) {
                jo[2 * l] = px[l];
                jo[2 * l + 1] = py[l];
            }
        }
        const float tau = P.moving ? P.tsup[ii] : 0.f;
        const f32x2 t2 = {tau, tau};
        float cmin = INFINITY;  // the sample's minimum and its l·64 + o
        int ccode = 0;
#pragma unroll
        for (int l = 0; l < D; ++l) {
            const float L = P.link[l];
            const float ex = L * cs[l], ey = L * sn[l];
            const float inv = 1.0f / (L * L);  // IEEE division, once per link
            const float ax = l ? px[l - 1] : 0.f, ay = l ? py[l - 1] : 0.f;
            const f32x2 ex2 = {ex, ex}, ey2 = {ey, ey}, ax2 = {ax, ax}, ay2 = {ay, ay}, inv2 = {inv, inv};
            f32x2 gb = {INFINITY, INFINITY};  // running minimum of the even / odd obstacles …
            int pe = 0, po = 0;               // … and the pair that attained it
            for (int c = 0; c < npair; ++c) {
                f32x4 p = o4[c];
                if (P.moving) {
                    const f32x4 wv = w4[c];
                    p.xy = pkfma(t2, wv.xy, p.xy);
                    p.zw = pkfma(t2, wv.zw, p.zw);
                }
                const f32x2 ux = p.xy - ax2, uy = p.zw - ay2;
                const f32x2 dot = pkfma(uy, ey2, ux * ex2);
                f32x2 s = dot * inv2;
                s.x = fminf(fmaxf(s.x, 0.f), 1.f);
                s.y = fminf(fmaxf(s.y, 0.f), 1.f);
                const f32x2 rx = pkfma(-s, ex2, ux), ry = pkfma(-s, ey2, uy);
                const f32x2 dd = pkfma(ry, ry, rx * rx);
                const f32x2 d = {sqrtf(dd.x), sqrtf(dd.y)};  // IEEE square root
                const f32x2 g = (d - r2[c]) - lr2;
                if (g.x < gb.x) {
                    gb.x = g.x;
                    pe = c;
                }
                if (g.y < gb.y) {
                    gb.y = g.y;
                    po = c;
                }
            }
            // even against odd: the lower value, then the lower obstacle index
            const int oe = 2 * pe, oo = 2 * po + 1;
            const bool odd = gb.y < gb.x || (gb.y == gb.x && oo < oe);
            const float gl = odd ? gb.y : gb.x;
            const int ol = odd ? oo : oe;
            if (live) lmin[l] = fminf(lmin[l], gl);
            if (gl < cmin) {  // links in ascending order: a tie keeps the lower link
                cmin = gl;
                ccode = l * 64 + ol;
            }
        }
        if (A.clear && live) A.clear[(size_t)b * M + i] = cmin;
        const unsigned long long hit = __ballot(live && cmin < 0.f);
        if (hit) {
            ncoll += __popcll(hit);
            if (first == kClrNone) first = base + (int)__builtin_ctzll(hit);  // chunks ascend within a wave
        }
        float nv = live ? -cmin : -INFINITY;
        int ni = live ? (i << 9) | ccode : kClrNone;
        wred_argmax(nv, ni);  // the maximum of −c_i is the minimum of c_i; ties go to the lower (i, l, o)
        amax_step(nbest, ibest, nv, ni);
    }
#pragma unroll
    for (int l = 0; l < D; ++l) lmin[l] = wred_min(lmin[l]);
    if (lane == 0) {
        float* r = red + wave * kClrRedW;
        r[0] = nbest;
        r[1] = __int_as_float(ibest);
        r[2] = __int_as_float(ncoll);
        r[3] = __int_as_float(first);
#pragma unroll
        for (int l = 0; l < D; ++l) r[4 + l] = lmin[l];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int wv = 1; wv < kDenseT / 64; ++wv) {
        const float* r = red + wv * kClrRedW;
        amax_step(nbest, ibest, r[0], __float_as_int(r[1]));
        ncoll += __float_as_int(r[2]);
        first = min(first, __float_as_int(r[3]));
#pragma unroll
        for (int l = 0; l < D; ++l) lmin[l] = fminf(lmin[l], r[4 + l]);
    }
    const bool none = P.O == 0;
    irm_clearance_report o;
    o.min_clearance = none ? INFINITY : -nbest;
    o.argmin_time = none ? -1 : ibest >> 9;
    o.argmin_link = none ? -1 : (ibest >> 6) & 7;
    o.argmin_obstacle = none ? -1 : ibest & 63;
    o.n_colliding = ncoll;
    o.first_colliding = first == kClrNone ? -1 : first;
    o.collision_free = ncoll == 0 ? 1 : 0;
    o.pad_ = 0;
    A.rep[b] = o;
    if (A.link) {
#pragma unroll
        for (int l = 0; l < D; ++l) A.link[(size_t)b * D + l] = lmin[l];
    }
}

static size_t clearance_lds(const KParams& p) {
    const int words = al4(p.N * p.D) + (p.moving ? 2 : 1) * obs_pitch(p.O) + clr_rad_pitch(p.O) + 4 +
                      (kDenseT / 64) * kClrRedW;
    return (size_t)words * 4;
}

hipError_t launch_clearance(const KParams& p, const float* kqT, int M, const float* radius, int radius_stride,
                            float link_radius, irm_clearance_report* rep, float* clear, float* link, float* joints,
                            hipStream_t s) {
    if (p.B <= 0 || M <= 0) return hipSuccess;
    KParams q = p;
    q.TB = 1;  // stage_obstacles: one table per workgroup, strided by kDenseT threads
    q.BT = kDenseT;
    const ClearanceArgs a = {radius, radius_stride, link_radius, rep, clear, link, joints};
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        return launch_lds(k_clearance<DD>, q.B, kDenseT, clearance_lds(q), s, q, kqT, M, a);
    });
}

}  // namespace irm
