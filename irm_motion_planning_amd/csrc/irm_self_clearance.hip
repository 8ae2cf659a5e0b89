// irm_self_clearance.hip — gfx950 kernel of irm_self_clearance: the signed clearance between the arm's own links
// (every pair of links that do not share a joint) on the context's evaluation times.  include/irm.h states the
// arithmetic; this file follows it operation for operation.
//
// The shape is k_clearance's: one workgroup per problem, 256 threads, one lane per evaluation time, looping over
// M in chunks; α (N×D) lies in LDS.  A lane forms q (dense_sample) and the FK prefix (fk_prefix: sines, cosines,
// joint positions, kept in registers) and then passes over the link pairs (a, b), a + 2 ≤ b, fully unrolled for the
// compile-time D (21 pairs at D = 8).  A pair is two packed-fp32 chains — the two end points of b against a, the
// two end points of a against b — each giving two point–segment distances and two orientations; the pair crosses
// iff both chains see their two points on strictly opposite sides.  The pairs, then the samples combine with
// "lower value, then lower index"; every pair also keeps its own minimum over the samples.
#include "irm_dense_sample.hpp"  // kDenseT, dense_sample, dense_stage_alpha
#include "irm_dispatch.hpp"
#include "irm_fk_prefix.hpp"  // fk_prefix
#include "irm_wave.hpp"       // wred_*, amax_step

namespace irm {

// What the launch adds to KParams (whose layout is every kernel's argument block and stays as it is).
struct SelfClearanceArgs {
    float link_radius;
    irm_self_clearance_report* rep;  // B
    float* clear;                    // B×M, nullable
    float* pair;                     // B×P, nullable
    float* joints;                   // B×M×D×2, nullable
};

__host__ __device__ constexpr int self_pairs(int D) { return D > 2 ? (D - 1) * (D - 2) / 2 : 0; }

// words per wave of the cross-wave combine: −min, index, colliding, first, crossing, then the pair minima
constexpr int kSelfRedHead = 5;
constexpr int kSelfRedW = 28;  // ≥ kSelfRedHead + self_pairs(8)
constexpr int kSelfNone = 0x7fffffff;

// The two points (x.x, y.x) and (x.y, y.y) against the segment from (ax, ay) with direction (ex, ey) and inverse
// squared length inv: their distances d and orientations o (include/irm.h: dist and orient).
__device__ __forceinline__ void self_chain(f32x2 x, f32x2 y, float ax, float ay, float ex, float ey, float inv,
                                           f32x2& d, f32x2& o) {
    const f32x2 ex2 = {ex, ex}, ey2 = {ey, ey}, ax2 = {ax, ax}, ay2 = {ay, ay}, inv2 = {inv, inv};
    const f32x2 ux = x - ax2, uy = y - ay2;
    const f32x2 dot = pkfma(uy, ey2, ux * ex2);
    f32x2 s = dot * inv2;
    s.x = fminf(fmaxf(s.x, 0.f), 1.f);
    s.y = fminf(fmaxf(s.y, 0.f), 1.f);
    const f32x2 rx = pkfma(-s, ex2, ux), ry = pkfma(-s, ey2, uy);
    const f32x2 dd = pkfma(ry, ry, rx * rx);
    d = f32x2{sqrtf(dd.x), sqrtf(dd.y)};  // IEEE square root
    o = pkfma(ux, ey2, -(uy * ex2));
}

// strictly opposite signs (a zero is not a sign)
__device__ __forceinline__ bool self_opposite(f32x2 o) { return (o.x > 0.f && o.y < 0.f) || (o.x < 0.f && o.y > 0.f); }

template <int D>
__global__ __launch_bounds__(kDenseT) void k_self_clearance(KParams P, const float* kqT, int M, SelfClearanceArgs A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NP = self_pairs(D);
    constexpr int NR = NP > 0 ? NP : 1;
    static_assert(kSelfRedHead + NP <= kSelfRedW, "the combine's record holds every pair");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    float* Al = smem;
    float* red = smem + al4(P.N * D);
    dense_stage_alpha<D>(P, b, Al);
    __syncthreads();

    const float lr2 = 2.0f * A.link_radius;

    float nbest = -INFINITY;  // −(running minimum) of this wave, with its packed (i, a, b)
    int ibest = kSelfNone;
    int ncoll = 0, ncross = 0, first = kSelfNone;
    float pmin[NR];
#pragma unroll
    for (int p = 0; p < NR; ++p) pmin[p] = INFINITY;

    for (int base = wave * 64; base < M; base += kDenseT) {  // wave-uniform
        const int i = base + lane;
        const bool live = i < M;
        const int ii = live ? i : M - 1;
        float q[D], v[D];
        dense_sample<D, false>(P, Al, kqT, nullptr, (unsigned)M, (unsigned)ii, q, v);
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
        float ex[D], ey[D], inv[D];
#pragma unroll
        for (int l = 0; l < D; ++l) {
            const float L = P.link[l];
            ex[l] = L * cs[l];
            ey[l] = L * sn[l];
            inv[l] = 1.0f / (L * L);  // IEEE division, once per link
        }
        float cmin = INFINITY;  // the sample's minimum and its a·8 + b
        int ccode = 0;
        bool coll = false, cross = false;
#pragma unroll
        for (int a = 0; a + 2 < D; ++a) {
            const float aax = a ? px[a - 1] : 0.f, aay = a ? py[a - 1] : 0.f;  // p_{a−1}
#pragma unroll
            for (int c = a + 2; c < D; ++c) {
                const int pi = a * (D - 2) - a * (a - 1) / 2 + (c - a - 2);  // the pair's place in the order
                f32x2 d12, o12, d34, o34;
                // the end points of link c against link a, the end points of link a against link c
                self_chain(f32x2{px[c - 1], px[c]}, f32x2{py[c - 1], py[c]}, aax, aay, ex[a], ey[a], inv[a], d12, o12);
                self_chain(f32x2{aax, px[a]}, f32x2{aay, py[a]}, px[c - 1], py[c - 1], ex[c], ey[c], inv[c], d34, o34);
                const bool x = self_opposite(o12) && self_opposite(o34);
                const float d = x ? 0.f : fminf(fminf(d12.x, d12.y), fminf(d34.x, d34.y));
                const float g = d - lr2;
                coll |= x || g < 0.f;
                cross |= x;
                if (live) pmin[pi] = fminf(pmin[pi], g);
                if (g < cmin) {  // pairs in ascending order: a tie keeps the lower pair
                    cmin = g;
                    ccode = a * 8 + c;
                }
            }
        }
        if (A.clear && live) A.clear[(size_t)b * M + i] = cmin;
        const unsigned long long hit = __ballot(live && coll);
        const unsigned long long xhit = __ballot(live && cross);
        if (hit) {
            ncoll += __popcll(hit);
            if (first == kSelfNone) first = base + (int)__builtin_ctzll(hit);  // chunks ascend within a wave
        }
        ncross += __popcll(xhit);
        float nv = live ? -cmin : -INFINITY;
        int ni = live ? (i << 6) | ccode : kSelfNone;
        wred_argmax(nv, ni);  // the maximum of −c_i is the minimum of c_i; ties go to the lower (i, a, b)
        amax_step(nbest, ibest, nv, ni);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) pmin[p] = wred_min(pmin[p]);
    if (lane == 0) {
        float* r = red + wave * kSelfRedW;
        r[0] = nbest;
        r[1] = __int_as_float(ibest);
        r[2] = __int_as_float(ncoll);
        r[3] = __int_as_float(first);
        r[4] = __int_as_float(ncross);
#pragma unroll
        for (int p = 0; p < NP; ++p) r[kSelfRedHead + p] = pmin[p];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int wv = 1; wv < kDenseT / 64; ++wv) {
        const float* r = red + wv * kSelfRedW;
        amax_step(nbest, ibest, r[0], __float_as_int(r[1]));
        ncoll += __float_as_int(r[2]);
        first = min(first, __float_as_int(r[3]));
        ncross += __float_as_int(r[4]);
#pragma unroll
        for (int p = 0; p < NP; ++p) pmin[p] = fminf(pmin[p], r[kSelfRedHead + p]);
    }
    const bool none = NP == 0;
    irm_self_clearance_report o;
    o.min_clearance = none ? INFINITY : -nbest;
    o.argmin_time = none ? -1 : ibest >> 6;
    o.argmin_link_a = none ? -1 : (ibest >> 3) & 7;
    o.argmin_link_b = none ? -1 : ibest & 7;
    o.n_colliding = ncoll;
    o.first_colliding = first == kSelfNone ? -1 : first;
    o.collision_free = ncoll == 0 ? 1 : 0;
    o.n_crossing = ncross;
    A.rep[b] = o;
    if (A.pair) {
#pragma unroll
        for (int p = 0; p < NP; ++p) A.pair[(size_t)b * NP + p] = pmin[p];
    }
}

static size_t self_clearance_lds(const KParams& p) {
    return (size_t)(al4(p.N * p.D) + (kDenseT / 64) * kSelfRedW) * 4;
}

hipError_t launch_self_clearance(const KParams& p, const float* kqT, int M, float link_radius,
                                 irm_self_clearance_report* rep, float* clear, float* pair, float* joints,
                                 hipStream_t s) {
    if (p.B <= 0 || M <= 0) return hipSuccess;
    const SelfClearanceArgs a = {link_radius, rep, clear, pair, joints};
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        return launch_lds(k_self_clearance<DD>, p.B, kDenseT, self_clearance_lds(p), s, p, kqT, M, a);
    });
}

}  // namespace irm
