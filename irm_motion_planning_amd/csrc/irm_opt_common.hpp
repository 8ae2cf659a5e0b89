// irm_opt_common.hpp — what both optimiser kernels share: the evaluation's wave reduction (ered_store), the
// reference's fp32 α update with its rounding residual (alpha_step*), the IEEE quotient in three VALU
// (rcp_refined, div_rcp, rcp_rn_of), ld_frag and the problem shapes (FixShape, DenseShape, DynShape).
// Included by irm_kernels_impl.hpp, irm_lean_plan.hpp and by irm_kernels.hip (the shapes it dispatches on).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "irm_kernels.hpp"
#include "irm_wave.hpp"

namespace irm {

// ------------------------------------------------------------ optimiser
// Wave reduction of one evaluation's per-waypoint terms.
// usum: Σ_n [(1−λmax)/N·cost_v[n] + λjl/N·(jp[n] + jv[n])], the mean-obstacle and
// joint-limit terms of trajectory.py:281 folded into one sum; cmax with the
// first-index argmax of jnp.argmax (trajectory.py:97) from a ballot of the lanes
// holding the wave maximum.  tx/tn/va (constraint extrema) only when `ext`.
// Lane 0 stores the wave's record at red[wave·8].
__device__ __forceinline__ void ered_store(bool live, float cv, float us, float tx, float tn, float va, bool ext,
                                           int n0, float* red, int wave) {
    float m = live ? cv : -INFINITY, s = live ? us : 0.f;  // cv ≥ +0 (a sum of reciprocals): maxpos
    m = maxpos(m, dppf<0xB1>(m));
    s += dppf<0xB1>(s);
    m = maxpos(m, dppf<0x4E>(m));
    s += dppf<0x4E>(s);
    m = maxpos(m, dppf<0x141>(m));
    s += dppf<0x141>(s);
    m = maxpos(m, dppf<0x140>(m));
    s += dppf<0x140>(s);
    // cross-row combine with the GFX9 row broadcasts: row_bcast:15 into rows 1 and 3, row_bcast:31 into
    // rows 2 and 3, so lane 63 holds (r3 ∘ r2) ∘ (r1 ∘ r0) — the association of the readlane form
    // (lanes 0, 16, 32, 48), fp addition being commutative; read back as a wave-uniform value
    float wm, ws;
    {
        m = maxpos(m, __int_as_float(__builtin_amdgcn_update_dpp((int)0x80000000, __float_as_int(m), 0x142, 0xA, 0xF, false)));
        s = bcast_add<15>(s);
        m = maxpos(m, __int_as_float(__builtin_amdgcn_update_dpp((int)0x80000000, __float_as_int(m), 0x143, 0xC, 0xF, false)));
        s = bcast_add<31>(s);
        wm = lanef(m, 63);
        ws = lanef(s, 63);
    }
    const unsigned long long hit = __ballot(live && cv == wm);
    const int idx = hit ? n0 + __builtin_ctzll(hit) : 0x7fffffff;
    float ox = 0.f, on = 0.f, oa = 0.f;
    if (ext) {
        ox = wred_max(live ? tx : -INFINITY);
        on = wred_min(live ? tn : INFINITY);
        oa = wred_max(live ? va : 0.f);
    }
    if ((threadIdx.x & 63) == 0) {
        float* q = red + wave * 8;
        q[0] = wm;
        q[1] = __int_as_float(idx);
        q[2] = ws;
        q[3] = ox;
        q[4] = on;
        q[5] = oa;
    }
}

// A value the compiler may not fuse into a neighbouring operation (hipcc contracts a·b − c into
// an fma even under `#pragma clang fp contract(off)` when the product comes from __fmul_rn).
__device__ __forceinline__ float unfused(float x) {
    asm("" : "+v"(x));
    return x;
}

// a/b through a reciprocal refined by one Newton step (r = rcp_refined(b)): q = a·r, then q + (a − q·b)·r —
// the correctly rounded quotient but in rare near-ties, in 3 VALU per quotient once r is known (the IEEE
// division expands to ~10 with its scaling and fix-up).  The BLS trial stages form ĝ = G/‖G‖ with it
// (optimizer_BLS.py:165); its operands are normal numbers there.
__device__ __forceinline__ float rcp_refined(float b) {
    const float r0 = __builtin_amdgcn_rcpf(b);
    return fmaf(fmaf(-b, r0, 1.f), r0, r0);
}
__device__ __forceinline__ float div_rcp(float a, float b, float r) {
    const float q = a * r;
    return fmaf(fmaf(-q, b, a), r, q);
}
// The IEEE quotient a/b in div_rcp's 3 VALU (round 6): with r = RN(1/b), the correctly rounded reciprocal
// (shared by every quotient of the same divisor), q = RN(a·r) is within an ulp of a/b and the fma
// correction RN(q + (a − q·b)·r) is the correctly rounded a/b (Markstein's theorem; normal operands, and a
// remainder a − q·b above the subnormal range).  RN(1/b) itself: one Newton step from v_rcp_f32 (faithful,
// ≤ 1 ulp) is the correctly rounded reciprocal for every divisor but those with an all-ones mantissa
// (b = 2^e·(2 − 2^-23)), whose RN(1/b) = 2^(−e−1)·(1 + 2^-23) has the bit pattern 0x7F000000 − bits(b) (b > 0)
// and is selected there (branch-free; a branch here split the trial stage's block).
// tests/test_division.py checks both statements on the host (every divisor mantissa); the IRM_DIV_CHECK build
// counts the kernel's mismatches against __fdiv_rn (tools/div_check.py → profiles/r06_div_check.txt: 0).
// The BLS step direction ĝ = G/‖G‖ (optimizer_BLS.py:165) uses it (b = ‖G‖ > 0, normal).
__device__ __forceinline__ float rcp_rn_of(float b, float r) {  // r = rcp_refined(b)
    const unsigned u = __float_as_uint(b);
    return (u & 0x7fffffu) == 0x7fffffu ? __uint_as_float(0x7F000000u - u) : r;
}

// One f32x4 of an operator fragment array through a buffer descriptor: the per-lane part of the address in
// one VGPR (voff, shared by every load of a stream), the wave-uniform part (tile, k-quad) in soff — a
// streamed operator holds no 64-bit address per load (the dense stages' unrolled k-loops spilled them)
__device__ __forceinline__ f32x4 ld_frag(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// Smallest step a rounding residual is folded with (e' = −e/step): |e'| ≤ 1e-3·2^80 ≈ 1e21 stays
// finite where a tiny BLS step (lr/‖G‖ after many rejected trials, or --gd-lr 0) would give ±inf.
constexpr float kMinRefStep = 8.271806e-25f;  // 2^-80

// One fp32 α element of the reference's GD / BLS update and its rounding residual:
//   α' = fl(fl(c·α) − fl(lr·ĝ))                        (optimizer_GD.py:81, optimizer_BLS.py:139)
//   e  = α' − (c·α − step·G)  exactly (to fp32 rounding of e itself), where c·[T; V] − step·F·y'
//        is the waypoint-space update the kernel applies (ĝ = G for GD, G/‖G‖ for BLS).
// Products and the subtraction are rounded separately (the reference's arithmetic, no fma); the
// residuals come from fma (c·α − fl(c·α) is exact) and TwoSum.
__device__ __forceinline__ float alpha_step(float al, float c, float lr, float gh, float step, float G, float& e) {
    const float p1 = unfused(c * al), p2 = unfused(lr * gh);
    const float an = unfused(p1 - p2);
    const float ep1 = fmaf(c, al, -p1);                 // c·α − p1
    const float bb = an - p1;                           // TwoSum(p1, −p2) = an + es
    const float es = (p1 - (an - bb)) + (-p2 - bb);
    const float p = unfused(step * G);
    const float ep = fmaf(step, G, -p);                 // step·G − p
    e = (((p - p2) - es) + ep) - ep1;                   // α' − (c·α − step·G)
    return an;
}

// alpha_step for GD (ĝ = G, step = lr): step·G is the reference's own product p2, so its term drops.
// α' = fl(fl(c·α) − fl(lr·G)) (optimizer_GD.py:81) and the scaled residual the direction folds in,
// e' = −(α' − (c·α − lr·G))/lr = (c·α − α')/lr − G, as u = fl(c·α − α') (one rounding, |u| ≈ |lr·G|) and
// e' = fl(u·(1/lr) − G) (ne = −1/lr): the residual to 2^-24 of |G| (i.e. the waypoint state to 2^-24 of a
// step per step, below the rank-16 direction's own 1.5e-7) in two FMAs instead of TwoSum and the two
// product errors (alpha_step's form: 9 more VALU per component on the round's critical path)
__device__ __forceinline__ float alpha_step_gd2(float al, float c, float lr, float G, float ne, float& eo) {
    const float p1 = unfused(c * al), p2 = unfused(lr * G);
    const float an = unfused(p1 - p2);
    const float u = fmaf(c, al, -an);
    eo = fmaf(-u, ne, -G);
    return an;
}

// Operator fragments a wave keeps in VGPRs across all rounds (REGOPS).
// Capacities mirror regops_fit (irm_kernels.hpp): a 512-thread workgroup (8 waves) keeps 4 stage-1
// k-quads and 2 stage-2 tiles per wave (N ≤ 128 at R = 32), a 256-thread one up to 8 of each.

// Problem shape of an optimiser launch.  FixShape: compile-time N / R (and everything derived,
// incl. the LDS layout head) for the common shapes; DynShape: any shape, read from KParams.
template <int D_, int N_, int RP_>
struct FixShape {
    static constexpr int D = D_, N = N_, NK = (N_ + 15) / 16 * 16, MP = 2 * NK, RP = RP_;
    static constexpr int NW = (N_ + 63) / 64 * 64, WPT = NW / 64, NSPLIT = stage1_splits(NK);
    static constexpr bool kVariants = false;  // end-effector cost only (the reference's)
    static constexpr bool kDense = false;
    static constexpr int kNW = NW;             // lanes per trajectory (0: only known at run time)
    // stage-1 k-quads per split-K unit when the split is even (else 0: checked per quad)
    static constexpr int KQU = (NK / 16) % NSPLIT == 0 ? (NK / 16) / NSPLIT : 0;
    __device__ explicit FixShape(const KParams&) {}
};
// The dense operator (--operator-rank -1: R = N, F = L = [K; dK], V_R = I, so G = y'' and z = e') of a
// fixed shape, for k_lean's GD single loop: one split, every operator fragment streamed from L2.
template <int D_, int N_>
struct DenseShape {
    static constexpr int D = D_, N = N_, NK = (N_ + 15) / 16 * 16, MP = 2 * NK, RP = NK;
    static constexpr int NW = (N_ + 63) / 64 * 64, WPT = NW / 64, NSPLIT = 1;
    static constexpr bool kVariants = false;
    static constexpr bool kDense = true;
    static constexpr int kNW = NW;
    static constexpr int KQU = 0;
    __device__ explicit DenseShape(const KParams&) {}
};
template <int D_>
struct DynShape {
    static constexpr int D = D_;
    static constexpr bool kVariants = true;  // cost variants chosen at run time (whole_robot)
    static constexpr bool kDense = false;
    static constexpr int kNW = 0;
    static constexpr int KQU = 0;
    int N, NK, MP, RP, NW, WPT, NSPLIT;
    __device__ explicit DynShape(const KParams& P)
        : N(P.N), NK(P.NK), MP(P.MP), RP(P.RP), NW(P.NW), WPT(P.NW >> 6), NSPLIT(P.nsplit) {}
};
constexpr int kS1Q(int maxt) { return maxt <= 256 ? 8 : 4; }   // stage-1 float4 per wave
constexpr int kS2T(int maxt) { return maxt <= 256 ? 8 : 2; }   // stage-2 tiles per wave (KQ2 ≤ 2)
// MP of a shape-specialised shape (0 for DynShape, whose MP is a run-time value)
template <class S>
constexpr int shape_mp() {
    if constexpr (S::kNW > 0) return S::MP;
    else return 0;
}

}  // namespace irm
