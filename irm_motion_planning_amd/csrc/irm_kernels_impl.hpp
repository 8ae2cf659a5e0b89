// irm_kernels_impl.hpp — gfx950 (CDNA4) kernel templates of the RKHS trajectory optimiser.
// The optimiser kernels k_optimize and k_lean, then (last lines) the headers of k_forward and the launchers;
// included by the instantiation units irm_opt_inst.hip (one k_optimize shape / k_forward D per object,
// compiled in parallel).  The helpers lie in part headers (below): irm_kernels.hip, irm_dense.hip and
// irm_fit.hip include the parts they use and not this file.
//
// Hot path of simongroeger/irm_motion_planning: optimizer_GD.py:173-232 and
// optimizer_BLS.py:126-213 over trajectory.py:271-297 / robot.py:29-87 /
// environment.py:32-58.  DESIGN.md describes the formulation:
//   * the optimiser state is kept in trajectory space, T = K·α·J and
//     V = dK·α·J (the reference keeps α, |α|≈1e3, which cancels in fp32);
//   * the α-space step α' = c·α − s·G, G = (Kᵀa + dKᵀb)Jᵀ, becomes
//     [T';V'] = c·[T;V] − s·L·Lᵀ[a;b]·JᵀJ with L = [K;dK];
//   * L·Lᵀ is applied as F·(Fᵀ[a;b]) with F = L·V_R (V_R = top-R right
//     singular vectors of L; R = N, V = I is the exact dense operator);
//   * both contractions run on v_mfma_f32_16x16x4_f32 with the TB·D
//     (trajectory, joint) columns of a workgroup as the 16 MFMA columns;
//   * one lane per (trajectory, waypoint): the trajectory's waypoints and
//     velocities live in that lane's registers for the whole optimisation;
//     FK / obstacle potential / penalties are VALU, per-trajectory
//     reductions are DPP wave reductions + a cross-wave LDS combine;
//   * the GD / BLS control flow is a per-trajectory state machine whose
//     scalar state is replicated in the trajectory's lanes (every lane takes
//     the same decision from the same reduced values), inside one persistent
//     launch per optimize().
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "irm_kernels.hpp"
// the parts cut out so far (each includes what it needs)
#include "irm_alpha_exact.hpp"  // eval_exact, eval_exact_loop, grad_exact
#include "irm_lean_plan.hpp"    // LeanFlow, LeanPhase, LeanPlan: k_lean's compile-time decisions
#include "irm_wave.hpp"         // packed-fp32 types, DPP wave reductions, store_tile
#include "irm_prof.hpp"         // phase profiler, IRM_STAMP / IRM_COUNT
#include "irm_physics.hpp"      // per-waypoint physics and its reductions
#include "irm_opt_common.hpp"   // optimiser arithmetic and problem shapes
#include "irm_dispatch.hpp"     // dispatch_d, dispatch_t, launch_lds
#include "irm_launch_decl.hpp"  // per-shape launcher declarations, the shape lists, IRM_EXTERN_*

namespace irm {

// Row layout of the optimiser's [a; b] / [T; V] buffers and of F: the velocity
// half starts at row NK (= N rounded up to 16), so the position half is whole
// k-quads of its own and stage 1 can skip the velocity half when b is zero
// away from the two endpoint rows (the usual case); the endpoint rows then enter
// through the precomputed operator columns h0 = F·F[NK]ᵀ, h1 = F·F[NK+N−1]ᵀ.
//
// One round of a workgroup (TB trajectories, one lane per waypoint):
//   stage 1   y' = Fᵀ·[a'; b']          (MFMA, split-K over the waves → Ypart)
//             a' = a·JᵀJ, b' = b·JᵀJ were mixed per lane when written, so y' = y·JᵀJ
//   stage 2   G = (V_R·y')·J⁻¹ (MFMA tile set); GD also Δ[T; V] = F·y' (B operand = Σ partials,
//             summed on load)
//   update    GD:  [T; V]' = c·[T; V] − s·Δ  (Δ latched in registers per direction)
//             BLS: [T; V]' = eval_exact(α_j), the trial's fp32 iterate (below)
//   evaluate  cost at the trial point; gradient inputs for the next direction
//   decide    the reference's accept / reject / λ logic per trajectory
//   GD accept α' = fl(fl(c·α) − fl(lr·G)) per lane in fp32 with the reference's rounding, the rounding
//             residual folded into the next direction through z = V_Rᵀ·e' (k_lean's scheme)
// BLS: every trial's α_j = fl(fl(c_j·α) − fl(lr_j·ĝ)), ĝ = G/‖G‖ (optimizer_BLS.py:139, 165) is formed
// per lane and its trajectory evaluated exactly, as the reference evaluates it: at N ≳ 500 (|α| ≈ 1e3,
// singular K) one ulp of α moves the endpoint velocities by ~2e-3, so a trajectory that takes a trial's
// rounding one step late (the GD scheme) decides a noise-dominated line search on other losses than the
// reference (tools/e2e_ensemble.py: 47-67 gradient evaluations against the reference's 89-122 at
// N = 500); the exact evaluation costs 2·N²·D fp64 FMAs per trial, this path's shapes are the small
// batches outside k_lean's set.  Accepting a trial takes α_j and its [T; V] as they are.
// When an inner loop ends (PH_RESYNC) [T; V] is replaced by eval_exact(α).
// FULL (shape-specialised REGOPS launches of exactly MAXT threads): the stage-2 tiles per wave are
// known exactly, so only those operator fragments occupy VGPRs (as in k_lean<…, FULL>).
template <class S, int MAXT, bool OPS_LDS, bool REGOPS, bool BLS, bool FULL = false>
// 256-thread workgroups without register-resident operators fit two per CU (≤ 256 VGPRs); the
// REGOPS variants need more and keep one (they are launched one per CU anyway).
__global__ __launch_bounds__(MAXT, (MAXT <= 256 && !REGOPS) ? 2 : 1) void k_optimize(KParams P) {
    constexpr int D = S::D;
    static_assert(!FULL || (REGOPS && S::kNW > 0), "FULL: shape-specialised REGOPS variants only");
    constexpr int S1Q = kS1Q(MAXT);
    constexpr int S2T = FULL ? (shape_mp<S>() / 16 + MAXT / 64 - 1) / (MAXT / 64) : kS2T(MAXT);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const S sh(P);
    const Head H = plan_head(sh.MP, sh.RP, sh.NSPLIT, true);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = FULL ? MAXT / 64 : P.BT >> 6;
    const int N = sh.N, NW = sh.NW, TB = P.TB, RP = sh.RP, MP = sh.MP, NK = sh.NK;
    const int WPT = sh.WPT;             // waves per trajectory
    const int t = wave / WPT;           // this lane's trajectory (wave-uniform)
    const int n = tid - t * NW;         // this lane's waypoint (and row r of y for n < RP)
    const int n0 = (wave - t * WPT) * 64;  // first waypoint of this wave
    const int tb0 = blockIdx.x * TB;
    const int ntb = min(TB, P.B - tb0);
    if (ntb <= 0) return;
    const bool tvalid = t < ntb;
    const bool valid = tvalid && n < N;
    const bool yrow = tvalid && n < RP;
    const size_t b = (size_t)(tb0 + (tvalid ? t : 0));
    constexpr bool bls = BLS;
    const bool rec = P.record_series && P.series;
    Prof prof;
    if (tid == 0) prof.init();

    float* X = smem + H.X;    // [a'; b'] (rows 0..N-1, NK..NK+N-1) × 16 columns
    float* dP = smem + H.dP;  // Δ[T; V], same row layout
    float* Ypart = smem + H.Ypart;
    float* Ymix = smem + H.Ymix;
    float* red = smem + H.red;
    float* sg = smem + H.sg;
    float* wp = smem + H.wp;
    // [0,1] direction masks (bit per column) and [3,4] resync masks (bit per trajectory) by
    // round parity; [2] done mask; [5,6] "b' non-zero away from the endpoints" by round parity
    unsigned* flagw = reinterpret_cast<unsigned*>(smem + H.flags);
    float* obsL = smem + H.obs;
    const float* F1 = P.F1frag;
    const float* F2 = P.F2frag;

    const int KQ1 = MP / 16, KQa = NK / 16, MT1 = RP / 16;  // stage 1: (RP × MP)·(MP × 16)
    const int KQ2 = RP / 16, MT2 = MP / 16;                 // stage 2: (MP × RP)·(RP × 16)
    const int nsplit = sh.NSPLIT;
    // stage-1 unit of this wave (split-K over the position half): tile, k-quads [kq0, kq1)
    const bool has1 = wave < MT1 * nsplit;
    const int tile1 = wave % MT1, sp1 = wave / MT1;
    const int kq0 = (KQa * sp1) / nsplit, kq1 = (KQa * (sp1 + 1)) / nsplit;

    // ----------------------------------------------------------- prologue
    if (OPS_LDS && !REGOPS) {
        bool mov = false;  // (only the DynShape instantiations have the moving variant)
        if constexpr (S::kVariants) mov = P.moving != 0;
        bool vias = false;  // (nor the via words, which precede the staged operators)
        if constexpr (S::kVariants) vias = P.via != 0;
        const Plan L = plan_lds(P, OPS_LDS, true, false, mov, vias);
        const int n1 = (int)frag_floats(RP, MP) / 4, n2 = (int)frag_floats(MP, RP) / 4;
        const f32x4* g1 = reinterpret_cast<const f32x4*>(P.F1frag);
        const f32x4* g2 = reinterpret_cast<const f32x4*>(P.F2frag);
        f32x4* l1 = reinterpret_cast<f32x4*>(smem + L.f1);
        f32x4* l2 = reinterpret_cast<f32x4*>(smem + L.f2);
        for (int e = tid; e < n1; e += P.BT) l1[e] = g1[e];
        for (int e = tid; e < n2; e += P.BT) l2[e] = g2[e];
        F1 = smem + L.f1;
        F2 = smem + L.f2;
    }
    // RV: the velocity half of stage 1's fragments is register-resident too (dense rounds, where
    // b' is non-zero away from the endpoints, then read no operator from memory)
    constexpr bool RV = REGOPS && MAXT > 256 && !BLS;  // (the BLS state leaves no room: spills)
    f32x4 a1[REGOPS ? S1Q : 1], a2[REGOPS ? S2T * 2 : 1], a1v[RV ? S1Q : 1];
    if (REGOPS) {  // operator A-fragments resident in VGPRs for the whole launch
        const f32x4* g1 = reinterpret_cast<const f32x4*>(P.F1frag);
        const f32x4* g2 = reinterpret_cast<const f32x4*>(P.F2frag);
#pragma unroll
        for (int i = 0; i < S1Q; ++i) {
            a1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (has1 && kq0 + i < kq1) a1[i] = g1[((size_t)tile1 * KQ1 + kq0 + i) * 64 + lane];
            if constexpr (RV) {
                a1v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (has1 && kq0 + i < kq1) a1v[i] = g1[((size_t)tile1 * KQ1 + KQa + kq0 + i) * 64 + lane];
            }
        }
#pragma unroll
        for (int j = 0; j < S2T; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a2[j * 2 + i] = f32x4{0.f, 0.f, 0.f, 0.f};
                const int tile = wave + j * nwaves;
                if (tile < MT2 && i < KQ2) a2[j * 2 + i] = g2[((size_t)tile * KQ2 + i) * 64 + lane];
            }
    }
    // endpoint-velocity operator columns for this lane's rows (sparse stage 1), and the
    // F rows of the two endpoint velocities for the BLS norms (rows r = n < RP)
    const float h0T = valid ? P.Hend[n] : 0.f, h1T = valid ? P.Hend[MP + n] : 0.f;
    const float h0V = valid ? P.Hend[NK + n] : 0.f, h1V = valid ? P.Hend[MP + NK + n] : 0.f;
    const float fb0 = yrow ? P.Fbot[(size_t)0 * RP + n] : 0.f;
    const float fb1 = yrow ? P.Fbot[(size_t)(N - 1) * RP + n] : 0.f;
    stage_obstacles<S::kVariants>(P, tb0, ntb, obsL);
    for (int e = tid; e < RP * kLd; e += P.BT) Ymix[e] = 0.f;
    // GD: the rounding residual rows e' live in dP's direction columns between an accepted step and the
    // next stage 1 (stage 2 rewrites dP only after the stage-1 barrier); none pending at start
    if constexpr (!BLS)
        for (int e = tid; e < MP * kLd; e += P.BT) dP[e] = 0.f;
    // G's endpoint velocity columns for this lane's row (G = V_R·y'·J⁻¹, see the latch)
    const float hv0 = valid ? P.HV[n] : 0.f, hv1 = valid ? P.HV[NK + n] : 0.f;
    if (tid < 8) flagw[tid] = 0u;
    // Parameters used only on rare paths (outer-loop step, line search, resync, series) live in
    // LDS so that they hold no SGPRs across the loop.
    float* cold = smem + H.cold;
    for (int i = tid; i < kColdWords; i += P.BT) {
        float val = 0.f;
        if (i < IRM_MAX_LR) val = P.gd_lr[i];
        else if (i == C_LCI) val = P.lci;
        else if (i == C_EPSP) val = P.eps_p;
        else if (i == C_EPSV) val = P.eps_v;
        else if (i == C_PMAX) val = P.pmax;
        else if (i == C_PMIN) val = P.pmin;
        else if (i == C_VMAX) val = P.vmax;
        else if (i == C_BLR0) val = P.bls_lr0;
        else if (i == C_BA) val = P.bls_a;
        else if (i == C_BP) val = P.bls_bp;
        else if (i == C_BM) val = P.bls_bm;
        else if (i == C_MAXOUT) val = __int_as_float(P.max_outer);
        else if (i == C_MAXBLS) val = __int_as_float(P.max_bls);
        else if (i == C_MAXSER) val = __int_as_float(P.max_series);
        else if (i == C_TRCAP) val = __int_as_float(P.trace ? P.trace_cap : 0);
        else if (i >= C_PTR && i < C_PTR + 10) {
            const int w = i - C_PTR;
            const void* ptrs[5] = {P.series, P.Vr, P.Kt, P.dKt, P.trace};
            const uint64_t a = reinterpret_cast<uint64_t>(ptrs[w >> 1]);
            val = __uint_as_float((w & 1) ? (uint32_t)(a >> 32) : (uint32_t)a);
        } else if (i >= C_MINV && i < C_MINV + D * D) val = P.Minv[i - C_MINV];
        else if (i >= C_WAL && i < C_WAL + D) val = P.wal[i - C_WAL];
        else if (i >= C_JINV && i < C_JINV + D * D) val = P.Jinv[i - C_JINV];
        else if (i >= C_J && i < C_J + D * D) val = P.J[i - C_J];
        cold[i] = val;
    }
    auto cold_ptr = [&](int w) -> float* {
        const uint64_t lo = __float_as_uint(cold[C_PTR + 2 * w]), hi = __float_as_uint(cold[C_PTR + 2 * w + 1]);
        return reinterpret_cast<float*>(lo | (hi << 32));
    };
    auto cold_int = [&](int i) { return __float_as_int(cold[i]); };
    stage_alpha<D>(P, tb0, ntb, X, NK);
    __syncthreads();
    // T0 = (K·α0)·J, V0 = (dK·α0)·J  (trajectory.py:63-65), correctly rounded.
    // ab: this lane's row of the α the state is expressed against (α0, then the α
    // materialised at the last resync).
    float q[D], v[D], s[D], g[D], ab[D], dT[D], dV[D], Gl[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        q[k] = v[k] = 0.f;
        dT[k] = dV[k] = Gl[k] = 0.f;
        ab[k] = valid ? X[n * kLd + t * D + k] : 0.f;
        s[k] = tvalid ? P.start[b * D + k] : 0.f;
        g[k] = tvalid ? P.goal[b * D + k] : 0.f;
    }
    if (valid) {
        eval_exact<D>(P, X + t * D, n, q, v);
        if (rec) {
#pragma unroll
            for (int k = 0; k < D; ++k) P.series[(b * P.max_series) * N * D + n * D + k] = q[k];
        }
    }
    __syncthreads();  // every lane has read α0 from X
    for (int e = tid; e < MP * kLd; e += P.BT) X[e] = 0.f;
    const float* obs = obsL + (P.obs_stride ? t * obs_pitch(P.O) : 0);
    // moving obstacles (DynShape launches only, launch_optimize): the velocity table behind the positions and
    // this lane's support time t[n]
    const float* obsv = obs;
    float tau = 0.f;
    if constexpr (S::kVariants) {
        if (P.moving) {
            obsv = obs + obs_vel_offset(P);
            tau = valid ? P.tsup[n] : 0.f;
        }
    }
    // end-effector goal (DynShape launches only): the lane of row N−1 (it reads its problem's target in every
    // evaluation — one lane, an L2 hit — so that nothing more stays in registers across the rounds)
    bool task_row = false;
    if constexpr (S::kVariants) task_row = P.task && valid && n == N - 1;
    // via-points (DynShape launches only): the lane of row m_v (via_code; rows lie in 1 … N−2, so never a
    // start / goal row) and the trajectories' via words r_v², a region of its own behind the obstacles
    // (recomputed from the kernel arguments where they are used: nothing more lives across the rounds)
    auto via_of = [&]() -> int {
        if constexpr (S::kVariants) return (P.via && valid) ? via_code(P, n) : -1;
        else return -1;
    };
    auto via_count = [&]() -> int {
        if constexpr (S::kVariants) return P.via ? P.n_via : 0;
        else return 0;
    };
    auto via_words = [&]() -> float* {
        return smem + obs_region_end(P, H.obs, P.moving != 0) + t * IRM_MAX_VIA;  // Plan::via (plan_lds), this
                                                                                  // trajectory's words
    };

    // stage 1 over the units of this wave: Ypart[s] = Fᵀ·[a'; b'] (velocity half if `full`)
    auto stage1 = [&](bool full) {
        const float* xl = X + (lane >> 4) * kLd + (lane & 15);
        // QB k-quads per batch: their operator fragments (L2) and B rows (LDS) in flight together, then
        // the MFMAs in the sequential order (dense / large-N operators; the REGOPS shapes keep QB = 1)
        auto quads = [&](const f32x4* ap, int qoff, int k0, int k1, f32x4& acc0, f32x4& acc1) {
            constexpr int QB = REGOPS ? 1 : 4;
            for (int kq = k0; kq < k1; kq += QB) {
                f32x4 a[QB];
                float bq[QB][4];
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const bool in = kq + j < k1;
                    const float* xb = xl + (qoff + kq + j) * 16 * kLd;
                    a[j] = in ? ap[(size_t)(kq + j) * 64] : f32x4{0.f, 0.f, 0.f, 0.f};
                    bq[j][0] = in ? xb[0] : 0.f;
                    bq[j][1] = in ? xb[4 * kLd] : 0.f;
                    bq[j][2] = in ? xb[8 * kLd] : 0.f;
                    bq[j][3] = in ? xb[12 * kLd] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    if (kq + j < k1) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][0], bq[j][0], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][1], bq[j][1], acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][2], bq[j][2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][3], bq[j][3], acc1, 0, 0, 0);
                    }
                }
            }
        };
        if (REGOPS) {  // one unit per wave (regops_fit), position-half fragments in VGPRs
            if (has1) {
                // k-quads of this unit: compile-time count for the shape-specialised kernels
                constexpr bool kFix = S::KQU > 0 && S::KQU <= S1Q;
                constexpr int KQU = kFix ? S::KQU : S1Q;
                auto in = [&](int i) { return kFix ? i < KQU : kq0 + i < kq1; };
                float bv[KQU][4], bw[RV ? KQU : 1][4];
#pragma unroll
                for (int i = 0; i < KQU; ++i) {
                    const float* xb = xl + (kq0 + i) * 16 * kLd;
                    bv[i][0] = in(i) ? xb[0] : 0.f;
                    bv[i][1] = in(i) ? xb[4 * kLd] : 0.f;
                    bv[i][2] = in(i) ? xb[8 * kLd] : 0.f;
                    bv[i][3] = in(i) ? xb[12 * kLd] : 0.f;
                }
                if constexpr (RV) {
                    if (full) {
#pragma unroll
                        for (int i = 0; i < KQU; ++i) {
                            const float* xb = xl + (KQa + kq0 + i) * 16 * kLd;
                            bw[i][0] = in(i) ? xb[0] : 0.f;
                            bw[i][1] = in(i) ? xb[4 * kLd] : 0.f;
                            bw[i][2] = in(i) ? xb[8 * kLd] : 0.f;
                            bw[i][3] = in(i) ? xb[12 * kLd] : 0.f;
                        }
                    }
                }
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < KQU; ++i) {
                    if (in(i)) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][0], bv[i][0], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][1], bv[i][1], acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][2], bv[i][2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][3], bv[i][3], acc1, 0, 0, 0);
                    }
                }
                if constexpr (RV) {
                    if (full) {
#pragma unroll
                        for (int i = 0; i < KQU; ++i) {
                            if (in(i)) {
                                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][0], bw[i][0], acc0, 0, 0, 0);
                                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][1], bw[i][1], acc1, 0, 0, 0);
                                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][2], bw[i][2], acc0, 0, 0, 0);
                                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][3], bw[i][3], acc1, 0, 0, 0);
                            }
                        }
                    }
                } else if (full) {
                    quads(reinterpret_cast<const f32x4*>(F1) + ((size_t)tile1 * KQ1 + KQa) * 64 + lane, KQa, kq0,
                          kq1, acc0, acc1);
                }
                store_tile(Ypart + sp1 * RP * kLd, tile1, acc0 + acc1, 0xFFFFu);
            }
        } else {
            for (int u = wave; u < MT1 * nsplit; u += nwaves) {
                const int tile = u % MT1, sp = u / MT1;
                const int k0 = (KQa * sp) / nsplit, k1 = (KQa * (sp + 1)) / nsplit;
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                const f32x4* ap = reinterpret_cast<const f32x4*>(F1) + ((size_t)tile * KQ1) * 64 + lane;
                quads(ap, 0, k0, k1, acc0, acc1);
                if (full) quads(ap + (size_t)KQa * 64, KQa, k0, k1, acc0, acc1);
                store_tile(Ypart + sp * RP * kLd, tile, acc0 + acc1, 0xFFFFu);
            }
        }
    };

    // replicated per-trajectory scalar state
    float loss = 0.f, lsg = P.lsg0, ljl = P.ljl0, lr = 0.f, gnorm = 1.f, anorm = 0.f;
    float cfac = 1.f, step = 0.f;
    int phase = tvalid ? PH_OUTER_START : PH_DONE, outer = 0, inner = 0, trial = 0;
    bool needs_dir = false;
    irm_stats st{};
    st.series_len = rec ? 1 : 0;
    const unsigned tmask = (1u << D) - 1u;
    const unsigned fullmask = (ntb >= 32) ? 0xFFFFFFFFu : ((1u << ntb) - 1u);
    __syncthreads();
    IRM_STAMP(14);

    for (int round = 0;; ++round) {
        const int par = round & 1;
        const unsigned dirmask = flagw[par];
        const unsigned rmask = flagw[3 + par];
        const bool dense = flagw[5 + par] != 0u;  // b' has rows beyond the endpoints: full stage 1
        IRM_STAMP(4);
        if (tid == 0) {  // next round's masks (set in this round's flag section)
            flagw[par ^ 1] = 0u;
            flagw[3 + (par ^ 1)] = 0u;
            flagw[5 + (par ^ 1)] = 0u;
        }
        // ------------------------------------------------ direction (stage 1+2)
        if (dirmask) {
            // the two endpoint velocity rows of the trajectory's gradient inputs (sparse stage 1), read
            // before stage 1 (the waits move to the first use after the stage-1 barrier)
            float e0[D], e1[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                e0[k] = X[NK * kLd + t * D + k];
                e1[k] = X[(NK + N - 1) * kLd + t * D + k];
            }
            IRM_STAMP(1);
            IRM_COUNT(13, dense);
            stage1(dense);
            if constexpr (!BLS) {
                // GD: z = V_Rᵀ·e' (the last accepted step's rounding residual, e' = −e·J/lr, rows of dP)
                // into Ymix, one unit per r-tile over all k-quads, operator from L2 — added to y' for
                // stage 2's F tiles, i.e. [T; V] += L·e·J one step late (k_lean's scheme)
                const float* xl = dP + (lane >> 4) * kLd + (lane & 15);
                // V_R = I (dense operator): z is e' itself (the MFMA's 1·e' plus exact zeros, from +0)
                if (P.v_ident) {
                    for (int u = nwaves - 1 - wave; u < MT1; u += nwaves) {
                        const float* er = dP + (u * 16 + 4 * (lane >> 4)) * kLd + (lane & 15);
                        f32x4 c0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) c0[i] = 0.f + er[i * kLd];
                        store_tile(Ymix, u, c0, 0xFFFFu);
                    }
                } else
                for (int u = nwaves - 1 - wave; u < MT1; u += nwaves) {
                    const f32x4* ap = reinterpret_cast<const f32x4*>(P.VTs) + (size_t)u * KQa * 64 + lane;
                    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    for (int kq = 0; kq < KQa; ++kq) {
                        const f32x4 a = ap[(size_t)kq * 64];
                        const float* xb = xl + kq * 16 * kLd;
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], xb[0], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], xb[4 * kLd], acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], xb[8 * kLd], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], xb[12 * kLd], acc1, 0, 0, 0);
                    }
                    store_tile(Ymix, u, acc0 + acc1, 0xFFFFu);
                }
            }
            IRM_STAMP(5);
            __syncthreads();
            IRM_STAMP(0);
            // BLS norms from y' rows (lane n = row r):
            //   ‖G‖² = Σ_r y'(JᵀJ)⁻¹y'ᵀ,  alpha_norm·‖G‖ = Σ_r (y'·w)², w = (JᵀJ)⁻¹Jᵀ1
            if (bls && needs_dir) {
                float g2 = 0.f, al = 0.f;
                if (yrow) {
                    float y[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) y[d] = fmaf(fb0, e0[d], fb1 * e1[d]);
                    for (int sp = 0; sp < nsplit; ++sp) {
#pragma unroll
                        for (int d = 0; d < D; ++d) y[d] += Ypart[(sp * RP + n) * kLd + t * D + d];
                    }
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        float m = 0.f;
#pragma unroll
                        for (int d = 0; d < D; ++d) m = fmaf(y[d], cold[C_MINV + d * D + k], m);
                        g2 = fmaf(y[k], m, g2);
                        al = fmaf(cold[C_WAL + k], y[k], al);
                    }
                    al = al * al;
                }
                g2 = wred_sum(g2);
                al = wred_sum(al);
                if (lane == 0) {
                    wp[wave * 2] = g2;
                    wp[wave * 2 + 1] = al;
                }
            }
            IRM_STAMP(2);
            // stage 2: G tiles; GD also dP = F(MP × RP)·Σ_s Ypart[s], only the direction columns
            {
                constexpr int kTG = REGOPS ? 1 : 4;  // L2-operand tiles per pass (dense / large-N operators)
                const float* xl = Ypart + (lane >> 4) * kLd + (lane & 15);
                // y' rows (+ GD: z, the folded rounding residual, for the F tiles)
                auto bload = [&](int i, float& b0, float& b1, float& b2, float& b3, bool withz = true) {
                    b0 = b1 = b2 = b3 = 0.f;
                    for (int sp = 0; sp < nsplit; ++sp) {
                        const float* xb = xl + (sp * RP + i * 16) * kLd;
                        b0 += xb[0];
                        b1 += xb[4 * kLd];
                        b2 += xb[8 * kLd];
                        b3 += xb[12 * kLd];
                    }
                    if (withz) {
                        const float* zb = Ymix + (i * 16 + (lane >> 4)) * kLd + (lane & 15);
                        b0 += zb[0];
                        b1 += zb[4 * kLd];
                        b2 += zb[8 * kLd];
                        b3 += zb[12 * kLd];
                    }
                };
                {
                    // G tiles: (V_R·y')[waypoint] into X's position rows (X was consumed by stage 1;
                    // only the direction columns are written; every evaluation round rewrites X), from the
                    // top wave down
                    // dense operator (V_R = I): tile u of V_R·y' is y' rows u·16.. themselves — the MFMA's
                    // 1·y + exact zeros, i.e. the partial sums from +0 (bload's order): no operator loads
                    if (P.v_ident) {
                        for (int u = nwaves - 1 - wave; u < KQa; u += nwaves) {
                            const float* yr = Ypart + (u * 16 + 4 * (lane >> 4)) * kLd + (lane & 15);
                            f32x4 c0 = {0.f, 0.f, 0.f, 0.f};
                            for (int sp = 0; sp < nsplit; ++sp) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) c0[i] += yr[(sp * RP + i) * kLd];
                            }
                            store_tile(X, u, c0, dirmask);
                        }
                    } else
                    // up to kTG tiles per pass over the k-quads: one B read shared by the pass's tiles and
                    // their A fragments in flight together (each tile's accumulation order unchanged)
                    for (int u0 = nwaves - 1 - wave; u0 < KQa; u0 += kTG * nwaves) {
                        f32x4 c[kTG];
#pragma unroll
                        for (int g = 0; g < kTG; ++g) c[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                        for (int i = 0; i < KQ2; ++i) {
                            float b0, b1, b2, b3;
                            bload(i, b0, b1, b2, b3, false);
                            f32x4 a[kTG];
#pragma unroll
                            for (int g = 0; g < kTG; ++g) {
                                const int u = u0 + g * nwaves;
                                a[g] = u < KQa ? reinterpret_cast<const f32x4*>(P.VNs)[((size_t)u * KQ2 + i) * 64 + lane]
                                               : f32x4{0.f, 0.f, 0.f, 0.f};
                            }
#pragma unroll
                            for (int g = 0; g < kTG; ++g) {
                                if (u0 + g * nwaves < KQa) {
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][0], b0, c[g], 0, 0, 0);
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][1], b1, c[g], 0, 0, 0);
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][2], b2, c[g], 0, 0, 0);
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][3], b3, c[g], 0, 0, 0);
                                }
                            }
                        }
#pragma unroll
                        for (int g = 0; g < kTG; ++g)
                            if (u0 + g * nwaves < KQa) store_tile(X, u0 + g * nwaves, c[g], dirmask);
                    }
                }
                if constexpr (BLS) {
                    // BLS: no F tiles (the trial trajectories are evaluated exactly)
                } else if (REGOPS) {
                    f32x4 acc[S2T];
#pragma unroll
                    for (int j = 0; j < S2T; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    float bv[2][4];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (i < KQ2) bload(i, bv[i][0], bv[i][1], bv[i][2], bv[i][3]);
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (i < KQ2) {
#pragma unroll
                            for (int j = 0; j < S2T; ++j) {
                                if (wave + j * nwaves < MT2) {
                                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2 + i][0], bv[i][0], acc[j], 0, 0, 0);
                                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2 + i][1], bv[i][1], acc[j], 0, 0, 0);
                                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2 + i][2], bv[i][2], acc[j], 0, 0, 0);
                                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2 + i][3], bv[i][3], acc[j], 0, 0, 0);
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < S2T; ++j)
                        if (wave + j * nwaves < MT2) store_tile(dP, wave + j * nwaves, acc[j], dirmask);
                } else {
                    for (int t0 = wave; t0 < MT2; t0 += kTG * nwaves) {  // kTG tiles per pass, as above
                        f32x4 c[kTG];
#pragma unroll
                        for (int g = 0; g < kTG; ++g) c[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                        for (int i = 0; i < KQ2; ++i) {
                            float b0, b1, b2, b3;
                            bload(i, b0, b1, b2, b3);
                            f32x4 a[kTG];
#pragma unroll
                            for (int g = 0; g < kTG; ++g) {
                                const int tile = t0 + g * nwaves;
                                a[g] = tile < MT2 ? reinterpret_cast<const f32x4*>(F2)[((size_t)tile * KQ2 + i) * 64 + lane]
                                                  : f32x4{0.f, 0.f, 0.f, 0.f};
                            }
#pragma unroll
                            for (int g = 0; g < kTG; ++g) {
                                if (t0 + g * nwaves < MT2) {
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][0], b0, c[g], 0, 0, 0);
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][1], b1, c[g], 0, 0, 0);
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][2], b2, c[g], 0, 0, 0);
                                    c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][3], b3, c[g], 0, 0, 0);
                                }
                            }
                        }
#pragma unroll
                        for (int g = 0; g < kTG; ++g)
                            if (t0 + g * nwaves < MT2) store_tile(dP, t0 + g * nwaves, c[g], dirmask);
                    }
                }
            }
            __syncthreads();
            IRM_STAMP(3);
            if (needs_dir) {
                // GD: latch this lane's direction rows (+ the endpoint-velocity columns)
                if constexpr (!BLS) {
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        float ut = dP[n * kLd + t * D + k], uv = dP[(NK + n) * kLd + t * D + k];
                        // endpoint velocity rows: their operator columns in every round (stage 1's
                        // operator has zero columns there)
                        ut = fmaf(h0T, e0[k], fmaf(h1T, e1[k], ut));
                        uv = fmaf(h0V, e0[k], fmaf(h1V, e1[k], uv));
                        dT[k] = ut;
                        dV[k] = uv;
                    }
                }
                IRM_STAMP(16);
                // G = (V_R·y')·J⁻¹ + its endpoint velocity columns (y' = y·JᵀJ, G = V_R·y·Jᵀ)
                {
                    float gr[D];
#pragma unroll
                    for (int k = 0; k < D; ++k)
                        gr[k] = valid ? fmaf(hv0, e0[k], fmaf(hv1, e1[k], X[n * kLd + t * D + k])) : 0.f;
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        float gk = 0.f;
#pragma unroll
                        for (int l = 0; l < D; ++l) gk = fmaf(gr[l], cold[C_JINV + l * D + k], gk);
                        Gl[k] = gk;
                    }
                }
                if (bls) {
                    float tg = 0.f, ta = 0.f;
                    for (int ww = 0; ww < WPT; ++ww) {
                        tg += wp[(t * WPT + ww) * 2];
                        ta += wp[(t * WPT + ww) * 2 + 1];
                    }
                    gnorm = sqrtf(tg);
                    anorm = ta / gnorm;
                    st.grad_evals++;  // inner-loop head: cost + grad at α (optimizer_BLS.py:163-164)
                    st.cost_evals++;
                    phase = PH_BLS_TRIAL;
                    trial = 0;
                } else {
                    cfac = P.gd_c[outer];  // fp32(1 − λ_reg·lr) (optimizer_GD.py:185)
                    step = lr;
                }
                needs_dir = false;
            }
        }
        if (phase == PH_BLS_TRIAL) cfac = unfused(1.f - unfused(P.lreg * lr));  // (1 − λ_reg·bls_lr) in fp32 (optimizer_BLS.py:139)
        // ------------------------------------------------------- resync
        // Trajectories whose inner loop ended last round: [T; V] = eval_exact(α) (α is the reference's
        // fp32 iterate), so the constraint check below and the caller's evaluate(α_out) see the same
        // waypoints bit for bit; GD's pending residual is absorbed.
        if (rmask) {  // block-uniform; α is carried explicitly in fp32 (both optimisers)
            const bool rs = tvalid && ((rmask >> t) & 1u);  // wave-uniform
            if (rs && valid) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    X[n * kLd + t * D + k] = ab[k];
                    dP[n * kLd + t * D + k] = 0.f;  // the pending residual is in the exact trajectory
                }
            }
            __syncthreads();
            if (rs && valid) {
                eval_exact<D>(P, X + t * D, n, q, v, cold_ptr(2), cold_ptr(3));
                // the last extended-vis frame shows the exact trajectory of this α — but frame 0 stays the
                // initial trajectory: a BLS inner loop that ends on its first, accepted step has moved α
                // without a snapshot (optimizer_BLS.py:97-107)
                if (rec && st.series_len > 1) {
                    float* ser = cold_ptr(0);
                    const int ms = cold_int(C_MAXSER);
#pragma unroll
                    for (int k = 0; k < D; ++k) ser[((b * ms) + st.series_len - 1) * N * D + n * D + k] = q[k];
                }
            }
        }
        IRM_STAMP(17);
        // ------------------------------------------------------- update
        float q2[D], v2[D], aj[BLS ? D : 1];
        // (K / dK rows per pipelined batch of the trial's exact evaluation: 8, as the resync's)
        constexpr int kTrialU = 8;
        if constexpr (BLS) {
            // the trial's α_j = fl(fl(c_j·α) − fl(lr_j·ĝ)), ĝ = G/‖G‖ (optimizer_BLS.py:139, 165), through
            // X's position rows (consumed by this round's stage 1 and latch; rewritten by the gradient
            // inputs after the evaluation barrier), [T; V] = eval_exact(α_j)
            const bool trl = (phase == PH_BLS_TRIAL);  // wave-uniform
            if (trl && valid) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    aj[k] = unfused(unfused(cfac * ab[k]) - unfused(lr * (Gl[k] / gnorm)));
                    X[n * kLd + t * D + k] = aj[k];
                }
            }
            __syncthreads();
            if (trl && valid) {
                eval_exact<D, kTrialU>(P, X + t * D, n, q2, v2, cold_ptr(2), cold_ptr(3));
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    q2[k] = q[k];
                    v2[k] = v[k];
                }
            }
        } else if (phase == PH_GD_INNER) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                q2[k] = fmaf(cfac, q[k], -(step * dT[k]));
                v2[k] = fmaf(cfac, v[k], -(step * dV[k]));
            }
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                q2[k] = q[k];
                v2[k] = v[k];
            }
        }
        // ------------------------------------------------------- evaluate
        IRM_STAMP(6);
        const bool ev = (phase != PH_DONE);  // wave-uniform
        WP<D> w;
        if (ev) {
            float task_r2 = 0.f;
            if (valid) {
                if constexpr (S::kVariants) {
                    EE<D> ee;
                    if (P.moving) {  // this waypoint's obstacle table is the one at its support time
                        if (P.whole_robot) eval_waypoint<D, true, true, true, true, true>(P, q2, v2, obs, w, nullptr, obsv, tau, &ee);
                        else eval_waypoint<D, false, true, true, true, true>(P, q2, v2, obs, w, nullptr, obsv, tau, &ee);
                    } else if (P.whole_robot) eval_waypoint<D, true, true, true, false, true>(P, q2, v2, obs, w, nullptr, nullptr, 0.f, &ee);
                    else eval_waypoint<D, false, true, true, false, true>(P, q2, v2, obs, w, nullptr, nullptr, 0.f, &ee);
                    // end-effector goal: the end row's ge = J_eeᵀ·(f − p) replaces this lane's copy of the
                    // joint goal (not read again in such a launch) and r² the squared joint distance below
                    if (task_row) task_end_row<D>(ee, P.goal_xy[b * 2], P.goal_xy[b * 2 + 1], g, task_r2);
                    // via row: ge_v likewise (an interior row never reads its copy of the joint goal), r_v²
                    // to the trajectory's via words (the lane reads its target in every evaluation, as above)
                    if (const int via = via_of(); via >= 0) {
                        float r2 = 0.f;
                        via_row_terms<D, true>(P, b, via, q2, ee, g, r2);
                        via_words()[via & 3] = r2;
                    }
                } else {
                    eval_waypoint<D, false, true, true>(P, q2, v2, obs, w);
                }
            }
            IRM_STAMP(8);
            const LeanW cw = lean_weights(P, ljl);
            const float us = fmaf(cw.c_mean, w.cv, cw.c_pen * (w.jp + w.jv));
            ered_store(valid, w.cv, us, w.tx, w.tn, w.va, phase == PH_RESYNC, n0, red, wave);
            if (valid && (n == 0 || n == N - 1)) {  // trajectory.py:183-204 rows 0 and N−1
                float a = 0.f, bb = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float e = q2[d] - (n == 0 ? s[d] : g[d]);
                    a = fmaf(e, e, a);
                    bb = fmaf(v2[d], v2[d], bb);
                }
                if constexpr (S::kVariants) a = task_row ? task_r2 : a;
                sg[t * 4 + (n == 0 ? 0 : 2)] = a;
                sg[t * 4 + (n == 0 ? 1 : 3)] = bb;
            }
        }
        IRM_STAMP(9);
        __syncthreads();
        IRM_STAMP(7);
        if (ev) {
            // combine the trajectory's wave partials (fixed order)
            const float* r0 = red + (t * WPT) * 8;
            float cmax = r0[0];
            int cidx = __float_as_int(r0[1]);
            float usum = r0[2], tx = r0[3], tn = r0[4], va = r0[5];
            for (int ww = 1; ww < WPT; ++ww) {
                const float* rw = red + (t * WPT + ww) * 8;
                amax_step(cmax, cidx, rw[0], __float_as_int(rw[1]));
                usum += rw[2];
                tx = fmaxf(tx, rw[3]);
                tn = fminf(tn, rw[4]);
                va = fmaxf(va, rw[5]);
            }
            const float e_a0 = sg[t * 4 + 0], e_b0 = sg[t * 4 + 1], e_a1 = sg[t * 4 + 2], e_b1 = sg[t * 4 + 3];
            IRM_STAMP(18);
            float sgpc = fmaf(0.5f, e_a0, 0.5f * e_a1);                         // trajectory.py:187
            bool via_ok = true;  // every via distance below eps_position (read by the resync's check)
            if constexpr (S::kVariants) {  // the via terms, in index order after the two (include/irm.h)
                const int nvia = via_count();
                for (int i = 0; i < nvia; ++i) {
                    const float r2 = via_words()[i];
                    sgpc = fmaf(0.5f, r2, sgpc);
                    via_ok = via_ok && sqrtf(r2) < cold[C_EPSP];
                }
            }
            const float sgvc = fmaf(0.5f, e_b0, 0.5f * e_b1);                   // trajectory.py:203
            // trajectory.py:85-87 + 281 (mean and joint-limit terms pre-summed in usum)
            const float nl = fmaf(lsg, sgpc + sgvc, fmaf(P.lam_max, cmax, usum));
            const float lsg_e = lsg, ljl_e = ljl;
            // --------------------------------------------------- decide
            int accept = 0;
            bool snap = false, to_end = false;
            if (phase == PH_OUTER_START) {  // optimizer_GD.py:209-211 / optimizer_BLS.py:193
                loss = nl;
                if (!bls) st.cost_evals++;
                accept = 2;
                lr = bls ? cold[C_BLR0] : cold[outer];
                needs_dir = true;
                if (!bls) phase = PH_GD_INNER;
                // BLS with max_outer_iteration <= 0: the reference's outer while_loop never runs and
                // optimize() returns α0 (optimizer_BLS.py:184-186, 210-213) — straight to the resync
                // (α materialised, constraints reported), no outer iteration counted
                if (P.max_inner <= 0 || (bls && cold_int(C_MAXOUT) <= 0)) to_end = true;
            } else if (phase == PH_BLS_REEVAL) {  // gradient at the unchanged α after a fully rejected search
                needs_dir = true;
            } else if (phase == PH_RESYNC) {
                // constraintsFulfilled(α) (trajectory.py:129-137, robot.py:90-113) on the
                // materialised α; optimizer_GD.py:214-224 / optimizer_BLS.py:201-211
                const float eps_p = cold[C_EPSP], eps_v = cold[C_EPSV];
                bool ok = sqrtf(e_a0) < eps_p && sqrtf(e_a1) < eps_p && sqrtf(e_b0) < eps_v &&
                          sqrtf(e_b1) < eps_v && tx <= cold[C_PMAX] && tn >= cold[C_PMIN] && va <= cold[C_VMAX];
                ok = ok && via_ok;
                if (!bls || cold_int(C_MAXOUT) > 0) st.outer_iterations++;
                st.constraints_ok = ok ? 1 : 0;
                if (ok) {
                    phase = PH_DONE;
                } else {
                    outer++;
                    lsg = lsg * cold[C_LCI];
                    ljl = ljl * cold[C_LCI];
                    inner = 0;
                    phase = (outer >= cold_int(C_MAXOUT)) ? PH_DONE : PH_OUTER_START;
                }
            } else if (phase == PH_GD_INNER) {  // optimizer_GD.py:180-195
                st.grad_evals++;
                st.cost_evals++;
                if (loss - nl < P.llr) {
                    to_end = true;  // minimized: the step is discarded
                } else {
                    accept = 1;
                    loss = nl;
                    inner++;
                    st.inner_iterations++;
                    snap = true;
                    if (inner >= P.max_inner) to_end = true;
                    else needs_dir = true;
                }
            } else {  // PH_BLS_TRIAL: optimizer_BLS.py:136-150, 172-178
                st.cost_evals++;
                st.bls_trials++;
                const float required = loss - cold[C_BA] * lr * anorm;
                // line-search log of problem 0 (diagnostics; the reference's per-trial values,
                // optimizer_BLS.py:139-149, 163-166)
                if (b == 0 && n == 0 && st.bls_trials - 1 < cold_int(C_TRCAP)) {
                    float* r = cold_ptr(4) + (size_t)(st.bls_trials - 1) * kTraceW;
                    r[0] = (float)outer;
                    r[1] = (float)inner;
                    r[2] = (float)trial;
                    r[3] = lr;
                    r[4] = nl;
                    r[5] = required;
                    r[6] = (nl > required) ? 0.f : 1.f;
                    r[7] = loss;
                    r[8] = gnorm;
                    r[9] = anorm;
                }
                bool inner_end = false, rejected_all = false;
                float improve = 0.f;
                if (nl > required) {
                    lr = lr * cold[C_BM];
                    trial++;
                    if (trial >= cold_int(C_MAXBLS)) inner_end = rejected_all = true;  // new_loss = loss
                } else {
                    accept = 1;
                    lr = lr * cold[C_BP];
                    improve = loss - nl;
                    loss = nl;
                    inner_end = true;
                }
                if (inner_end) {
                    if (improve < P.llr) {
                        to_end = true;
                    } else {
                        inner++;
                        st.inner_iterations++;
                        snap = true;
                        if (inner >= P.max_inner) {
                            to_end = true;
                        } else if (rejected_all) {
                            phase = PH_BLS_REEVAL;
                        } else {
                            needs_dir = true;
                        }
                    }
                }
            }
            if (to_end) {  // inner loop over: materialise α next round, then check constraints
                st.final_loss = loss;
                needs_dir = false;
                phase = PH_RESYNC;
            }
            IRM_STAMP(10);
            // ------------------------- gradient inputs at T2, mixed by JᵀJ (→ y' = y·JᵀJ)
            bool bfar = false;
            if (valid) {
                float a[D], bb[D], tg[D];
                const bool endrow = (n == 0 || n == N - 1);
                const bool viar = via_of() >= 0;
#pragma unroll
                for (int k = 0; k < D; ++k) tg[k] = (n == N - 1 || viar) ? g[k] : s[k];
                // (a via row: g holds ge_v, weighed by λsg in a only — lsg_ep, which weighs v in b, stays 0)
                grad_waypoint_lean<D, S::kVariants>(P, w, q2, v2, n == cidx, endrow ? lsg_e : 0.f, lean_weights(P, ljl_e),
                                                    tg, a, bb, task_row || viar, (endrow || viar) ? lsg_e : 0.f);
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    float ma = 0.f, mb = 0.f;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        ma = fmaf(a[d], P.JtJ[d * D + k], ma);
                        mb = fmaf(bb[d], P.JtJ[d * D + k], mb);
                    }
                    X[n * kLd + t * D + k] = ma;
                    X[(NK + n) * kLd + t * D + k] = mb;
                    bfar |= (!endrow && bb[k] != 0.f);
                }
            }
            if (__ballot(bfar) && lane == 0) atomicOr(&flagw[5 + (par ^ 1)], 1u);
            IRM_STAMP(12);
            // --------------------------------------------------- accept
            if (accept == 1) {
                if constexpr (BLS) {
                    // the trial's α_j and its exactly evaluated [T; V]
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        ab[k] = aj[k];
                        q[k] = q2[k];
                        v[k] = v2[k];
                    }
                } else {
                    // α' = fl(fl(c·α) − fl(lr·G)) (optimizer_GD.py:81, 185) and its residual e' = −e·J/lr
                    // for the next stage 1 (dP rows of this lane: stage 2 has been read)
                    float er[D];
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        ab[k] = alpha_step(ab[k], cfac, lr, Gl[k], step, Gl[k], er[k]);
                        q[k] = q2[k];
                        v[k] = v2[k];
                    }
                    if (valid) {
                        const float ne = -1.f / fmaxf(lr, kMinRefStep);
#pragma unroll
                        for (int k = 0; k < D; ++k) {
                            float z = 0.f;
#pragma unroll
                            for (int l = 0; l < D; ++l) z = fmaf(er[l], cold[C_J + l * D + k], z);
                            dP[n * kLd + t * D + k] = ne * z;
                        }
                    }
                }
            }
            // extended-vis snapshot after every non-breaking inner iteration
            // (optimizer_GD.py:153-154, optimizer_BLS.py:106-107)
            if (rec && snap && st.series_len < cold_int(C_MAXSER)) {
                if (valid) {
                    float* ser = cold_ptr(0);
                    const int ms = cold_int(C_MAXSER);
#pragma unroll
                    for (int k = 0; k < D; ++k) ser[((b * ms) + st.series_len) * N * D + n * D + k] = q[k];
                }
                st.series_len++;
            }
            if (n == 0) {
                if (needs_dir) atomicOr(&flagw[par ^ 1], tmask << (t * D));
                if (phase == PH_DONE) atomicOr(&flagw[2], 1u << t);
                if (phase == PH_RESYNC) atomicOr(&flagw[3 + (par ^ 1)], 1u << t);
            }
        }
        IRM_STAMP(15);
        __syncthreads();
        IRM_STAMP(11);
        if (flagw[2] == fullmask) break;
    }

    // ----------------------------------------------------------- epilogue
    // Every trajectory ended through PH_RESYNC: α = ab and T = eval_exact(α) exactly.
    if (valid) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (P.traj_out) P.traj_out[(b * N + n) * D + k] = q[k];
            if (P.alpha_out) P.alpha_out[(b * N + n) * D + k] = ab[k];
        }
    }
    if (P.stats && tvalid && n == 0) P.stats[b] = st;
    if (tid == 0) prof.flush(P.prof);
}

// ------------------------------------------- GD single loop, lean optimiser
// optimizer_GD.py jit_optimize (max_outer_iteration == 1, dualOptimization false;
// optimizer_GD.py:68-97): G = ∇L(α); α' = (1 − λ_reg·lr)·α − lr·G; accept iff
// L − L(α') ≥ loop_loss_reduction, else stop keeping α; at most max_inner steps; then
// constraintsFulfilled(α) decides constraints_ok.  Without the general state machine: every
// trajectory is either stepping or done, so a round needs no phase logic, no direction / resync
// masks; one parity flag word per round (bit per wave still stepping, bit 31 = dense stage 1) is
// OR-ed by the wave leaders and read by every wave after the end barrier.  Shape-specialised,
// F operators register-resident.
//
// α is carried in fp32 with the reference's rounding.  The reference iterates α (|α| ≈ 1e3, ulp
// ≈ 6e-5, singular K) in fp32: α' = fl(fl(c·α) − fl(lr·G)) — and the rounding of c·α is biased
// (c = 1 − 1.8e-7 moves α by 1.5–3 ulp per step), so its iterate drifts from the same iteration in
// exact arithmetic by ~1e-2 in waypoint space over 200 steps, 10× its own ±1-ulp sensitivity
// (tests/test_reference_bench.py).  Each lane therefore keeps its waypoint's α row
// and applies exactly that update.  The gradient inputs are mixed by Jᵀ when written ([a'; b'] =
// [a; b]·Jᵀ), so stage 1 gives y'' = Fᵀ[a; b]·Jᵀ and G = Lᵀ[a; b]·Jᵀ = V_R·y'' comes from a
// stage-2 tile set (G's endpoint velocity columns through hV) with no mix; the waypoint state
// [T; V] = L·α·J follows the exact part c·[T; V] − lr·(F·y'')·J as before, and the rounding
// residual e = α' − (c·α − lr·G) (error-free transformations: fma residuals and TwoSum) enters
// one round later through stage 1: z = V_Rᵀ·e', e' = −e/lr, is added to y'' on the way into stage
// 2's F tiles, i.e. [T; V] += L·e·J (rank R: the discarded part is below σ_R / σ_0 ≈ 1e-6 of it).
// Only J enters the per-lane mixes (D² scalars: at D = 7 three D×D matrices spilled SGPRs).  The
// evaluation point of a round therefore lags the exact L·α·J by one residual (≤ 1e-4 in
// waypoints, the size of the reference's own fp32 K@α noise); α itself is bit-for-bit the
// reference's update of the G the kernel computes, and the epilogue returns it with
// traj_out = K·α_out·J correctly rounded.
// LDS is column-major here — X / dP as [column][row] (stride MP + 8), the stage-1 partials as
// [split][column][r] (stride RP + 8), e' and G as [column][waypoint] (stride NK + 8) — with the
// k-permuted operator fragments (F1p / F2p / VTp / VNp, frag_index_kp): a lane's four B values of
// a k-group are then one ds_read_b128 and an MFMA result tile one ds_write_b128 per lane (strides
// ≡ 8 mod 16 keep both conflict-free).
// WPL waypoints per lane (lane li of a trajectory owns waypoints li + j·NW/WPL): WPL = 2 lets
// N = 256 trajectories run four to a 512-thread workgroup (C4) without exceeding 256 VGPRs.
template <int WPL>
__device__ __forceinline__ void ered_store_wpl(const bool (&live)[WPL], const float (&cv)[WPL], float us,
                                               float tx, float tn, float va, bool ext, int n0, int nwl,
                                               float* red, int wave) {
    if constexpr (WPL == 1) {
        ered_store(live[0], cv[0], us, tx, tn, va, ext, n0, red, wave);
    } else {
        // this lane's best waypoint (first index on ties: j = 0 is the smaller index)
        float best = live[0] ? cv[0] : -INFINITY;
        int jb = 0;
#pragma unroll
        for (int j = 1; j < WPL; ++j) {
            const float c = live[j] ? cv[j] : -INFINITY;
            if (c > best) {
                best = c;
                jb = j;
            }
        }
        const bool any = live[0];
        float m = best, s = any ? us : 0.f;  // best ≥ +0 or −inf: maxpos (see ered_store)
        m = maxpos(m, dppf<0xB1>(m));
        s += dppf<0xB1>(s);
        m = maxpos(m, dppf<0x4E>(m));
        s += dppf<0x4E>(s);
        m = maxpos(m, dppf<0x141>(m));
        s += dppf<0x141>(s);
        m = maxpos(m, dppf<0x140>(m));
        s += dppf<0x140>(s);
        auto pm = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
        auto ps = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
        const float m2 = maxpos(__uint_as_float(pm[0]), __uint_as_float(pm[1]));
        const float s2 = __uint_as_float(ps[0]) + __uint_as_float(ps[1]);
        auto qm = __builtin_amdgcn_permlane32_swap(__float_as_uint(m2), __float_as_uint(m2), false, false);
        auto qs = __builtin_amdgcn_permlane32_swap(__float_as_uint(s2), __float_as_uint(s2), false, false);
        const float wm = maxpos(__uint_as_float(qm[0]), __uint_as_float(qm[1]));
        const float ws = __uint_as_float(qs[0]) + __uint_as_float(qs[1]);
        int idx = 0x7fffffff;
#pragma unroll
        for (int j = WPL - 1; j >= 0; --j) {  // the smallest j with a hit holds the first index
            const unsigned long long hit = __ballot(best == wm && jb == j && live[j]);
            if (hit) idx = n0 + j * nwl + __builtin_ctzll(hit);
        }
        float ox = 0.f, on = 0.f, oa = 0.f;
        if (ext) {
            ox = wred_max(any ? tx : -INFINITY);
            on = wred_min(any ? tn : INFINITY);
            oa = wred_max(any ? va : 0.f);
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
}

// FULL: the launch has exactly MAXT threads, so the stage-2 tiles per wave are known exactly
// (otherwise kS2T(MAXT) bounds them for smaller launches): C7's 256-thread variant then holds 4
// tiles of operator fragments instead of 8 (32 VGPRs) and does not spill.
//
// QUE: the work queue (LF_GD2 / LF_BLS, one waypoint per lane).  The launch runs a fixed number of
// workgroups; a slot whose problem has finished writes its outputs, takes the next problem index from
// the device counter P.queue (the host sets it to grid·TB) and loads it in the next round (LP_LOAD): that
// round is a resync round of the slot — α0 into its X columns, the exact trajectory, the evaluation with
// the first outer iteration's λ — followed by round 0's decision.  An index ≥ B leaves the slot done for
// good.  No workgroup waits on another: a workgroup leaves when its flag word is empty.
template <class S, int MAXT, int WPL, bool FULL = false, int FLOW = LF_GD1, bool QUE = false>
__global__ __launch_bounds__(MAXT, (LeanPlan<S, MAXT, WPL, FULL, FLOW, QUE>::kBlocksPerCU)) void k_lean(KParams P) {
    // the plan: every compile-time decision of this instantiation (irm_lean_plan.hpp)
    using PL = LeanPlan<S, MAXT, WPL, FULL, FLOW, QUE>;
    constexpr int D = S::D;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const S sh(P);
    const Head H = plan_head(sh.MP, sh.RP, sh.NSPLIT, true, true);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = PL::kWaves > 0 ? PL::kWaves : P.BT >> 6;
    if constexpr (PL::kWaves > 0) __builtin_assume(wave >= 0 && wave < PL::kWaves);  // tile guards fold
    const int N = sh.N, TB = P.TB, RP = sh.RP, MP = sh.MP, NK = sh.NK;
    const int t = wave / PL::WPTL;
    const int li = tid - t * PL::NWL;               // this lane within its trajectory
    const int n0 = (wave - t * PL::WPTL) * 64;     // li of this wave's lane 0
    const int tb0 = blockIdx.x * TB;
    const int ntb = min(TB, P.B - tb0);
    if (ntb <= 0) return;
    const bool tvalid = t < ntb;
    int nn[WPL];
    bool vl[WPL];
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        nn[j] = li + j * PL::NWL;
        vl[j] = tvalid && nn[j] < N;
    }
    bool wl[WPL];  // vl[j] where the trajectory is known to be valid
#pragma unroll
    for (int j = 0; j < WPL; ++j) wl[j] = PL::kAllLive || nn[j] < N;
    size_t b = (size_t)(tb0 + (tvalid ? t : 0));  // (QUE: the slot's current problem)
    const bool rec = !PL::GD1 && !PL::kQueue && P.record_series && P.series;
    Prof prof;
    if (tid == 0) prof.init();

    float* X = smem + H.X;
    float* dP = smem + H.dP;
    float* Ypart = smem + H.Ypart;
    float* red = smem + H.red;
    float* sg = smem + H.sg;
    float* wp = smem + H.wp;
    unsigned* fw = reinterpret_cast<unsigned*>(smem + H.flags);
    float* obsL = smem + H.obs;
    const int nsplit = sh.NSPLIT, zsplit = lean_zsplit(sh.NSPLIT, PL::VL);
    const LeanX LX = lean_extra(plan_lds(P, false, true, true).total, MP, NK, RP, nsplit, PL::VL, D, PL::kHelp ? MAXT : 0, PL::BLS, PL::DENSE);
    float* Eb = smem + LX.eb;  // e' rows [column][waypoint]
    float* Zp = smem + LX.zp;  // stage-1 partials of V_Rᵀ·e'
    float* Gb = smem + LX.gb;  // (V_R·y'')[waypoint] rows [column][waypoint]
    // b'[0], b'[N−1] of this trajectory (a copy of X's endpoint velocity rows, written with them): the B
    // operand of stage 1's endpoint MFMA (below)
    float* EPt = smem + LX.ep + t * 2 * kEpS;
    const float* VT = PL::VL ? smem + LX.vt : P.VTp;
    const float* VN = PL::VL ? smem + LX.vn : P.VNp;
    // V_R fragment quad q (VT: V_Rᵀ for z, VN: V_R for G): from LDS when staged there, else from L2 through a
    // buffer descriptor — the lane's offset in one VGPR, the wave-uniform quad offset in an SGPR, so a wave's
    // batch of fragment loads holds no 64-bit address per load (at N = 256 those spilled)
    const unsigned vbytes = (unsigned)(frag_floats(RP, NK) * 4);
    const __amdgpu_buffer_rsrc_t rVT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.VTp), 0, (int)vbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rVN = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.VNp), 0, (int)vbytes, 0x00020000);
    auto vt_frag = [&](int q) -> f32x4 {
        if constexpr (PL::VL) return reinterpret_cast<const f32x4*>(VT)[(size_t)q * 64 + lane];
        else return ld_frag(rVT, lane * 16, q * 1024);
    };
    auto vn_frag = [&](int q) -> f32x4 {
        if constexpr (PL::VL) return reinterpret_cast<const f32x4*>(VN)[(size_t)q * 64 + lane];
        else return ld_frag(rVN, lane * 16, q * 1024);
    };

    const int KQ1 = MP / 16, KQa = NK / 16, MT1 = RP / 16, KQ2 = RP / 16, MT2 = MP / 16, MTG = NK / 16;
    const int ldx = MP + 8, ldy = lean_ldy(RP), lde = lean_ld(NK);  // column strides, all ≡ 8 mod 64
    const int cl = lane & 15, r4 = 4 * (lane >> 4);  // MFMA column / first of 4 rows of this lane
    // Bank swizzle of every [column][row] buffer: row r of column c lives at r ^ (c & 4) (the 4-row
    // quads of a 16-row group swap pairwise in columns 4-7 / 12-15).  With column strides ≡ 8 mod 64
    // the MFMA tiles' ds_read_b128 (16-lane groups, 64 banks) and ds_write_b128 (8-lane groups, 32
    // banks) are then both conflict-free; per-row accesses stay so (a column's rows only permute).
    const int r4x = r4 ^ (cl & 4);
    auto swz = [](int r, int c) { return r ^ (c & 4); };
    // 7-DoF shapes: a lane index laundered at a rare path's use, so that the path's per-lane addresses are
    // formed there instead of being held across the round loop (the 7-DoF dual-loop / BLS variants spilled
    // them); the 3-joint shapes have the registers, and measured 3 % slower on C3-BLS with it
    auto lnd = [](int x) {
        if constexpr (PL::kLaunder) asm volatile("" : "+v"(x));
        return x;
    };
    int ycl = cl;     // stage 2's Ypart column for this lane's B column (a helper round: the helper's read t*'s)
    int r4y = r4x;    // its first row under the row swizzle of column ycl
    const bool has1 = wave < MT1 * nsplit;
    const int tile1 = wave % MT1, sp1 = wave / MT1;
    const int kq0 = (KQa * sp1) / nsplit, kq1 = (KQa * (sp1 + 1)) / nsplit;

    // ----------------------------------------------------------- prologue
    f32x4 a1[PL::S1Q], a1v[PL::RV ? PL::S1Q : 1], a2[PL::S2T * 2];
    auto load_ops = [&]() {
        if constexpr (!PL::VL) {  // (the shapes whose operands are read from L2: N = 256, 7-DoF, 256-thread)
            // buffer loads (the lane's offset in one VGPR): this also runs after each 7-DoF resync
            // (kReloadOps), where per-load 64-bit addresses held across the round loop were spilled
            const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(P.F1p), 0, (int)(frag_floats(RP, MP) * 4), 0x00020000);
            const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(P.F2p), 0, (int)(frag_floats(MP, RP) * 4), 0x00020000);
            const int vo = lane * 16;
#pragma unroll
            for (int i = 0; i < PL::S1Q; ++i) {
                a1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (has1 && kq0 + i < kq1) a1[i] = ld_frag(r1, vo, ((tile1 * KQ1 + kq0 + i) * 64) * 16);
                if constexpr (PL::RV) {
                    a1v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (has1 && kq0 + i < kq1) a1v[i] = ld_frag(r1, vo, ((tile1 * KQ1 + KQa + kq0 + i) * 64) * 16);
                }
            }
#pragma unroll
            for (int j = 0; j < PL::S2T; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a2[j * 2 + i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const int tile = wave + j * nwaves;
                    if (tile < MT2 && i < KQ2) a2[j * 2 + i] = ld_frag(r2, vo, ((tile * KQ2 + i) * 64) * 16);
                }
        } else {
            const f32x4* g1 = reinterpret_cast<const f32x4*>(P.F1p);
            const f32x4* g2 = reinterpret_cast<const f32x4*>(P.F2p);
#pragma unroll
            for (int i = 0; i < PL::S1Q; ++i) {
                a1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (has1 && kq0 + i < kq1) a1[i] = g1[((size_t)tile1 * KQ1 + kq0 + i) * 64 + lane];
                if constexpr (PL::RV) {
                    a1v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (has1 && kq0 + i < kq1) a1v[i] = g1[((size_t)tile1 * KQ1 + KQa + kq0 + i) * 64 + lane];
                }
            }
#pragma unroll
            for (int j = 0; j < PL::S2T; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a2[j * 2 + i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const int tile = wave + j * nwaves;
                    if (tile < MT2 && i < KQ2) a2[j * 2 + i] = g2[((size_t)tile * KQ2 + i) * 64 + lane];
                }
        }
    };
    if constexpr (!PL::DENSE) load_ops();  // (DENSE: every operator fragment streamed from L2 in its stage)
    // The endpoint velocity rows b'[0], b'[N−1] (stage 1's operator Fᵀ has zero columns there, so that a
    // sparse round can skip the velocity half) enter y'' through one more MFMA per stage-1 row tile, on
    // the split-0 units: k = 0 ↔ b'[0], k = 1 ↔ b'[N−1], k = 2, 3 zero.  A = the operator's endpoint
    // columns Fᵀ[r][NK], Fᵀ[r][NK + N − 1] (F_bot rows 0 and N − 1), held in one VGPR for the launch;
    // B = the trajectory's compact copy of the two rows (EPt, column cl = t·D + k).  Stage 2 then sees
    // them in y'' like every other row: the direction F·(y'' + z), G = V_R·y'' and the BLS norms need no
    // endpoint terms of their own.
    const bool hasep = has1 && sp1 == 0;  // wave-uniform
    float aep = 0.f;
    if (hasep && (lane >> 4) < 2) aep = P.Fbot[(size_t)((lane >> 4) ? N - 1 : 0) * RP + tile1 * 16 + (lane & 15)];
    // this lane's B address: column cl of trajectory cl / D, row k = lane >> 4 (a zero slot for k ≥ 2)
    const int epoff = (lane >> 4) < 2 ? LX.ep + (cl / D) * 2 * kEpS + (lane >> 4) * kEpS + cl % D : LX.ep0;
    // the 7-DoF BLS flow forms it again at its use (held across the round loop it was spilled)
    auto ep_at = [&]() {
        if constexpr (PL::kEpAtUse) {
            int l = lane;
            asm volatile("" : "+v"(l));
            const int c = l & 15;
            return (l >> 4) < 2 ? LX.ep + (c / D) * 2 * kEpS + (l >> 4) * kEpS + c % D : LX.ep0;
        } else {
            return epoff;
        }
    };
    if constexpr (PL::VL) {
        const int nv = (int)frag_floats(RP, NK) / 4;  // = frag_floats(NK, RP) / 4
        const f32x4* gt = reinterpret_cast<const f32x4*>(P.VTp);
        const f32x4* gn = reinterpret_cast<const f32x4*>(P.VNp);
        f32x4* lt = reinterpret_cast<f32x4*>(smem + LX.vt);
        f32x4* ln = reinterpret_cast<f32x4*>(smem + LX.vn);
        for (int e = tid; e < nv; e += P.BT) {
            lt[e] = gt[e];
            ln[e] = gn[e];
        }
    }
    for (int e = tid; e < 16 * lde; e += P.BT) Eb[e] = 0.f;  // no pending residual; rows ≥ N stay 0 (BLS: α rows)
    if constexpr (PL::BLS)
        for (int e = tid; e < kMaxTraj * kTsW; e += P.BT) smem[LX.ts + e] = 0.f;  // no slot in a line search yet
    for (int e = tid; e < kMaxTraj * 2 * kEpS + 4; e += P.BT) smem[LX.ep + e] = 0.f;  // + the zero word
    stage_obstacles(P, tb0, ntb, obsL);
    stage_alpha<D>(P, tb0, ntb, X, NK);
    if (tid < 2) fw[tid] = 0u;
    // J for the resyncs' exact evaluations (eval_exact's Jm), in the head's parameter block
    float* Jl = smem + H.cold + C_J;
    if (tid < D * D) Jl[tid] = P.J[tid];
    __syncthreads();
    // the reference's α (fp32, this lane's waypoint rows) and T0 = (K·α0)·J, V0 = (dK·α0)·J
    float q[WPL][D], v[WPL][D], al[WPL][D];
    float s[D], g[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        s[k] = tvalid ? P.start[b * D + k] : 0.f;
        g[k] = tvalid ? P.goal[b * D + k] : 0.f;
    }
    float epf[WPL], tg[WPL][D];  // start/goal rows of the gradient inputs, per lane
    unsigned long long endm[WPL];  // the wave's endpoint-row lanes
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        epf[j] = (nn[j] == 0 || nn[j] == N - 1) ? 1.f : 0.f;
        // opaque to the compiler: tests of epf stay one compare (it otherwise re-derives the nested
        // n == 0 / n == N − 1 tests from the select, an exec-mask cascade of ≈ 20 scalar instructions)
        asm volatile("" : "+v"(epf[j]));
        endm[j] = __ballot(epf[j] != 0.f);
#pragma unroll
        for (int k = 0; k < D; ++k) tg[j][k] = (nn[j] == N - 1) ? g[k] : s[k];
    }
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            q[j][k] = v[j][k] = 0.f;
            al[j][k] = vl[j] ? X[nn[j] * kLd + t * D + k] : 0.f;
            // BLS: the α rows the trial stages read (written with every accepted trial)
            if (PL::BLS && vl[j]) Eb[(t * D + k) * lde + swz(nn[j], t * D + k)] = al[j][k];
        }
        if (vl[j]) {
            eval_exact<D>(P, X + t * D, nn[j], q[j], v[j]);
            if (rec) {  // series frame 0: the initial trajectory
#pragma unroll
                for (int k = 0; k < D; ++k) P.series[(b * P.max_series) * N * D + nn[j] * D + k] = q[j][k];
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < MP * kLd; e += P.BT) X[e] = 0.f;
    const float* obs = obsL + (P.obs_stride ? t * obs_pitch(P.O) : 0);  // (a helper round: t*'s)
    // (PL::OREG) 9-12 obstacles (the reference's 11): the padded table in VGPRs for the whole launch
    f32x4 oreg[PL::OREG ? 6 : 1];
    const bool obs_reg = ((P.O + 3) >> 2) == 3;
#pragma unroll
    for (int i = 0; i < (PL::OREG ? 6 : 1); ++i) oreg[i] = obs_reg ? reinterpret_cast<const f32x4*>(obs)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    // replicated per-trajectory state
    float lsg = P.lsg0, ljl = P.ljl0;
    float lr = PL::BLS ? P.bls_lr0 : P.gd_lr[0];
    float cfac = P.gd_c[0];  // GD: fp32(1 − λ_reg·lr) of the outer iteration
    float gnorm = 1.f, anorm = 0.f;  // BLS: ‖G‖ and alpha_norm of the current direction
    int outer = 0, inner = 0, trial = 0;
    int phase = tvalid ? LP_STEP : LP_DONE;
    bool needs_dir = false, xdense = false;
    const float nilr = -1.f / fmaxf(lr, kMinRefStep);  // GD single loop: e' = −e/lr (the dual loop recomputes per outer)

    // evaluation of (q2, v2) with this trajectory's waves: wave partials + endpoint rows
    auto evaluate = [&](const float (&q2)[WPL][D], const float (&v2)[WPL][D], bool ext, float ljl_e,
                        WP<D> (&w)[WPL]) {
        float cvs[WPL], us = 0.f, tx = -INFINITY, tn = INFINITY, va = 0.f;
        const LeanW cw = lean_weights(P, ljl_e);
        // every lane of an evaluating trajectory holds waypoints when N fills whole waves (only valid
        // trajectories evaluate): the liveness selects of the reductions fold away
        bool lv[WPL];
#pragma unroll
        for (int j = 0; j < WPL; ++j) lv[j] = PL::kAllLive || vl[j];
        if constexpr (PL::kEvalPair) {  // both waypoints' obstacle terms in one pass (vl[0] = vl[1] = tvalid here)
            if (tvalid) {
                eval_waypoint<D, false, false, true>(P, q2[0], v2[0], obs, w[0]);
                eval_waypoint<D, false, false, true>(P, q2[1], v2[1], obs, w[1]);
                potential_pair<D>(P, obs, w[0], w[1]);
            }
        }
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
            if (PL::kEvalOne && lv[j]) eval_waypoint<D, false, true, true>(P, q2[j], v2[j], obs, w[j], PL::OREG ? oreg : nullptr);  // oreg: read only when nq == 3
            cvs[j] = w[j].cv;
            const float u = fmaf(cw.c_mean, w[j].cv, cw.c_pen * (w[j].jp + w[j].jv));
            if (j == 0) {
                us = u;
                tx = w[j].tx;
                tn = w[j].tn;
                va = w[j].va;
            } else if (vl[j]) {
                us += u;
                tx = fmaxf(tx, w[j].tx);
                tn = fminf(tn, w[j].tn);
                va = fmaxf(va, w[j].va);
            }
        }
        IRM_STAMP(6);
        ered_store_wpl<WPL>(lv, cvs, us, tx, tn, va, ext, n0, PL::NWL, red, wave);
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
            const int n = nn[j];
            if (lv[j] && epf[j] != 0.f) {  // trajectory.py:183-204 rows 0 and N−1 (epf: one compare, no cascade)
                float a = 0.f, bb = 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const float e = q2[j][d] - tg[j][d];  // tg: s on row 0, g on row N − 1
                    a = fmaf(e, e, a);
                    bb = fmaf(v2[j][d], v2[j][d], bb);
                }
                sg[t * 4 + (n == 0 ? 0 : 2)] = a;
                sg[t * 4 + (n == 0 ? 1 : 3)] = bb;
            }
        }
    };
    struct Fin {
        float nl, tx, tn, va, a0, b0, a1, b1;
        int idx;
    };
    // (PL::kLatF: the latency-hiding batch of the records and start/goal terms, below)
    auto finalize = [&](float lsg_e, int ft) {  // ft: the trajectory slot whose records are read
        if constexpr (!PL::kLatF) {
            const float* r0 = red + (ft * PL::WPTL) * 8;
            float cmax = r0[0];
            int cidx = __float_as_int(r0[1]);
            float usum = r0[2], tx = r0[3], tn = r0[4], va = r0[5];
            for (int ww = 1; ww < PL::WPTL; ++ww) {
                const float* rw = red + (ft * PL::WPTL + ww) * 8;
                amax_step(cmax, cidx, rw[0], __float_as_int(rw[1]));
                usum += rw[2];
                tx = fmaxf(tx, rw[3]);
                tn = fminf(tn, rw[4]);
                va = fmaxf(va, rw[5]);
            }
            Fin f;
            f.a0 = sg[ft * 4 + 0];
            f.b0 = sg[ft * 4 + 1];
            f.a1 = sg[ft * 4 + 2];
            f.b1 = sg[ft * 4 + 3];
            const float sgpc = fmaf(0.5f, f.a0, 0.5f * f.a1);  // trajectory.py:187
            const float sgvc = fmaf(0.5f, f.b0, 0.5f * f.b1);  // trajectory.py:203
            f.nl = fmaf(lsg_e, sgpc + sgvc, fmaf(P.lam_max, cmax, usum));
            f.idx = cidx;
            f.tx = tx;
            f.tn = tn;
            f.va = va;
            return f;
        }
        // every wave record and the start/goal terms are read before the first use (one LDS round trip;
        // the argmax merge as selects, so no read is sunk into a branch)
        float rr[PL::WPTL][6], sgr[4];
#pragma unroll
        for (int ww = 0; ww < PL::WPTL; ++ww)
#pragma unroll
            for (int e = 0; e < 6; ++e) rr[ww][e] = red[(ft * PL::WPTL + ww) * 8 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) sgr[e] = sg[ft * 4 + e];
        __builtin_amdgcn_sched_barrier(0);
        float cmax = rr[0][0];
        int cidx = __float_as_int(rr[0][1]);
        float usum = rr[0][2], tx = rr[0][3], tn = rr[0][4], va = rr[0][5];
#pragma unroll
        for (int ww = 1; ww < PL::WPTL; ++ww) {
            const float ov = rr[ww][0];
            const int oi = __float_as_int(rr[ww][1]);
            const bool take = (ov > cmax) | ((ov == cmax) & (oi < cidx));  // amax_step (no short-circuit branch)
            cmax = take ? ov : cmax;
            cidx = take ? oi : cidx;
            usum += rr[ww][2];
            tx = fmaxf(tx, rr[ww][3]);
            tn = fminf(tn, rr[ww][4]);
            va = fmaxf(va, rr[ww][5]);
        }
        Fin f;
        f.a0 = sgr[0];
        f.b0 = sgr[1];
        f.a1 = sgr[2];
        f.b1 = sgr[3];
        const float sgpc = fmaf(0.5f, f.a0, 0.5f * f.a1);  // trajectory.py:187
        const float sgvc = fmaf(0.5f, f.b0, 0.5f * f.b1);  // trajectory.py:203
        // the same value in every lane (LDS broadcasts): as a scalar, the loss and the step decisions
        // built on it are wave-uniform to the compiler too (scalar branches, the loss in an SGPR)
        f.nl = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(
                                             __builtin_bit_cast(int, fmaf(lsg_e, sgpc + sgvc, fmaf(P.lam_max, cmax, usum)))));
        f.idx = cidx;
        f.tx = tx;
        f.tn = tn;
        f.va = va;
        return f;
    };
    // gradient inputs at (q2, v2), mixed by Jᵀ, into X; returns "b' non-zero away from the endpoints"
    auto grad_inputs = [&](const WP<D> (&w)[WPL], const float (&q2)[WPL][D], const float (&v2)[WPL][D], int cidx,
                           float lsg_e, float ljl_e, int gt) {  // gt: the trajectory slot whose X columns are written
        float* EPg = EPt + (gt - t) * 2 * kEpS;
        unsigned long long bfar = 0ull;  // lanes with b' ≠ 0 (as ballots of the compares: no boolean in a VGPR)
        const LeanW cw = lean_weights(P, ljl_e);
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
            const int n = nn[j];
            if (wl[j]) {  // (valid trajectories only)
                float a[D], bb[D], ep[D];
                grad_waypoint_lean<D>(P, w[j], q2[j], v2[j], n == cidx, epf[j] * lsg_e, cw, tg[j], a, bb);
                const bool endrow = epf[j] != 0.f;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    float ma = 0.f, mb = 0.f;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        ma = fmaf(a[d], P.J[k * D + d], ma);
                        mb = fmaf(bb[d], P.J[k * D + d], mb);
                    }
                    X[(gt * D + k) * ldx + swz(n, gt * D + k)] = ma;
                    X[(gt * D + k) * ldx + NK + swz(n, gt * D + k)] = mb;
                    bfar |= __ballot(bb[k] != 0.f) & ~endm[j];
                    ep[k] = mb;
                }
                if (endrow) {  // the compact copy of the endpoint rows (read at the next round's top)
                    // (one region with a per-lane address: the nested n == 0 / n == N − 1 tests compiled to
                    // an exec-mask cascade of ≈ 20 scalar instructions on every wave)
                    const int n2 = lnd(n);  // (7-DoF: the offset formed here, not held across the round loop)
                    float* e = EPg + (n2 == 0 ? 0 : kEpS);
#pragma unroll
                    for (int k = 0; k < D; ++k) e[k] = ep[k];
                }
            }
        }
        return bfar != 0ull;
    };
    // stage 1's B operand read at the top of the round (PL::kPre1, PL::kPreW: with the velocity half), in
    // the order of its use (PL::kS1Ord)
    auto stage1_load = [&](f32x4 (&bv)[PL::KQU1], f32x4 (&bw)[PL::KQU1], float& bep) {
        const float* xl = X + cl * ldx + r4x;
        if constexpr (PL::kS1Ord) {
            // (has1 waves) the endpoint word, then the position quads in the order stage 1's chains consume
            // them, then the velocity quads: LDS returns in order, so each MFMA group waits for its own quad
            bep = smem[epoff];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < PL::KQU1; ++i) {
                bv[i] = *reinterpret_cast<const f32x4*>(xl + (kq0 + i) * 16);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < PL::KQU1; ++i) {
                bw[i] = *reinterpret_cast<const f32x4*>(xl + (KQa + kq0 + i) * 16);
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
        if (has1) {  // wave-uniform
#pragma unroll
            for (int i = 0; i < PL::KQU1; ++i) {
                bv[i] = *reinterpret_cast<const f32x4*>(xl + (kq0 + i) * 16);
                if constexpr (PL::kPreW) bw[i] = *reinterpret_cast<const f32x4*>(xl + (KQa + kq0 + i) * 16);
            }
            bep = smem[epoff];  // (a valid word on every stage-1 wave; used on the endpoint waves)
        }
    };
    // Ypart[sp] = Fᵀ·[a'; b'] over this wave's unit (+ the endpoint rows' MFMA on the split-0 units)
    auto stage1 = [&](bool full, const f32x4 (&pre)[PL::KQU1], const f32x4 (&prew)[PL::KQU1], float prep) {
        if (!has1) return;
        const float* xl = X + cl * ldx + r4x;
        auto in = [&](int i) { return PL::kFix1 ? i < PL::KQU1 : kq0 + i < kq1; };
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        f32x4 bv[PL::KQU1], bw[PL::RV ? PL::KQU1 : 1];
#pragma unroll
        for (int i = 0; i < PL::KQU1; ++i) {
            if constexpr (PL::kPre1) bv[i] = pre[i];
            else bv[i] = in(i) ? *reinterpret_cast<const f32x4*>(xl + (kq0 + i) * 16) : z4;
        }
        if constexpr (PL::RV) {
            if (full) {
#pragma unroll
                for (int i = 0; i < PL::KQU1; ++i) {
                    if constexpr (PL::kPreW) bw[i] = prew[i];
                    else bw[i] = in(i) ? *reinterpret_cast<const f32x4*>(xl + (KQa + kq0 + i) * 16) : z4;
                }
            }
        }
        f32x4 acc0 = z4, acc1 = z4;
        // fixed shapes: the second chain's first product is the endpoint MFMA's successor or starts from
        // zero itself (one MFMA result either way: no zeroed accumulator on the non-endpoint waves)
        if constexpr (PL::kFix1) {
            if (hasep) {
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(aep, PL::kPre1 ? prep : smem[ep_at()], z4, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[0][1], bv[0][1], acc1, 0, 0, 0);
            } else {
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[0][1], bv[0][1], z4, 0, 0, 0);
            }
        } else if (hasep) {
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(aep, PL::kPre1 ? prep : smem[ep_at()], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < PL::KQU1; ++i) {
            if (in(i)) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][0], bv[i][0], acc0, 0, 0, 0);
                if (!PL::kFix1 || i > 0) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][1], bv[i][1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][2], bv[i][2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i][3], bv[i][3], acc1, 0, 0, 0);
            }
        }
        if (full) {
            if constexpr (PL::RV) {
#pragma unroll
                for (int i = 0; i < PL::KQU1; ++i) {
                    if (in(i)) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][0], bw[i][0], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][1], bw[i][1], acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][2], bw[i][2], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1v[i][3], bw[i][3], acc1, 0, 0, 0);
                    }
                }
            } else if constexpr (!PL::VL) {
                // (buffer loads: the lane's offset in one VGPR, no 64-bit address held across the round loop)
                const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float*>(P.F1p), 0, (int)(frag_floats(RP, MP) * 4), 0x00020000);
                for (int kq = kq0; kq < kq1; ++kq) {
                    const f32x4 a = ld_frag(r1, lane * 16, ((tile1 * KQ1 + KQa + kq) * 64) * 16);
                    const f32x4 bb = *reinterpret_cast<const f32x4*>(xl + (KQa + kq) * 16);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bb[0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bb[1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bb[2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bb[3], acc1, 0, 0, 0);
                }
            } else {
                const f32x4* ap = reinterpret_cast<const f32x4*>(P.F1p) + ((size_t)tile1 * KQ1 + KQa) * 64 + lane;
                for (int kq = kq0; kq < kq1; ++kq) {
                    const f32x4 a = ap[(size_t)kq * 64];
                    const f32x4 bb = *reinterpret_cast<const f32x4*>(xl + (KQa + kq) * 16);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bb[0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bb[1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bb[2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bb[3], acc1, 0, 0, 0);
                }
            }
        }
        *reinterpret_cast<f32x4*>(Ypart + (sp1 * 16 + cl) * ldy + tile1 * 16 + r4x) = acc0 + acc1;
    };
    // z = V_Rᵀ·e' (the last accepted step's rounding residual) at rank 16: the residual's components
    // along singular directions 16-31 of [K; dK] are below σ_16/σ_0 ≈ 4e-4 of |L·e| ≈ 1e-4, i.e. under
    // 1e-7 per step, so only V_R's first row tile is applied (half the MFMAs of rank 32; Zp rows 16-31
    // stay zero).  zsplit k-ranges over the waves from the top down (C3: waves 4-7, idle in the Fᵀ
    // stage), operator from LDS / L2.
    // PL::kZFix (FULL launches of a fixed shape with an even split): the unit's operator and e' loads are
    // issued up front (one wait), then the MFMAs — the same accumulation order as the loop below.  The V_Rᵀ /
    // V_R fragments are held in VGPRs for the launch (PL::kVReg) or loaded at the round's top (PL::kZPre)
    f32x4 vtR[PL::kVReg ? PL::kKQZ : 1], vnR[PL::kVReg ? PL::kGT : 1][2];
    if constexpr (PL::kVReg) {
        const int sp = nwaves - 1 - wave;
#pragma unroll
        for (int i = 0; i < PL::kKQZ; ++i) vtR[i] = sp < PL::kZS ? vt_frag(sp * PL::kKQZ + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < PL::kGT; ++g) {
            const int u = nwaves - 1 - wave + g * nwaves;
            vnR[g][0] = vnR[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < PL::kMTG) {
                vnR[g][0] = vn_frag(u * KQ2);
                vnR[g][1] = vn_frag(u * KQ2 + 1);
            }
        }
    }
    auto zpre_load = [&](f32x4 (&zp)[PL::kZPre ? PL::kKQZ : 1]) {
        if constexpr (PL::kZPre) {
            const int sp = nwaves - 1 - wave;
            if (sp < PL::kZS) {
#pragma unroll
                for (int i = 0; i < PL::kKQZ; ++i) zp[i] = vt_frag(sp * PL::kKQZ + i);
            }
        }
    };
    auto stage1z = [&](const f32x4 (&zp)[PL::kZPre ? PL::kKQZ : 1]) {
        const float* el = Eb + cl * lde + r4x;
        if constexpr (PL::kZFix) {
            const int sp = nwaves - 1 - wave;
            if (sp >= PL::kZS) return;
            f32x4 a[PL::kKQZ], bb[PL::kKQZ];
#pragma unroll
            for (int i = 0; i < PL::kKQZ; ++i) {
                if constexpr (PL::kZPre) a[i] = zp[i];
                else a[i] = PL::kVReg ? vtR[i] : vt_frag(sp * PL::kKQZ + i);
                bb[i] = *reinterpret_cast<const f32x4*>(el + (sp * PL::kKQZ + i) * 16);
            }
            if constexpr (PL::kLatS) __builtin_amdgcn_sched_barrier(0);  // all loads in flight before the first MFMA
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < PL::kKQZ; ++i) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][0], bb[i][0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][1], bb[i][1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][2], bb[i][2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][3], bb[i][3], acc1, 0, 0, 0);
            }
            *reinterpret_cast<f32x4*>(Zp + (sp * 16 + cl) * ldy + r4x) = acc0 + acc1;
            return;
        }
        for (int sp = nwaves - 1 - wave; sp < zsplit; sp += nwaves) {
            const int k0 = (KQa * sp) / zsplit, k1 = (KQa * (sp + 1)) / zsplit;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            for (int kq = k0; kq < k1; ++kq) {
                const f32x4 a = vt_frag(kq);
                const f32x4 bb = *reinterpret_cast<const f32x4*>(el + kq * 16);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], bb[0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], bb[1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], bb[2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], bb[3], acc1, 0, 0, 0);
            }
            *reinterpret_cast<f32x4*>(Zp + (sp * 16 + cl) * ldy + r4x) = acc0 + acc1;
        }
    };
    // stage 2: dP = F·(Σ_s Ypart[s] + Σ_s Zp[s]) (the pending residual folded in) at rank 16 (kR16F),
    // Gb = V_R·Σ_s Ypart[s] at rank 24 (kR24): the host puts the singular components 24-31 (σ/σ_0 ≈
    // 3e-8, fp32 noise of the rank-32 factorisation) into the rank slots that MFMAs 2-3 of the second
    // k-quad read, and those MFMAs are skipped (irm_host.cpp, slot()); k_lean always runs at RP = 32.
    // The α iterate uses G (rank 24, the reference's gradient to fp32 resolution); the waypoint state
    // follows the rank-16 direction, off L·α·J by ≲ 1.5e-7 of a step per step (the one-residual lag
    // below is 1e-4), and every inner-loop end replaces it by eval_exact(α).
    // FULL launches of a fixed shape (PL::kS2Fix): the G tiles of a wave are known at compile time; their
    // operator fragments are loaded with the partial sums (in one batch: PL::kS2Batch) and their MFMAs
    // interleave with the F tiles' (same accumulation order per tile as the general form below)
    // WF: the F tiles (dP, with the residual z folded in), WG: the G tiles (Gb).  The GD flows run both in
    // one pass; the BLS flow runs G in the rounds with a new gradient input and F in every trial round
    // (its trial's own residual folded in, so the direction is the trial iterate's)
    f32x4 glY0 = f32x4{0.f, 0.f, 0.f, 0.f}, glY1 = f32x4{0.f, 0.f, 0.f, 0.f};
    // (kGLate) the G tiles, issued right after the stage-2 barrier: their MFMAs under the update /
    // evaluation's VALU work; Gb is read after the evaluation's barrier (the decision).  Issued after the
    // update instead, C3 measured +5.7 %
    auto glate_tiles = [&]() {
#pragma unroll
        for (int g = 0; g < PL::kGT; ++g) {
            const int u = nwaves - 1 - wave + g * nwaves;
            if (u < PL::kMTG) {
                const f32x4 g0 = PL::kVReg ? vnR[g][0] : vn_frag(u * KQ2);
                const f32x4 g1 = PL::kVReg ? vnR[g][1] : vn_frag(u * KQ2 + 1);
                f32x4 ag = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int m = 0; m < 4; ++m) ag = __builtin_amdgcn_mfma_f32_16x16x4f32(g0[m], glY0[m], ag, 0, 0, 0);
#pragma unroll
                for (int m = 0; m < 2; ++m) ag = __builtin_amdgcn_mfma_f32_16x16x4f32(g1[m], glY1[m], ag, 0, 0, 0);
                *reinterpret_cast<f32x4*>(Gb + cl * lde + u * 16 + r4x) = ag;
            }
        }
    };
    auto stage2f = [&](auto WFc, auto WGc) {
        constexpr bool WF = decltype(WFc)::value, WG = decltype(WGc)::value;
        f32x4 acc[PL::S2T];
#pragma unroll
        for (int j = 0; j < PL::S2T; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 ga[PL::kS2Fix ? PL::kGT : 1][2];
        if constexpr (PL::kS2Fix && WG) {
#pragma unroll
            for (int g = 0; g < PL::kGT; ++g) {
                const int u = nwaves - 1 - wave + g * nwaves;
                ga[g][0] = ga[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (u < PL::kMTG) {
                    ga[g][0] = PL::kVReg ? vnR[g][0] : vn_frag(u * KQ2);
                    ga[g][1] = PL::kVReg ? vnR[g][1] : vn_frag(u * KQ2 + 1);
                }
            }
        }
        f32x4 by[2], bt[2];
        if constexpr (PL::kS2Batch) {
            // every split-K partial of y'' and z is read before the first sum (one LDS round trip; the
            // machine scheduler otherwise reuses one register quad for the reads and waits after each,
            // seven round trips per round); same sums in the same order as the general form below
            // (the second k-quad feeds only the G tiles' MFMAs 0-1 (kR24): its rows 0-1 of each quad)
            // (read as whole quads: the swizzled layout is conflict-free for ds_read_b128, not for the
            // b64 reads the compiler narrows these to — SQ_LDS_BANK_CONFLICT 0.8 M -> 4.1 M cycles)
            constexpr int NS = S::NSPLIT;
            f32x4 yp[NS], zq[PL::kZS], yq[NS];
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) {
                yp[sp] = *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + r4y);
                yq[sp] = *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + 16 + r4y);
            }
#pragma unroll
            for (int sp = 0; sp < (WF ? PL::kZS : 0); ++sp) zq[sp] = *reinterpret_cast<const f32x4*>(Zp + (sp * 16 + cl) * ldy + r4x);
            // every quad stays whole (no narrowing, no register reuse of its unused half while in flight)
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) asm volatile("" ::"v"(yq[sp]));
#pragma unroll
            for (int g = 0; g < (WG ? PL::kGT : 0); ++g) asm volatile("" ::"v"(ga[g][1]));
            __builtin_amdgcn_sched_barrier(0);
            // the sums start from the first partial (not from +0: four adds fewer per quad; a partial
            // of −0 stays −0, which changes no MFMA product sum that is not exactly zero)
            f32x2 b1 = {yq[0].x, yq[0].y};
            by[0] = yp[0];
#pragma unroll
            for (int sp = 1; sp < NS; ++sp) {
                by[0] += yp[sp];
                b1 += f32x2{yq[sp].x, yq[sp].y};
            }
            if constexpr (PL::kS2Fix && WF && WG) {
                // the G tiles first, on y'' alone (read first), while the z partials are still in flight;
                // then the F tiles on y'' + z — each tile's MFMA chain unchanged (bit-identical; C3 −0.4 %,
                // C3 faithful −1 %)
                const f32x4 by1 = f32x4{b1.x, b1.y, 0.f, 0.f};
                f32x4 ag[PL::kGT];
                if constexpr (PL::kGLate) {
                    glY0 = by[0];
                    glY1 = by1;
                }
#pragma unroll
                for (int g = 0; g < PL::kGT; ++g) {
                    ag[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (!PL::kGLate && nwaves - 1 - wave + g * nwaves < PL::kMTG) {
#pragma unroll
                        for (int m = 0; m < 4; ++m) ag[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[g][0][m], by[0][m], ag[g], 0, 0, 0);
#pragma unroll
                        for (int m = 0; m < 2; ++m) ag[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[g][1][m], by1[m], ag[g], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);  // (the z sums after the G chain: it must not wait for them)
                f32x4 bz = zq[0];
#pragma unroll
                for (int sp = 1; sp < PL::kZS; ++sp) bz += zq[sp];
                const f32x4 b0 = by[0] + bz;
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int j = 0; j < PL::S2T; ++j)
                        if (wave + j * nwaves < MT2)
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2][m], b0[m], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < PL::S2T; ++j)
                    if (wave + j * nwaves < MT2)
                        *reinterpret_cast<f32x4*>(dP + cl * ldx + (wave + j * nwaves) * 16 + r4x) = acc[j];
#pragma unroll
                for (int g = 0; g < PL::kGT; ++g) {
                    const int u = nwaves - 1 - wave + g * nwaves;
                    if (!PL::kGLate && u < PL::kMTG) *reinterpret_cast<f32x4*>(Gb + cl * lde + u * 16 + r4x) = ag[g];
                }
                return;
            }
            if constexpr (WF) {
                f32x4 bz = zq[0];
#pragma unroll
                for (int sp = 1; sp < PL::kZS; ++sp) bz += zq[sp];
                bt[0] = by[0] + bz;
            } else {
                bt[0] = by[0];
            }
            by[1] = bt[1] = f32x4{b1.x, b1.y, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < (PL::kS2Batch ? 0 : 2); ++i) {
            by[i] = bt[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < KQ2) {
                f32x4 bz = {0.f, 0.f, 0.f, 0.f};
                for (int sp = 0; sp < nsplit; ++sp)
                    by[i] += *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + i * 16 + r4y);
                if (i == 0 && WF) {  // z has rank 16: rows 0-15 only
                    for (int sp = 0; sp < zsplit; ++sp)
                        bz += *reinterpret_cast<const f32x4*>(Zp + (sp * 16 + cl) * ldy + r4x);
                }
                bt[i] = by[i] + bz;
            }
        }
        // the waypoint direction F·(y'' + z) at rank 16: F_r·y''_r ∝ σ_r², (σ_16/σ_0)² ≈ 1.5e-7 (N = 128),
        // i.e. the fp32 rounding level of the direction itself (kR16F)
        if constexpr (PL::kS2Fix) {
            f32x4 ag[PL::kGT];
#pragma unroll
            for (int g = 0; g < PL::kGT; ++g) ag[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < 4; ++m) {
#pragma unroll
                for (int j = 0; j < (WF ? PL::S2T : 0); ++j)
                    if (wave + j * nwaves < MT2)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2][m], bt[0][m], acc[j], 0, 0, 0);
#pragma unroll
                for (int g = 0; g < (WG ? PL::kGT : 0); ++g)
                    if (nwaves - 1 - wave + g * nwaves < PL::kMTG)
                        ag[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[g][0][m], by[0][m], ag[g], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)  // kR24
#pragma unroll
                for (int g = 0; g < (WG ? PL::kGT : 0); ++g)
                    if (nwaves - 1 - wave + g * nwaves < PL::kMTG)
                        ag[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[g][1][m], by[1][m], ag[g], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < (WF ? PL::S2T : 0); ++j)
                if (wave + j * nwaves < MT2)
                    *reinterpret_cast<f32x4*>(dP + cl * ldx + (wave + j * nwaves) * 16 + r4x) = acc[j];
#pragma unroll
            for (int g = 0; g < (WG ? PL::kGT : 0); ++g) {
                const int u = nwaves - 1 - wave + g * nwaves;
                if (u < PL::kMTG) *reinterpret_cast<f32x4*>(Gb + cl * lde + u * 16 + r4x) = ag[g];
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < (WF ? PL::S2T : 0); ++j) {
            if (wave + j * nwaves < MT2) {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2][m], bt[0][m], acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < (WF ? PL::S2T : 0); ++j) {
            if (wave + j * nwaves < MT2)
                *reinterpret_cast<f32x4*>(dP + cl * ldx + (wave + j * nwaves) * 16 + r4x) = acc[j];
        }
        // G tiles (waypoint rows of V_R·y''), from the top wave down
        for (int u = nwaves - 1 - wave; WG && u < MTG; u += nwaves) {
            f32x4 ag = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (i < KQ2) {
                    const f32x4 a = vn_frag(u * KQ2 + i);
#pragma unroll
                    for (int m = 0; m < (i == 1 ? 2 : 4); ++m)  // kR24
                        ag = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], by[i][m], ag, 0, 0, 0);
                }
            }
            *reinterpret_cast<f32x4*>(Gb + cl * lde + u * 16 + r4x) = ag;
        }
    };
    // ---- BLS trial stages.  A trial j of a line search is evaluated at its own fp32 iterate
    // α_j = fl(fl(c_j·α) − fl(lr_j·ĝ)) (optimizer_BLS.py:139-140): its trajectory is c_j·[T; V] − s_j·F·(y'' + z_j)·J
    // with z_j = V_Rᵀ·e'_j, e'_j = −(α_j − (c_j·α − s_j·G))/s_j the iterate's rounding residual.
    // The G-tile waves form e'_j themselves, element by element of their G tiles (the MFMA result layout
    // of a tile is the k-permuted B layout of the z MFMAs over the same 16 waypoints), and accumulate their
    // tiles' share of z_j in the same pass: no per-lane residual rows, no barrier between G, the residual
    // and z.  A round with a new direction: stage 1 → barrier → G tiles + ‖G‖ + α_j + z partials →
    // barrier → F tiles → barrier; a round that continues a line search: α_j + z partials from the stored
    // G / α rows → barrier → F tiles → barrier.  Every column's trial is its trajectory's current one (lr
    // from TS); a helper's columns take t*'s next (lr·β₋): ycl is the column whose y'', G and α the
    // lane's column reads.
    const int nzp = min(nwaves, MTG);  // z partials (one per G-tile wave)
    // (PL::kBFix, fixed shapes up to N = 128: the tiles' operands in one batch; else the per-tile loop)
    float* Ab = smem + LX.eb;    // BLS: α rows [column][waypoint] (Eb's place)
    float* Ajb = smem + LX.aj;   // BLS: the round's trial iterate α_j, rows [column][waypoint]
    float* Zq = smem + LX.zp;    // BLS: z partials, quad-major
    float* TS = smem + LX.ts;    // BLS: per-slot lr, ‖G‖, in-a-line-search flag
    // PL::kVRegB (V_R staged in LDS): the G-tile waves' V_R / V_Rᵀ fragments held in VGPRs for the launch
    f32x4 bvt[PL::kVRegB ? PL::kTB : 1], bvn[PL::kVRegB ? PL::kTB : 1][2];
    if constexpr (PL::kVRegB) {
#pragma unroll
        for (int g = 0; g < PL::kTB; ++g) {
            const int u = nwaves - 1 - wave + g * PL::kDW;
            bvt[g] = bvn[g][0] = bvn[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < PL::kMTG) {
                bvt[g] = vt_frag(u);
                bvn[g][0] = vn_frag(u * KQ2);
                bvn[g][1] = vn_frag(u * KQ2 + 1);
            }
        }
    }
    auto bls_gz = [&](auto freshc, bool hmr, int hsr) {  // fresh (a new direction this round): G from y''
        constexpr bool fresh = decltype(freshc)::value;
        const int pz = nwaves - 1 - wave;  // this wave's z partial; its G tiles are u = pz + g·nwaves
        if (pz >= MTG) return;             // (wave-uniform)
        const int sc = ycl / D;            // the trial's trajectory slot (t* for a helper's columns)
        // the slot's trial scalars, read with the round's first LDS batch
        const float lrs = TS[sc * kTsW + 0];
        const bool act = TS[sc * kTsW + 2] != 0.f;  // (other slots: no residual)
        const int ntl = PL::kBFix ? PL::kTB : (MTG - pz + nwaves - 1) / nwaves;
        f32x4 Gt[PL::kBFix ? PL::kTB : 1];
        // fixed shapes: every tile's α rows and V_Rᵀ fragment (and, continuing a search, its stored G) read
        // in the round's first LDS batch
        f32x4 Ap[PL::kBFix ? PL::kTB : 1], Vp[PL::kBFix ? PL::kTB : 1];
        if constexpr (PL::kBFix) {
#pragma unroll
            for (int g = 0; g < PL::kTB; ++g) {
                const int u = pz + g * PL::kDW;
                Ap[g] = Vp[g] = Gt[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (u < PL::kMTG) {
                    Ap[g] = *reinterpret_cast<const f32x4*>(Ab + ycl * lde + u * 16 + r4y);
                    Vp[g] = PL::kVRegB ? bvt[g] : vt_frag(u);
                    if constexpr (!fresh) Gt[g] = *reinterpret_cast<const f32x4*>(Gb + ycl * lde + u * 16 + r4y);
                }
            }
        }
        float gn;
        if constexpr (fresh) {
            // y'' of column ycl, ranks r4..r4+3 and 16+r4..19+r4, summed over the stage-1 splits in order
            f32x4 y0, y1;
            if constexpr (PL::kBFix) {
                f32x4 yp[S::NSPLIT], yq[S::NSPLIT], gv[PL::kTB][2];
#pragma unroll
                for (int sp = 0; sp < S::NSPLIT; ++sp) {
                    yp[sp] = *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + r4y);
                    yq[sp] = *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + 16 + r4y);
                }
#pragma unroll
                for (int g = 0; g < PL::kTB; ++g) {
                    const int u = pz + g * PL::kDW;
                    gv[g][0] = gv[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (u < PL::kMTG) {
                        gv[g][0] = PL::kVRegB ? bvn[g][0] : vn_frag(u * KQ2);
                        gv[g][1] = PL::kVRegB ? bvn[g][1] : vn_frag(u * KQ2 + 1);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                y0 = yp[0];
                y1 = yq[0];
#pragma unroll
                for (int sp = 1; sp < S::NSPLIT; ++sp) {
                    y0 += yp[sp];
                    y1 += yq[sp];
                }
                // G = V_R·y'' at rank 24 (kR24, the order of stage2f), issued before the norm's VALU work
#pragma unroll
                for (int g = 0; g < PL::kTB; ++g) {
                    Gt[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (pz + g * PL::kDW < PL::kMTG) {
#pragma unroll
                        for (int m = 0; m < 4; ++m) Gt[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[g][0][m], y0[m], Gt[g], 0, 0, 0);
#pragma unroll
                        for (int m = 0; m < 2; ++m) Gt[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[g][1][m], y1[m], Gt[g], 0, 0, 0);
                    }
                }
            } else {
                y0 = *reinterpret_cast<const f32x4*>(Ypart + ycl * ldy + r4y);
                y1 = *reinterpret_cast<const f32x4*>(Ypart + ycl * ldy + 16 + r4y);
                for (int sp = 1; sp < nsplit; ++sp) {
                    y0 += *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + r4y);
                    y1 += *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + 16 + r4y);
                }
            }
            // ‖G‖² = ‖y''‖² (V_R orthonormal) per trajectory (optimizer_BLS.py:165): the lane's 8 squares, the
            // column over its four lane rows (permlane swaps: the same sums in the same order in every lane),
            // then the slot's D columns in column order (lanes sc·D + a of row 0); every G-tile wave forms
            // the same values
            float sq = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) sq = fmaf(y0[i], y0[i], sq);
#pragma unroll
            for (int i = 0; i < 4; ++i) sq = fmaf(y1[i], y1[i], sq);
            const auto p16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(sq), __float_as_uint(sq), false, false);
            const float s2 = __uint_as_float(p16[0]) + __uint_as_float(p16[1]);
            const auto p32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s2), __float_as_uint(s2), false, false);
            const int cs = __float_as_int(__uint_as_float(p32[0]) + __uint_as_float(p32[1]));
            float g2;
            if constexpr (PL::kNormShift) {
                // the slot's D column sums by in-row shifts (the slot's columns sit in this lane's row; a
                // helper's own columns hold t*'s sums, from the same y'' columns): same adds in the same order
                // as the gather below, without its LDS round trips
                const int o = cl % D;
                const float c0 = __int_as_float(cs);
                const float r1 = __int_as_float(__builtin_amdgcn_mov_dpp(cs, 0x111, 0xF, 0xF, true));  // row_shr:1
                const float l1 = __int_as_float(__builtin_amdgcn_mov_dpp(cs, 0x101, 0xF, 0xF, true));  // row_shl:1
                if constexpr (D == 1) {
                    g2 = c0;
                } else if constexpr (D == 2) {
                    g2 = (o == 0 ? c0 : r1) + (o == 0 ? l1 : c0);
                } else {
                    const float r2 = __int_as_float(__builtin_amdgcn_mov_dpp(cs, 0x112, 0xF, 0xF, true));  // row_shr:2
                    const float l2 = __int_as_float(__builtin_amdgcn_mov_dpp(cs, 0x102, 0xF, 0xF, true));  // row_shl:2
                    const float a0 = o == 0 ? c0 : (o == 1 ? r1 : r2);
                    const float a1 = o == 0 ? l1 : (o == 1 ? c0 : r1);
                    const float a2 = o == 0 ? l2 : (o == 1 ? l1 : c0);
                    g2 = (a0 + a1) + a2;
                }
            } else {
                g2 = __int_as_float(__builtin_amdgcn_ds_bpermute((sc * D) << 2, cs));
#pragma unroll
                for (int a = 1; a < D; ++a) g2 += __int_as_float(__builtin_amdgcn_ds_bpermute((sc * D + a) << 2, cs));
            }
            gn = __builtin_amdgcn_sqrtf(g2);  // v_sqrt_f32 (≤ 1 ulp): every user reads this value (TS)
            if (pz == 0 && lane < kCols && ycl == cl && cl % D == 0) TS[(cl / D) * kTsW + 1] = gn;  // for the trajectories and the later rounds
            if constexpr (!PL::kBFix) {
                const f32x4 g0 = vn_frag(pz * KQ2), g1 = vn_frag(pz * KQ2 + 1);
                Gt[0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int m = 0; m < 4; ++m) Gt[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(g0[m], y0[m], Gt[0], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < 2; ++m) Gt[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(g1[m], y1[m], Gt[0], 0, 0, 0);
                (void)ntl;
            }
        } else {
            gn = TS[sc * kTsW + 1];
        }
        const float lrx = (hmr && cl / D == hsr) ? lrs * P.bls_bm : lrs;  // a helper: t*'s next trial (:147)
        const float cjx = unfused(1.f - unfused(P.lreg * lrx));            // optimizer_BLS.py:139
        // ĝ = G/‖G‖ (optimizer_BLS.py:165): the IEEE quotient through the correctly rounded reciprocal (div_rcp
        // with rcp_rn_of); the waypoint-space step s = lr/‖G‖ (not reference arithmetic: the residual e'
        // absorbs its rounding) through the refined one, as the trajectory lanes form it
        const float rr = rcp_refined(gn), rg = rcp_rn_of(gn, rr);
        const float sx = div_rcp(lrx, gn, rr);  // the trajectory lanes' step (the same expression there)
        const float ne = -rcp_refined(fmaxf(sx, kMinRefStep));
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        auto tile = [&](int u, f32x4 G, bool store_g, f32x4 A, f32x4 a) {  // α rows, V_Rᵀ fragment (rank tile 0)
            if (store_g) *reinterpret_cast<f32x4*>(Gb + cl * lde + u * 16 + r4x) = G;  // for the later rounds
            f32x4 AJ, E;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float gh = div_rcp(G[i], gn, rg);
#ifdef IRM_DIV_CHECK
                if (act && pz < MTG) {  // diagnostics: ĝ against the IEEE division, and round 5's refined-rcp form
                    const unsigned mis = __fdiv_rn(G[i], gn) != gh ? 1u : 0u;
                    const unsigned mis5 = __fdiv_rn(G[i], gn) != div_rcp(G[i], gn, rcp_refined(gn)) ? 1u : 0u;
                    atomicAdd(&P.prof[(size_t)blockIdx.x * kProfPhases + 0], (unsigned long long)mis);
                    atomicAdd(&P.prof[(size_t)blockIdx.x * kProfPhases + 1], (unsigned long long)mis5);
                    atomicAdd(&P.prof[(size_t)blockIdx.x * kProfPhases + 2], 1ull);
                }
#endif
                // α_j = fl(fl(c·α) − fl(lr·ĝ)) (optimizer_BLS.py:139) and its scaled residual e' = (c·α − α_j)/s − G,
                // u = fl(c·α − α_j) in one rounding (alpha_step_gd2's form: e' to 2^-24 of |G|)
                const float p1 = unfused(cjx * A[i]), p2 = unfused(lrx * gh);
                AJ[i] = unfused(p1 - p2);
                const float uu = fmaf(cjx, A[i], -AJ[i]);
                E[i] = act ? fmaf(-uu, ne, -G[i]) : 0.f;
            }
            *reinterpret_cast<f32x4*>(Ajb + cl * lde + u * 16 + r4x) = AJ;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], E[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], E[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], E[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], E[3], acc1, 0, 0, 0);
        };
        if constexpr (PL::kBFix) {
#pragma unroll
            for (int g = 0; g < PL::kTB; ++g) {
                const int u = pz + g * PL::kDW;
                if (u < PL::kMTG) tile(u, Gt[g], fresh, Ap[g], Vp[g]);
            }
        } else {
            for (int u = pz; u < MTG; u += nwaves) {
                f32x4 G;
                if (fresh && u == pz) {
                    G = Gt[0];
                } else if (fresh) {  // further tiles of the wave (general launches)
                    const f32x4 g0 = vn_frag(u * KQ2), g1 = vn_frag(u * KQ2 + 1);
                    f32x4 y0 = *reinterpret_cast<const f32x4*>(Ypart + ycl * ldy + r4y);
                    f32x4 y1 = *reinterpret_cast<const f32x4*>(Ypart + ycl * ldy + 16 + r4y);
                    for (int sp = 1; sp < nsplit; ++sp) {
                        y0 += *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + r4y);
                        y1 += *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + 16 + r4y);
                    }
                    G = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int m = 0; m < 4; ++m) G = __builtin_amdgcn_mfma_f32_16x16x4f32(g0[m], y0[m], G, 0, 0, 0);
#pragma unroll
                    for (int m = 0; m < 2; ++m) G = __builtin_amdgcn_mfma_f32_16x16x4f32(g1[m], y1[m], G, 0, 0, 0);
                } else {
                    G = *reinterpret_cast<const f32x4*>(Gb + ycl * lde + u * 16 + r4y);
                }
                tile(u, G, fresh, *reinterpret_cast<const f32x4*>(Ab + ycl * lde + u * 16 + r4y),
                     vt_frag(u));
            }
        }
        *reinterpret_cast<f32x4*>(Zq + pz * 256 + (r4 >> 2) * 64 + cl * 4) = acc0 + acc1;
    };
    // the F tiles of every column's trial: dP = F·(y'' + Σ_w z partial w) at rank 16 (kR16F)
    auto bls_f = [&]() {
        const float* zq = Zq + (r4 >> 2) * 64 + cl * 4;
        f32x4 by0, bz;
        if constexpr (PL::kBFix) {  // every partial read before the first sum (one LDS round trip)
            f32x4 yp[S::NSPLIT], zz[PL::kNZc];
#pragma unroll
            for (int sp = 0; sp < S::NSPLIT; ++sp) yp[sp] = *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + r4y);
#pragma unroll
            for (int w = 0; w < PL::kNZc; ++w) zz[w] = *reinterpret_cast<const f32x4*>(zq + w * 256);
            __builtin_amdgcn_sched_barrier(0);
            by0 = yp[0];
#pragma unroll
            for (int sp = 1; sp < S::NSPLIT; ++sp) by0 += yp[sp];
            bz = zz[0];
#pragma unroll
            for (int w = 1; w < PL::kNZc; ++w) bz += zz[w];
        } else {
            by0 = *reinterpret_cast<const f32x4*>(Ypart + ycl * ldy + r4y);
            for (int sp = 1; sp < nsplit; ++sp) by0 += *reinterpret_cast<const f32x4*>(Ypart + (sp * 16 + ycl) * ldy + r4y);
            bz = *reinterpret_cast<const f32x4*>(zq);
            for (int w = 1; w < nzp; ++w) bz += *reinterpret_cast<const f32x4*>(zq + w * 256);
        }
        const f32x4 bt = by0 + bz;
        f32x4 acc[PL::S2T];
#pragma unroll
        for (int j = 0; j < PL::S2T; ++j) {
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (wave + j * nwaves < MT2) {
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j * 2][m], bt[m], acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < PL::S2T; ++j)
            if (wave + j * nwaves < MT2) *reinterpret_cast<f32x4*>(dP + cl * ldx + (wave + j * nwaves) * 16 + r4x) = acc[j];
    };
    // ---- the dense operator (DENSE: DenseShape, F = L = [K; dK], V_R = I — G is y'' and z is e').
    // Stage 1, y'' = Fᵀ·[a'; b']: the N/16 row tiles of y'' over the waves, each over the whole k range
    // (the position half; the velocity half in dense rounds) plus the endpoint velocity rows' MFMA (as the
    // rank-32 kernel's split-0 units).  Stage 2, dP = F·(y'' + e'): the MP/16 row tiles of [T; V] over the
    // waves, the B operand one quad of y'' + e' per k-quad from LDS.  Every operator fragment (Fᵀ, F:
    // 512 KB each at N = 256) is streamed from L2 kDPF k-quads ahead of its MFMAs; a sched_barrier per
    // k-quad keeps the compiler from hoisting the whole stream (its registers) up front.
    float aepd[PL::kD1];  // F_bot rows 0 / N−1 of the wave's stage-1 row tiles (the endpoint MFMA's A)
#pragma unroll
    for (int j = 0; j < PL::kD1; ++j) {
        const int tl = wave + j * PL::kDW;
        aepd[j] = 0.f;
        if (PL::DENSE && tl < RP / 16 && (lane >> 4) < 2) aepd[j] = P.Fbot[(size_t)((lane >> 4) ? N - 1 : 0) * RP + tl * 16 + (lane & 15)];
    }
    auto dense_stage1 = [&](bool full) {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        constexpr int KQ1c = S::MP / 16;
        const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(P.F1p), 0, (int)(frag_floats(S::RP, S::MP) * 4), 0x00020000);
        const int vo = lane * 16;
        auto g1ld = [&](int tl, int kq) { return ld_frag(r1, vo, ((tl * KQ1c + kq) * 64) * 16); };
        const float* xl = X + cl * ldx + r4x;
        const float bep = smem[epoff];
        f32x4 acc[PL::kD1];
#pragma unroll
        for (int j = 0; j < PL::kD1; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(aepd[j], bep, z4, 0, 0, 0);
        auto half = [&](int kb) {  // k-quads kb … kb + kDQ − 1 of Fᵀ's MP columns
            f32x4 a[PL::kDPF][PL::kD1], b[PL::kDPF];
#pragma unroll
            for (int p = 0; p < PL::kDPF; ++p) {
#pragma unroll
                for (int j = 0; j < PL::kD1; ++j) a[p][j] = g1ld(wave + j * PL::kDW, kb + p);
                b[p] = *reinterpret_cast<const f32x4*>(xl + (kb + p) * 16);
            }
#pragma unroll
            for (int kq = 0; kq < PL::kDQ; ++kq) {
                const int sl = kq % PL::kDPF;
                f32x4 ac[PL::kD1];
#pragma unroll
                for (int j = 0; j < PL::kD1; ++j) ac[j] = a[sl][j];
                const f32x4 bc = b[sl];
                if (kq + PL::kDPF < PL::kDQ) {
#pragma unroll
                    for (int j = 0; j < PL::kD1; ++j) a[sl][j] = g1ld(wave + j * PL::kDW, kb + kq + PL::kDPF);
                    b[sl] = *reinterpret_cast<const f32x4*>(xl + (kb + kq + PL::kDPF) * 16);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int j = 0; j < PL::kD1; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[j][m], bc[m], acc[j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        half(0);
        if (full) half(PL::kDQ);
#pragma unroll
        for (int j = 0; j < PL::kD1; ++j)
            *reinterpret_cast<f32x4*>(Ypart + cl * ldy + (wave + j * PL::kDW) * 16 + r4x) = acc[j];
    };
    auto dense_stage2 = [&]() {
        constexpr int KQ2c = S::RP / 16;
        const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(P.F2p), 0, (int)(frag_floats(S::MP, S::RP) * 4), 0x00020000);
        const int vo = lane * 16;
        auto g2ld = [&](int tl, int kq) { return ld_frag(r2, vo, ((tl * KQ2c + kq) * 64) * 16); };
        const float* yl = Ypart + cl * ldy + r4x;
        const float* el = Eb + cl * lde + r4x;
        f32x4 acc[PL::kD2], a[PL::kDPF][PL::kD2], by[PL::kDPF], be[PL::kDPF];
#pragma unroll
        for (int j = 0; j < PL::kD2; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < PL::kDPF; ++p) {
#pragma unroll
            for (int j = 0; j < PL::kD2; ++j) a[p][j] = g2ld(wave + j * PL::kDW, p);
            by[p] = *reinterpret_cast<const f32x4*>(yl + p * 16);
            be[p] = *reinterpret_cast<const f32x4*>(el + p * 16);
        }
#pragma unroll
        for (int kq = 0; kq < PL::kDQ; ++kq) {
            const int sl = kq % PL::kDPF;
            f32x4 ac[PL::kD2];
#pragma unroll
            for (int j = 0; j < PL::kD2; ++j) ac[j] = a[sl][j];
            const f32x4 bt = by[sl] + be[sl];  // y'' + e' (z = V_Rᵀ·e' = e')
            if (kq + PL::kDPF < PL::kDQ) {
#pragma unroll
                for (int j = 0; j < PL::kD2; ++j) a[sl][j] = g2ld(wave + j * PL::kDW, kq + PL::kDPF);
                by[sl] = *reinterpret_cast<const f32x4*>(yl + (kq + PL::kDPF) * 16);
                be[sl] = *reinterpret_cast<const f32x4*>(el + (kq + PL::kDPF) * 16);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int j = 0; j < PL::kD2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[j][m], bt[m], acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < PL::kD2; ++j)
            *reinterpret_cast<f32x4*>(dP + cl * ldx + (wave + j * PL::kDW) * 16 + r4x) = acc[j];
    };
    // this lane's direction rows Δ = (F·y'')·J for waypoint j (the endpoint velocity rows are in y'')
    auto direction = [&](int j, float (&dt)[D], float (&dv)[D]) {
        float ut[D], uv[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            ut[k] = dP[(t * D + k) * ldx + swz(nn[j], t * D + k)];
            uv[k] = dP[(t * D + k) * ldx + NK + swz(nn[j], t * D + k)];
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            float a = ut[0] * P.J[k], c = uv[0] * P.J[k];
#pragma unroll
            for (int l = 1; l < D; ++l) {
                a = fmaf(ut[l], P.J[l * D + k], a);
                c = fmaf(uv[l], P.J[l * D + k], c);
            }
            dt[k] = a;
            dv[k] = c;
        }
    };
    // G[n] = (V_R·y'')[n] (no mix: [a'; b'] carry Jᵀ; the endpoint velocity rows are in y'')
    auto grad_alpha = [&](int j, float (&G)[D], int gt) {  // gt: the trajectory slot whose G is read
        const int r = wl[j] ? nn[j] : 0;  // (valid trajectories only)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if constexpr (PL::DENSE) G[k] = Ypart[(gt * D + k) * ldy + swz(r, gt * D + k)];  // V_R = I: G = y''
            else G[k] = Gb[(gt * D + k) * lde + swz(r, gt * D + k)];
        }
    };
    // a lane's row offset in a series frame, formed where it is used (a value held across the round loop
    // is a per-lane 64-bit address the 7-DoF dual loop spilled)
    auto ser_row = [&](int j) {
        int r = nn[j] * D;
        if constexpr (PL::kLaunder) asm volatile("" : "+v"(r));
        return r;
    };
    auto snapshot = [&](irm_stats& st) {  // extended-vis frame after a non-breaking inner iteration
        if (rec && st.series_len < P.max_series) {
#pragma unroll
            for (int j = 0; j < WPL; ++j) {
                if (vl[j]) {
#pragma unroll
                    for (int k = 0; k < D; ++k)
                        P.series[((b * P.max_series) + st.series_len) * N * D + ser_row(j) + k] = q[j][k];
                }
            }
            st.series_len++;
        }
    };

    // ---- BLS line-search helpers (PL::kHelp): when one trajectory t* of the workgroup is left in a
    // line search, the first done slot evaluates its next trial (lr·β₋, optimizer_BLS.py:143-147) in the
    // same round: a rejected trial changes nothing but lr, so the sequential search's decisions, counters
    // and log are unchanged — only rounds are saved.  The helper reads t*'s α, T, V rows (ss, written by
    // t* whenever they change) and scalars (hp, every round); its trial's direction folds its own residual
    // into t*'s y'' (stage 2 reads t*'s Ypart columns for the helper's columns); every wave of both slots
    // replays the decision; if the helper's trial is the accepted one, the helper writes t*'s gradient
    // inputs and α, T, V, which t* adopts at the next round's start.
    float* SS = smem + LX.ss;  // [3·D][MAXT]: α, T, V of the thread's waypoint
    float* HP = smem + LX.hp;  // [slot][kHpW]: lr, ljl, lsg, loss, trial, inner, bfar (per wave of the slot)
    auto ss_write = [&](int tt, const float (&a)[WPL][D], const float (&qq)[WPL][D], const float (&vv)[WPL][D]) {
        const int th = tt * PL::NWL + li;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            SS[k * MAXT + th] = a[0][k];
            SS[(D + k) * MAXT + th] = qq[0][k];
            SS[(2 * D + k) * MAXT + th] = vv[0][k];
        }
    };
    auto ss_read = [&](int tt) {
        const int th = tt * PL::NWL + li;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            al[0][k] = SS[k * MAXT + th];
            q[0][k] = SS[(D + k) * MAXT + th];
            v[0][k] = SS[(2 * D + k) * MAXT + th];
        }
    };
    bool adopt = false;  // t*: the helper's trial was accepted — take its α, T, V at the next round's start
    bool qpend = false;  // QUE: this slot took a queue index at the end of the previous round (wave-uniform)
    // BLS: this trajectory's trial scalars for the trial stages (lr of its next trial, in a line search)
    auto ts_write = [&]() {
        if (n0 == 0 && lane == 0) {
            TS[t * kTsW + 0] = lr;
            TS[t * kTsW + 2] = phase == LP_STEP ? 1.f : 0.f;
            if constexpr (PL::kQueue) TS[t * kTsW + 3] = __int_as_float((int)b);  // the slot's problem, for a helper
        }
    };
    int n_rounds = 0, n_hm = 0;  // diagnostics (trace_b bit 29): kernel rounds / helper rounds until this trajectory ended

    // round 0 (optimizer_GD.py:93 / :210: the loss at α0) and the first gradient inputs
    irm_stats st{};
    st.series_len = rec ? 1 : 0;
    // BLS: the per-trajectory counters in VGPRs
    if constexpr (PL::kStatVgpr) {
        asm volatile("" : "+v"(st.inner_iterations), "+v"(st.outer_iterations), "+v"(st.grad_evals), "+v"(st.cost_evals),
                     "+v"(st.bls_trials), "+v"(st.series_len), "+v"(n_rounds), "+v"(n_hm));
    }
    auto write_out = [&]() {  // this trajectory's outputs: T, α, counters
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
            if (vl[j]) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    if (P.traj_out) P.traj_out[(b * N + nn[j]) * D + k] = q[j][k];
                    if (P.alpha_out) P.alpha_out[(b * N + nn[j]) * D + k] = al[j][k];
                }
            }
        }
        if (P.stats && li == 0) P.stats[b] = st;
    };

    float loss;
    bool done = !tvalid;
    {
        WP<D> w[WPL];
        evaluate(q, v, false, ljl, w);
        __syncthreads();
        const Fin f = finalize(lsg, t);
        loss = f.nl;
        if constexpr (!PL::BLS) st.cost_evals = 1;
        bool to_end = P.max_inner <= 0;
        // BLS with max_outer_iteration <= 0: the outer while_loop never runs and α0 is returned
        // (optimizer_BLS.py:184-186, 210-213): straight to the constraint check
        if constexpr (PL::BLS) to_end = to_end || P.max_outer <= 0;
        bool bfar = false;
        if constexpr (PL::GD1) {
            if (to_end) done = true;
        } else if (to_end) {
            // (a slot without a problem stays LP_DONE: as LP_RESYNC it would run the constraint round, end it and —
            // QUE — claim a problem from the queue, which its tvalid-guarded write_out then never writes out)
            if (tvalid) {
                phase = LP_RESYNC;
                st.final_loss = loss;
            }
        } else {
            needs_dir = true;
        }
        if (!done && !to_end) {
            bfar = grad_inputs(w, q, v, f.idx, lsg, ljl, t);
            xdense = bfar;
        }
        if constexpr (PL::BLS) {
            if (tvalid) ts_write();
        }
        if constexpr (PL::kHelp) {
            if (tvalid) {
                if (n0 == 0 && lane == 0) {
                    HP[t * kHpW + 0] = lr;
                    HP[t * kHpW + 1] = ljl;
                    HP[t * kHpW + 2] = lsg;
                    HP[t * kHpW + 3] = loss;
                    HP[t * kHpW + 4] = __int_as_float(0);
                    HP[t * kHpW + 5] = __int_as_float(0);
                }
            }
        }
        if constexpr (PL::GD1) {
            if (lane == 0 && (!done || bfar)) atomicOr(&fw[0], (done ? 0u : 1u << wave) | (bfar ? 1u << 31 : 0u));
        } else {
            if (lane == 0 && tvalid)
                atomicOr(&fw[0], (1u << wave) | (needs_dir ? 1u << 28 : 0u) | (phase == LP_RESYNC ? 1u << 29 : 0u) |
                                     (phase == LP_STEP ? 1u << 30 : 0u) |
                                     ((PL::BLS ? xdense && phase == LP_STEP : bfar) ? 1u << 31 : 0u));
        }
    }
    __syncthreads();

    IRM_STAMP(14);
    // ---------------------------------------------------------- rounds
    // The second half of the waves (4-7: the younger partner on each SIMD) loses VALU arbitration to
    // the older one in every phase; static priority for that half (MI355X_MICROARCH.md, two waves per
    // SIMD, item 4): C3 +1.7 %.  Priority only reorders issue: results are unchanged.
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    // ---- the all-live loop (C3's kernel, kTopC3).  A workgroup whose every slot holds a problem runs its
    // rounds here up to and including the first in which one of its trajectories stops (a rejected step, or
    // max_inner reached); the loop below takes over from there, and runs a ragged batch's last, partial
    // workgroup from the start.  Same stages, LDS layout, MFMA chains and per-lane arithmetic as a round of
    // the loop below with every trajectory stepping (bit-identical, tests/test_gpu_gd1_fastpath.py); what the
    // round no longer carries: the done / stepping tests and the waypoint-state copies behind them, the
    // wave-role tests inside the stages (stage-1 waves and z waves take one branch each), the per-round
    // counters (one round count per wave, added to the statistics at the exit), the flag word's decoding
    // beyond "all eight wave bits set" (a stopped trajectory's waves leave theirs unset: the stop bit) and
    // the three compares of b' for the dense bit (the evaluation's velocity masks zvm decide it: b' = k_vel·zvm
    // away from the endpoints, and a dense round where b' is zero adds exact zeros).
    // The hand-over is the flag word itself: the loop below reads the word this loop declined.
    int par0 = 0;
    if constexpr (PL::kTopC3) {
        if (ntb == PL::kSlots) {  // workgroup-uniform: every slot holds a problem
            const unsigned wbit = 1u << wave;
            const LeanW cw = lean_weights(P, ljl);
            const f32x4 zpre[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};  // (kVReg: the z unit's fragments are in vtR)
            float llr = P.llr;  // (held in a register: the decision does not wait for a kernel-argument load)
            asm volatile("" : "+s"(llr));
            int rnd = 0;       // accepted steps here (a gradient and a cost evaluation each)
            bool rej = false;  // left through a rejected step (one more gradient and cost evaluation)
            int par = 0;
            for (;; par ^= 1) {
                f32x4 pre1[PL::KQU1], pre1w[PL::KQU1];
                float pre1e = 0.f;
                unsigned fl = 0u;
                const unsigned flv = fw[par];
                __builtin_amdgcn_sched_barrier(0);
                // one branch per wave role: the flag word, the exit test and the wave's stage-1 unit
                // (somebody stopped — a wave bit is missing: the loop below reads this word again)
                if (has1) {  // wave-uniform
                    stage1_load(pre1, pre1w, pre1e);
                    asm volatile("v_readfirstlane_b32 %0, %1 ; flag word, stage-1 waves (all-live)" : "=s"(fl) : "v"(flv));
                    if ((fl & PL::kAllW) != PL::kAllW) break;
                    IRM_STAMP(0);
                    IRM_COUNT(13, (fl >> 31) != 0u);
                    stage1((fl >> 31) != 0u, pre1, pre1w, pre1e);
                    // the next round's flag word (as below), by wave 0 alone under a scalar branch: behind a lane
                    // mask the store is issued, with no lane enabled, by the three other stage-1 waves as well
                    if (wave == 0) fw[par ^ 1] = 0u;
                } else {
                    asm volatile("v_readfirstlane_b32 %0, %1 ; flag word, z waves (all-live)" : "=s"(fl) : "v"(flv));
                    if ((fl & PL::kAllW) != PL::kAllW) break;
                    stage1z(zpre);
                }
                IRM_STAMP(1);
                __syncthreads();
                IRM_STAMP(2);
                stage2f(std::true_type{}, std::true_type{});
                IRM_STAMP(3);
                __syncthreads();
                IRM_STAMP(4);
                glate_tiles();
                // update + evaluate: the waypoint state moves to the trial point (a rejected step ends the trajectory)
                float q2[WPL][D], v2[WPL][D];
                WP<D> w[WPL];
                {
                    float dt[D], dv[D];
                    direction(0, dt, dv);
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        const float tq = -(lr * dt[k]), tv = -(lr * dv[k]);
                        q2[0][k] = fmaf(cfac, q[0][k], tq);
                        v2[0][k] = fmaf(cfac, v[0][k], tv);
                        asm volatile("" ::"v"(tq), "v"(tv), "v"(q2[0][k]), "v"(v2[0][k]));  // (three-address FMAs, as below)
                    }
                }
                IRM_STAMP(5);
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    q[0][k] = q2[0][k];
                    v[0][k] = v2[0][k];
                }
                evaluate(q2, v2, false, ljl, w);
                IRM_STAMP(7);
                __syncthreads();
                IRM_STAMP(8);
                // ---- decision
                float Gf[D];
                grad_alpha(0, Gf, t);
                const Fin f = finalize(lsg, t);
                IRM_STAMP(9);
                if (loss - f.nl < llr) {
                    // minimized: the step is discarded (optimizer_GD.py:87-90) and the trajectory ends with the α,
                    // loss and step count it has.  Its waves leave from here, behind the round's end barrier;
                    // their bits are missing in the next flag word, so every other wave leaves at the next top
                    rej = true;
                    par ^= 1;
                    IRM_STAMP(11);
                    __syncthreads();
                    IRM_STAMP(12);
                    break;
                } else {
                    loss = f.nl;
                    float eo[D];
#pragma unroll
                    for (int k = 0; k < D; ++k) al[0][k] = alpha_step_gd2(al[0][k], cfac, lr, Gf[k], nilr, eo[k]);
#pragma unroll
                    for (int k = 0; k < D; ++k) Eb[(t * D + k) * lde + swz(nn[0], t * D + k)] = eo[k];
                    if (rnd + 1 < P.max_inner) {  // (every round so far was a step: inner = rnd)
                        // gradient inputs at the new point (grad_inputs), the dense bit from the velocity masks
                        const int n = nn[0];
                        float a[D], bb[D], ep[D];
                        grad_waypoint_lean<D>(P, w[0], q2[0], v2[0], n == f.idx, epf[0] * lsg, cw, tg[0], a, bb);
                        unsigned zb = 0u;
#pragma unroll
                        for (int k = 0; k < D; ++k) {
                            float ma = 0.f, mb = 0.f;
#pragma unroll
                            for (int d = 0; d < D; ++d) {
                                ma = fmaf(a[d], P.J[k * D + d], ma);
                                mb = fmaf(bb[d], P.J[k * D + d], mb);
                            }
                            X[(t * D + k) * ldx + swz(n, t * D + k)] = ma;
                            X[(t * D + k) * ldx + NK + swz(n, t * D + k)] = mb;
                            zb |= __float_as_uint(w[0].zvm[k]);
                            ep[k] = mb;
                        }
                        const bool bfar = (__ballot(zb != 0u) & ~endm[0]) != 0ull;
                        if (epf[0] != 0.f) {  // the compact copy of the endpoint rows
                            float* e = EPt + (n == 0 ? 0 : kEpS);
#pragma unroll
                            for (int k = 0; k < D; ++k) e[k] = ep[k];
                        }
                        if (lane == 0) atomicOr(&fw[par ^ 1], wbit | (bfar ? 1u << 31 : 0u));
                    }
                }
                ++rnd;
                IRM_STAMP(11);
                __syncthreads();
                IRM_STAMP(12);
            }
            // the loop below continues at this parity with the state it keeps per round
            par0 = par;
            st.grad_evals += rnd + (rej ? 1 : 0);
            st.cost_evals += rnd + (rej ? 1 : 0);
            st.inner_iterations += rnd;
            inner += rnd;
            if (rej || inner >= P.max_inner) done = true;
        }
    }
    for (int par = par0;; par ^= 1) {
        f32x4 pre1[PL::KQU1], pre1w[PL::KQU1];
        f32x4 zpre[PL::kZPre ? PL::kKQZ : 1];
        zpre_load(zpre);
        float pre1e = 0.f;  // read only on the endpoint waves (hasep)
        // (the flag word read before the operand batch, so the branch need not wait for the batch: C3 even
        // to 2 % slower, not kept)
        unsigned flw = 0u;
        if constexpr (PL::kS1Ord) {
            // C3's kernel: the flag word first, then the stage-1 waves' operands in the order of their use, all
            // in one LDS queue.  The flag becomes a scalar inside each wave class's own block, so its wait
            // counts that block's later reads (lgkmcnt(9) on the stage-1 waves) instead of draining them,
            // and stage 1's MFMA groups each wait for their own quad.  X and the endpoint copy were written
            // before the round-end barrier
            const unsigned flv = fw[par];
            __builtin_amdgcn_sched_barrier(0);
            if (has1) {  // wave-uniform
                stage1_load(pre1, pre1w, pre1e);
                asm volatile("v_readfirstlane_b32 %0, %1 ; flag word, stage-1 waves" : "=s"(flw) : "v"(flv));
            } else {
                asm volatile("v_readfirstlane_b32 %0, %1 ; flag word, other waves" : "=s"(flw) : "v"(flv));
            }
        }
        if constexpr (PL::kPre1 && !PL::kS1Ord) stage1_load(pre1, pre1w, pre1e);
        const unsigned fl = PL::kS1Ord ? flw : fw[par];
        if constexpr (PL::GD1) {
            if ((fl & 0x7FFFFFFFu) == 0u) break;  // every trajectory of the block is done
        } else {
            if ((fl & 0xFFFFu) == 0u) break;
        }
        const bool dense = (fl >> 31) != 0u;
        const bool dirr = PL::GD1 || ((fl >> 28) & 1u);  // some trajectory needs a direction this round
        const bool rsy = !PL::GD1 && ((fl >> 29) & 1u);  // some trajectory ends an inner loop this round
        // (kS1Ord: cleared behind stage 1 — here the store's wait drained wave 0's operand batch)
        if constexpr (!PL::kS1Ord) {
            if (tid == 0) fw[par ^ 1] = 0u;
        }
        if constexpr (PL::kQueue) {
            // the index this slot's first wave took at the end of the previous round (its record's spare word):
            // a problem to load this round, or past the batch — the slot stays done
            if (qpend) {
                const int nx = __builtin_amdgcn_readfirstlane(__float_as_int(red[(t * PL::WPTL) * 8 + 6]));
                qpend = false;
                if (nx < P.B) {
                    b = (size_t)nx;
                    phase = LP_LOAD;
                }
            }
        }
        bool hm = false, helper = false;  // helper round (block-uniform) / this wave helps
        int ts = 0, hs = 0;               // t*, the helper slot
        float h_lr0 = 0.f, h_lr = 0.f, h_ljl = 0.f, h_lsg = 0.f, h_loss = 0.f, h_gn = 1.f, h_an = 0.f;
        int h_trial = 0, h_inner = 0;
        if constexpr (PL::kHelp) {
            n_rounds++;
            if (adopt) {  // t*: the previous round accepted the helper's trial
                ss_read(t);
                xdense = HP[t * kHpW + 6 + (wave - t * PL::WPTL)] != 0.f;
                adopt = false;
            }
            if (!rec && !P.lean_nohelp && ((fl >> 30) & 1u) && PL::kSlots > 1) {
                unsigned live = 0u;
#pragma unroll
                for (int s2 = 0; s2 < PL::kSlots; ++s2)
                    if ((fl >> (s2 * PL::WPTL)) & ((1u << PL::WPTL) - 1u)) live |= 1u << s2;
                if (__builtin_popcount(live) == 1) {
                    hm = true;
                    n_hm++;
                    ts = __builtin_ctz(live);
                    // the neighbouring slot: the other SIMD pair (slot s = waves 2s, 2s+1 → SIMDs 2s mod 4,
                    // 2s+1 mod 4 at two waves per slot), so the helper's VALU does not share t*'s SIMDs
                    hs = ts ^ 1;
                    // the helper's MFMA columns must exist: with five 3-joint trajectories per workgroup
                    // (N ≤ 64, traj_per_block = 5) slot 5 would own columns 15-17 — take the slot below t*
                    // then (ts ≥ 2 there, and slot ts − 1's columns end below t*'s)
                    if ((hs + 1) * D > kCols) hs = ts - 1;
                    helper = t == hs;
                }
            }
            ycl = (hm && cl / D == hs) ? ts * D + cl % D : cl;
            r4y = r4 ^ (ycl & 4);
            // a helper round: t*'s waves (the launch's critical path) ahead of every other wave of their SIMDs
            // (C2 0.516 -> 0.498 ms, C3-BLS faithful even; priority only reorders issue)
            if (hm) {
                if (t == ts) __builtin_amdgcn_s_setprio(3);
                else __builtin_amdgcn_s_setprio(0);
            }
            // (the helper priorities stay set in the rounds after a helper round — a lone trajectory's resync
            // rounds: t* keeps the issue lead there.  Restoring the launch's split (waves 4-7 at 1) once the helper
            // rounds end measured C3-BLS faithful +0.8 %, C2 even, and is not done; priority only reorders issue)
            // t* publishes its α, T, V for the helper at the top of each helper round (the helper reads them
            // after this round's G-tile barrier), instead of after every accepted trial of every trajectory
            if (hm && t == ts) ss_write(t, al, q, v);
            if (helper) {  // wave-uniform: t*'s state and scalars (its own trajectory is done and written out)
                // t*'s problem: its place in the launch, or (QUE) the index its slot claimed
                const size_t bs = PL::kQueue ? (size_t)__float_as_int(TS[ts * kTsW + 3]) : (size_t)(tb0 + ts);
#pragma unroll
                for (int k = 0; k < D; ++k) tg[0][k] = (nn[0] == N - 1) ? P.goal[bs * D + k] : P.start[bs * D + k];
                vl[0] = wl[0];
                obs = obsL + (P.obs_stride ? ts * obs_pitch(P.O) : 0);  // t*'s obstacles (per-problem sets)
                if constexpr (PL::OREG) {  // (the register copy of the table too)
                    if (P.obs_stride && obs_reg) {
#pragma unroll
                        for (int i = 0; i < 6; ++i) oreg[i] = reinterpret_cast<const f32x4*>(obs)[i];
                    }
                }
                h_lr0 = HP[ts * kHpW + 0];
                h_lr = h_lr0 * P.bls_bm;
                h_ljl = HP[ts * kHpW + 1];
                h_lsg = HP[ts * kHpW + 2];
                h_loss = HP[ts * kHpW + 3];
                // (a direction round of t* — the only live trajectory, so dirr is its own — resets its trial
                // count at the inner-loop head, after HP was written)
                h_trial = dirr ? 0 : __float_as_int(HP[ts * kHpW + 4]);
                h_inner = __float_as_int(HP[ts * kHpW + 5]);
            }
        }
        IRM_STAMP(0);
        if constexpr (!PL::BLS) {
            if (dirr) {  // block-uniform
                IRM_COUNT(13, dense);
                if constexpr (PL::DENSE) {
                    dense_stage1(dense);
                } else {
                    stage1(dense, pre1, pre1w, pre1e);
                    stage1z(zpre);
                    // the next round's flag word: last read at the previous round's top, next set by this
                    // round's decisions (two barriers on either side)
                    if constexpr (PL::kS1Ord) {
                        if (tid == 0) fw[par ^ 1] = 0u;
                    }
                }
                IRM_STAMP(1);
                __syncthreads();
                IRM_STAMP(2);
                if constexpr (PL::DENSE) dense_stage2();
                else stage2f(std::true_type{}, std::true_type{});
                IRM_STAMP(3);
                __syncthreads();
                IRM_STAMP(4);
                if constexpr (PL::kGLate) glate_tiles();
            }
        } else if ((fl >> 30) & 1u) {  // block-uniform: some trajectory has a line-search trial this round
            // (a round with a new direction: stage 1 first; the trial stages of bls_gz / bls_f, above)
            if (dirr) {
                IRM_COUNT(13, dense);
                stage1(dense, pre1, pre1w, pre1e);
                IRM_STAMP(1);
                __syncthreads();
                IRM_STAMP(2);
            }
            if (dirr) bls_gz(std::true_type{}, hm, hs);
            else bls_gz(std::false_type{}, hm, hs);
            if (dirr) {
                // alpha_norm·‖G‖ = Σ_r (y''_r·1)² with G = V_R·y'' (optimizer_BLS.py:166 without forming G; the
                // endpoint velocity rows are in y''), rows r = li < RP of the trajectory's first wave (‖G‖:
                // the G-tile waves, bls_gz)
                if (needs_dir && n0 == 0) {  // wave-uniform
                    float s1 = 0.f;
                    if (tvalid && li < RP) {
                        float sa = 0.f;
                        const int lr = lnd(li);
#pragma unroll
                        for (int a = 0; a < D; ++a) {
                            float y = Ypart[(t * D + a) * ldy + swz(lr, t * D + a)];
                            for (int sp = 1; sp < nsplit; ++sp) y += Ypart[(sp * 16 + t * D + a) * ldy + swz(lr, t * D + a)];
                            sa += y;
                        }
                        s1 = sa * sa;
                    }
                    s1 = wred_sum(s1);
                    if (lane == 0) wp[t * 2 + 1] = s1;
                }
            }
            IRM_STAMP(3);
            __syncthreads();
            IRM_STAMP(4);
            if constexpr (PL::kHelp) {
                if (helper) ss_read(ts);  // (t* wrote them at this round's top)
            }
            bls_f();
            __syncthreads();
        }
        // ------------------------------------------------ BLS: a new direction (the inner-loop head)
        if constexpr (PL::BLS) {
            if (needs_dir) {  // wave-uniform; optimizer_BLS.py:163-166
                gnorm = TS[t * kTsW + 1];  // ‖G‖ as the trial stages used it (bls_gz)
                anorm = wp[t * 2 + 1] / gnorm;
                st.grad_evals++;  // cost + grad at α (optimizer_BLS.py:163-164)
                st.cost_evals++;
                trial = 0;
                needs_dir = false;
            }
        }
        // this round's step (BLS: the trial's; a helper's: t*'s next trial, lr·β₋)
        float cj = cfac, stepj = lr, lrj = lr, gnj = gnorm;
        if constexpr (PL::BLS) {
            if (helper) {
                h_gn = TS[ts * kTsW + 1];  // t*'s ‖G‖ and alpha_norm, the same values as t*'s latch
                h_an = wp[ts * 2 + 1] / h_gn;
                lrj = h_lr;
                gnj = h_gn;
            }
            cj = unfused(1.f - unfused(P.lreg * lrj));  // (1 − λ_reg·bls_lr) in fp32 (optimizer_BLS.py:139)
            stepj = div_rcp(lrj, gnj, rcp_refined(gnj));  // bls_gz's step, bit for bit
        }
        // ------------------------------------------------ end of an inner loop: α's exact trajectory
        if (rsy) {  // block-uniform
            const bool rs = phase == LP_RESYNC || (PL::kQueue && phase == LP_LOAD);  // wave-uniform
            if constexpr (PL::kQueue) {
                if (phase == LP_LOAD) {
                    // the claimed problem b into this slot: everything the prologue sets per trajectory.  The
                    // slot's registers may have served as a helper (vl, obs, tg, oreg), its LDS rows and words
                    // hold the finished problem's
                    vl[0] = nn[0] < N;
#pragma unroll
                    for (int k = 0; k < D; ++k) tg[0][k] = (nn[0] == N - 1) ? P.goal[b * D + k] : P.start[b * D + k];
                    if (P.alpha0) {
#pragma unroll
                        for (int k = 0; k < D; ++k) al[0][k] = vl[0] ? P.alpha0[(b * N + nn[0]) * D + k] : 0.f;
                    } else {  // stage_alpha's α0, the same operations in the same order
                        const float un = vl[0] ? P.uvec[nn[0]] : 0.f, wn = vl[0] ? P.wvec[nn[0]] : 0.f;
#pragma unroll
                        for (int k = 0; k < D; ++k) {
                            float sj = 0.f, gj = 0.f;
#pragma unroll
                            for (int e2 = 0; e2 < D; ++e2) {
                                sj += P.start[b * D + e2] * P.Jinv[e2 * D + k];
                                gj += P.goal[b * D + e2] * P.Jinv[e2 * D + k];
                            }
                            al[0][k] = vl[0] ? un * sj + wn * gj : 0.f;
                        }
                    }
                    if constexpr (PL::BLS) {  // the α rows of the trial stages
                        if (vl[0]) {
#pragma unroll
                            for (int k = 0; k < D; ++k) Ab[(t * D + k) * lde + swz(nn[0], t * D + k)] = al[0][k];
                        }
                    }
                    obs = obsL + (P.obs_stride ? t * obs_pitch(P.O) : 0);
                    if (P.obs_stride) {  // the problem's own obstacle table (stage_obstacles' layout)
                        const int pitch = obs_pitch(P.O);
                        for (int r = li; r < pitch; r += PL::NWL) {
                            const int o = 2 * (r >> 2) + (r & 1), coord = (r >> 1) & 1;
                            obsL[t * pitch + r] = o < P.O ? P.obstacles[b * P.obs_stride + 2 * o + coord] : 1.0e20f;
                        }
                    }
                    lsg = P.lsg0;
                    ljl = P.ljl0;
                    lr = PL::BLS ? P.bls_lr0 : P.gd_lr[0];
                    cfac = P.gd_c[0];
                    gnorm = 1.f;
                    anorm = 0.f;
                    outer = inner = trial = 0;
                    needs_dir = xdense = adopt = false;
                    n_rounds = n_hm = 0;
                    st = irm_stats{};
                }
            }
            if (rs) {
#pragma unroll
                for (int j = 0; j < WPL; ++j) {
                    if (vl[j]) {
#pragma unroll
                        for (int k = 0; k < D; ++k) {
                            X[(t * D + k) * ldx + lnd(nn[j])] = al[j][k];
                            if constexpr (!PL::BLS) Eb[(t * D + k) * lde + swz(nn[j], t * D + k)] = 0.f;  // absorbed by the exact trajectory
                        }
                    }
                }
            }
            __syncthreads();
            if constexpr (PL::kQueOreg) {  // (the register copy of the loaded problem's table)
                if (phase == LP_LOAD && P.obs_stride && obs_reg) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) oreg[i] = reinterpret_cast<const f32x4*>(obs)[i];
                }
            }
            if (rs) {
#pragma unroll
                for (int j = 0; j < WPL; ++j) {
                    if (vl[j]) {
                        if constexpr (PL::kResyncBatch) eval_exact<D, PL::kResyncU, true>(P, X + (t * D) * ldx, nn[j], q[j], v[j], nullptr, nullptr, 1, ldx, Jl);
                        else eval_exact_loop<D, 4>(P, X + (t * D) * ldx, ldx, nn[j], N, Jl, q[j], v[j]);
                        // the last extended-vis frame shows the exact trajectory of the returned α (frame 0
                        // stays the initial trajectory, as in k_optimize)
                        if (rec && st.series_len > 1) {
#pragma unroll
                            for (int k = 0; k < D; ++k)
                                P.series[((b * P.max_series) + st.series_len - 1) * N * D + ser_row(j) + k] = q[j][k];
                        }
                    }
                }
            }
            // the operator fragments again (from L2): so they are not live across the resync's exact
            // evaluation, whose register peak spilled them (the 7-DoF dual-loop / BLS kernels)
            if constexpr (PL::kReloadOps) {
                asm volatile("" ::: "memory");
                load_ops();
            }
            __syncthreads();  // X is rewritten by this round's gradient inputs
        }
        // ------------------------------------------------ update + evaluate
        float q2[WPL][D], v2[WPL][D];
        WP<D> w[WPL];
        // (PL::kGPre) the GD single loop's G rows of the α update read with the direction (stage 2 wrote both)
        float Gp[PL::kGPre ? WPL : 1][D];
        // (PL::kAjPre) BLS: this slot's trial iterate α_j read with the direction (bls_gz wrote it)
        float Ajp[PL::kAjPre ? WPL : 1][D];
        const bool stepping = PL::GD1 ? !done : (phase == LP_STEP || helper);  // wave-uniform
        const bool ev = PL::GD1 ? !done : (phase != LP_DONE || helper);
        if (ev) {
#pragma unroll
            for (int j = 0; j < WPL; ++j) {
                if (stepping) {
                    float dt[D], dv[D];
                    {
                        direction(j, dt, dv);
                        if constexpr (PL::kGPre) grad_alpha(j, Gp[j], t);
                        if constexpr (PL::kAjPre) {
#pragma unroll
                            for (int k = 0; k < D; ++k) Ajp[j][k] = Ajb[(t * D + k) * lde + swz(wl[j] ? lnd(nn[j]) : 0, t * D + k)];
                        }
#pragma unroll
                        for (int k = 0; k < D; ++k) {
                            const float tq = -(stepj * dt[k]), tv = -(stepj * dv[k]);
                            q2[j][k] = fmaf(cj, q[j][k], tq);
                            v2[j][k] = fmaf(cj, v[j][k], tv);
                            // the products stay live past the FMAs: three-address FMAs, whose results
                            // can take the waypoint state's own registers (no copies at the round's end)
                            if constexpr (PL::GD1) asm volatile("" ::"v"(tq), "v"(tv), "v"(q2[j][k]), "v"(v2[j][k]));
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        q2[j][k] = q[j][k];
                        v2[j][k] = v[j][k];
                    }
                }
            }
            IRM_STAMP(5);
            if constexpr (PL::GD1) {
                // the GD single loop's waypoint state moves to the trial point unconditionally: a
                // rejected step ends the trajectory, whose q / v are not read again (the epilogue
                // evaluates α exactly) — no copies on the accept path
#pragma unroll
                for (int j = 0; j < WPL; ++j)
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        q[j][k] = q2[j][k];
                        v[j][k] = v2[j][k];
                    }
            }
            // an inner loop's end is evaluated with the next outer iteration's λ (its loss and gradient
            // start that iteration; the constraint terms do not depend on λ)
            const bool rs = !PL::GD1 && phase == LP_RESYNC;
            evaluate(q2, v2, rs, helper ? h_ljl : rs ? ljl * P.lci : ljl, w);
        }
        IRM_STAMP(7);
        if constexpr (PL::WPTL > 1) {
            __syncthreads();  // the trajectory's wave partials come from several waves
        } else if (hm) {      // block-uniform: t* reads the helper's records
            __syncthreads();
        } else {              // one wave per trajectory: its own LDS writes, in order
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        }
        IRM_STAMP(8);
        if constexpr (PL::kHelp) {
            if (helper) {  // replay t*'s decision up to this trial: is it the accepted one?
                const Fin f0 = finalize(h_lsg, ts);
                if (f0.nl > h_loss - P.bls_a * h_lr0 * h_an && h_trial + 1 < P.max_bls) {
                    const Fin f1 = finalize(h_lsg, t);
                    if (!(f1.nl > h_loss - P.bls_a * h_lr * h_an)) {
                        // t*'s α_j (the trial stages' iterate of this slot's columns), T, V — adopted at the next
                        // round's start; α_j also into t*'s α rows for the next trial stages
                        float ajh[WPL][D];
#pragma unroll
                        for (int k = 0; k < D; ++k) {
                            ajh[0][k] = PL::kAjPre ? Ajp[0][k] : Ajb[(t * D + k) * lde + swz(nn[0], t * D + k)];
                            if (wl[0]) Ab[(ts * D + k) * lde + swz(nn[0], ts * D + k)] = ajh[0][k];
                        }
                        ss_write(ts, ajh, q2, v2);
                        if (!(h_loss - f1.nl < P.llr) && h_inner + 1 < P.max_inner) {
                            const bool bf = grad_inputs(w, q2, v2, f1.idx, h_lsg, h_ljl, ts);  // t*'s columns
                            if (lane == 0) {
                                HP[ts * kHpW + 6 + (wave - t * PL::WPTL)] = bf ? 1.f : 0.f;
                                if (bf) atomicOr(&fw[par ^ 1], 1u << 31);
                            }
                        }
                    }
                }
            }
        }
        if (ev && !helper) {
            const bool rs = !PL::GD1 && phase == LP_RESYNC;
            const float lsg_e = rs ? lsg * P.lci : lsg;
            // (kGFin) the lane's G words of the α update read in one batch with finalize's records (glate_tiles
            // wrote Gb before the evaluation's barrier; finalize's reads stay behind its scheduling barrier):
            // the accepted step waits on no LDS read of its own; a rejected step leaves them unused
            float Gf[PL::kGFin ? WPL : 1][D];
            if constexpr (PL::kGFin) {
#pragma unroll
                for (int j = 0; j < WPL; ++j) grad_alpha(j, Gf[j], t);
            }
            const Fin f = finalize(lsg_e, t);
            IRM_STAMP(9);
            bool bfar = false, to_end = false, accept = false, snap = false, more = false;
            if constexpr (!PL::BLS) needs_dir = false;  // GD: every step consumes its direction
            if constexpr (PL::GD1) {
                st.grad_evals++;
                st.cost_evals++;
                if (loss - f.nl < P.llr) {
                    done = true;  // minimized: the step is discarded (optimizer_GD.py:87-90)
                } else {
                    accept = true;
                    loss = f.nl;
                    inner++;
                    st.inner_iterations++;
                    if (inner >= P.max_inner) done = true;
                    else more = true;
                }
            } else if (PL::kQueue && phase == LP_LOAD) {
                // round 0 of the loaded problem (optimizer_GD.py:93 / :210: the loss at α0), as after the prologue
                loss = f.nl;
                if constexpr (!PL::BLS) st.cost_evals = 1;
                bool te = P.max_inner <= 0;
                if constexpr (PL::BLS) te = te || P.max_outer <= 0;  // α0 is returned (optimizer_BLS.py:184-186)
                if (te) {
                    to_end = true;
                } else {
                    phase = LP_STEP;
                    more = true;
                }
            } else if (rs) {
                // constraintsFulfilled(α) (trajectory.py:129-137, robot.py:90-113) on α's exact
                // trajectory; optimizer_GD.py:214-224 / optimizer_BLS.py:196-208
                const bool ok = sqrtf(f.a0) < P.eps_p && sqrtf(f.a1) < P.eps_p && sqrtf(f.b0) < P.eps_v &&
                                sqrtf(f.b1) < P.eps_v && f.tx <= P.pmax && f.tn >= P.pmin && f.va <= P.vmax;
                if (!PL::BLS || P.max_outer > 0) st.outer_iterations++;
                st.constraints_ok = ok ? 1 : 0;
                outer++;
                if (ok || outer >= P.max_outer) {
                    phase = LP_DONE;
                } else {  // next outer iteration: λ escalated, lr reset, loss at α (optimizer_GD.py:210)
                    lsg = lsg_e;
                    ljl = ljl * P.lci;
                    loss = f.nl;
                    inner = 0;
                    if constexpr (PL::BLS) {
                        lr = P.bls_lr0;
                    } else {
                        lr = P.gd_lr[outer];
                        cfac = P.gd_c[outer];
                        st.cost_evals++;
                    }
                    if (P.max_inner <= 0) {
                        st.final_loss = loss;  // phase stays LP_RESYNC: the empty inner loop ends at once
                    } else {
                        phase = LP_STEP;
                        more = true;
                    }
                }
            } else if constexpr (!PL::BLS) {  // GD dual loop inner step (optimizer_GD.py:180-195)
                st.grad_evals++;
                st.cost_evals++;
                if (loss - f.nl < P.llr) {
                    to_end = true;  // minimized: the step is discarded
                } else {
                    accept = true;
                    snap = true;
                    loss = f.nl;
                    inner++;
                    st.inner_iterations++;
                    if (inner >= P.max_inner) to_end = true;
                    else more = true;
                }
            } else {  // BLS trial (optimizer_BLS.py:136-150, 172-178)
                bool inner_end = false, rejected_all = false;
                float improve = 0.f;
                // this round's trials in the sequential order: t*'s own, then (helper round) the helper's
#pragma unroll
                for (int kk = 0; kk < (PL::kHelp ? 2 : 1); ++kk) {
                    if (kk == 1 && (!hm || accept || inner_end)) break;  // (the helper's trial was not reached)
                    const Fin fk = kk == 0 ? f : finalize(lsg_e, hs);
                    st.cost_evals++;
                    st.bls_trials++;
                    const float required = loss - P.bls_a * lr * anorm;
                    if (P.trace && b == (size_t)(P.trace_b & 0xFFFFFF) && li == 0 && st.bls_trials - 1 < P.trace_cap) {  // line-search log
                        float* r = P.trace + (size_t)(st.bls_trials - 1) * kTraceW;
                        r[0] = (float)outer;
                        r[1] = (float)inner;
                        r[2] = (float)trial;
                        r[3] = lr;
                        r[4] = fk.nl;
                        r[5] = required;
                        r[6] = (fk.nl > required) ? 0.f : 1.f;
                        r[7] = loss;
                        r[8] = gnorm;
                        r[9] = anorm;
                        if (P.trace_b >> 30) {  // diagnostics: helper round (outer + 100), helper's trial (trial + 1000)
                            if (hm) r[0] += 100.f;
                            if (kk == 1) r[2] += 1000.f;
                        }
                    }
                    if (fk.nl > required) {
                        lr = lr * P.bls_bm;
                        trial++;
                        if (trial >= P.max_bls) inner_end = rejected_all = true;  // new_loss = loss
                    } else {
                        if (kk == 0) accept = true;
                        else adopt = true;  // the helper's α_j and trajectory, next round
                        lr = lr * P.bls_bp;
                        improve = loss - fk.nl;
                        loss = fk.nl;
                        inner_end = true;
                    }
                }
                if (inner_end) {
                    if (improve < P.llr) {
                        to_end = true;
                    } else {
                        inner++;
                        st.inner_iterations++;
                        snap = true;
                        if (inner >= P.max_inner) {
                            to_end = true;
                        } else if (rejected_all) {
                            needs_dir = true;  // the same α: X still holds its gradient inputs
                            bfar = xdense;
                        } else {
                            more = true;
                        }
                    }
                }
            }
            if (accept && PL::BLS) {
                // the trial's iterate α_j (formed by the trial stages, bls_gz) and its trajectory
                // (optimizer_BLS.py:149); α_j into the α rows for the next trial stages
#pragma unroll
                for (int j = 0; j < WPL; ++j)
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        const int o = (t * D + k) * lde + swz(wl[j] ? lnd(nn[j]) : 0, t * D + k);
                        if (wl[j]) {
                            al[j][k] = PL::kAjPre ? Ajp[j][k] : Ajb[o];
                            Ab[o] = al[j][k];
                        }
                        q[j][k] = q2[j][k];
                        v[j][k] = v2[j][k];
                    }
            } else if (accept) {
                // α' = fl(fl(c·α) − fl(lr·G)) (optimizer_GD.py:81) and its residual for the next direction
                // (−e/lr folded into stage 2's y'')
                const float ne = PL::GD1 ? nilr : -1.f / fmaxf(stepj, kMinRefStep);
#pragma unroll
                for (int j = 0; j < WPL; ++j) {
                    float G[D];
                    if constexpr (PL::kGPre) {
#pragma unroll
                        for (int k = 0; k < D; ++k) G[k] = Gp[j][k];
                    } else if constexpr (PL::kGFin) {
#pragma unroll
                        for (int k = 0; k < D; ++k) G[k] = Gf[j][k];
                    } else {
                        grad_alpha(j, G, t);
                    }
                    // the D element chains first (one basic block, interleaved), then the residual stores
                    float eo[D];
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        al[j][k] = alpha_step_gd2(al[j][k], cj, stepj, G[k], ne, eo[k]);
                        if constexpr (!PL::GD1) {
                            q[j][k] = q2[j][k];
                            v[j][k] = v2[j][k];
                        }
                    }
                    if (wl[j]) {
#pragma unroll
                        for (int k = 0; k < D; ++k) Eb[(t * D + k) * lde + swz(nn[j], t * D + k)] = eo[k];
                    }
                }
            }
            if (snap) snapshot(st);
            if (to_end) {  // inner loop over: α's exact trajectory and the constraint check next round
                st.final_loss = loss;
                phase = LP_RESYNC;
            }
            if constexpr (PL::GD1) {
                if (more) bfar = grad_inputs(w, q2, v2, f.idx, lsg, ljl, t);
                if (lane == 0 && (!done || bfar))
                    atomicOr(&fw[par ^ 1], (done ? 0u : 1u << wave) | (bfar ? 1u << 31 : 0u));
            } else {
                if (more) {
                    if (!(PL::kHelp && adopt)) {  // (adopted: the helper wrote the gradient inputs)
                        bfar = grad_inputs(w, q2, v2, f.idx, lsg, ljl, t);
                        xdense = bfar;
                    }
                    needs_dir = true;
                }
                if constexpr (PL::BLS) ts_write();  // the next round's trial stages read lr and the phase
                if constexpr (PL::kHelp) {
                    // publish this trajectory's scalars for a helper, every round (α, T, V: at the top of a
                    // helper round)
                    if (phase != LP_DONE && n0 == 0 && lane == 0) {
                        HP[t * kHpW + 0] = lr;
                        HP[t * kHpW + 1] = ljl;
                        HP[t * kHpW + 2] = lsg;
                        HP[t * kHpW + 3] = loss;
                        HP[t * kHpW + 4] = __int_as_float(trial);
                        HP[t * kHpW + 5] = __int_as_float(inner);
                    }
                    // done: the outputs now (this slot's registers may serve as a helper from here on)
                    if (phase == LP_DONE && tvalid) {
                        if ((P.trace_b >> 29) & 1) st.series_len = n_rounds | (n_hm << 16);  // diagnostics
                        write_out();
                    }
                }
                if constexpr (PL::kQueue) {
                    if (phase == LP_DONE) {  // (only valid slots get here)
                        if constexpr (!PL::kHelp) write_out();
                        // the next problem: one lane of the slot's first wave takes an index; the slot's waves
                        // read it after the round-end barrier.  A problem to load keeps the slot's wave bits
                        // set and asks for a resync round (its carrier)
                        if (n0 == 0 && lane == 0) {
                            const int nx = atomicAdd(P.queue, 1);
                            red[wave * 8 + 6] = __int_as_float(nx);
                            if (nx < P.B) atomicOr(&fw[par ^ 1], (((1u << PL::WPTL) - 1u) << wave) | 1u << 29);
                        }
                        qpend = true;
                    }
                }
                if (lane == 0 && phase != LP_DONE)
                    atomicOr(&fw[par ^ 1], (1u << wave) | (needs_dir ? 1u << 28 : 0u) |
                                               (phase == LP_RESYNC ? 1u << 29 : 0u) | (phase == LP_STEP ? 1u << 30 : 0u) |
                                               // BLS: every trajectory in a line search keeps the velocity
                                               // half on while its inputs have one (its Ypart / Gb columns
                                               // are recomputed by other trajectories' direction rounds)
                                               ((PL::BLS ? xdense && phase == LP_STEP : bfar) ? 1u << 31 : 0u));
            }
        }
        IRM_STAMP(11);
        __syncthreads();
        IRM_STAMP(12);
    }

    // ---------------------------------------------------------- epilogue
    if constexpr (PL::GD1) {
        // T = eval_exact(α) (correctly rounded K·α·J), constraintsFulfilled(α) (trajectory.py:129-137,
        // robot.py:90-113) on it.  Every wave has left the loop after its last barrier: X is free.
        st.final_loss = loss;
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
            if (vl[j]) {
#pragma unroll
                for (int k = 0; k < D; ++k) X[nn[j] * kLd + t * D + k] = al[j][k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WPL; ++j)
            if (vl[j]) eval_exact<D>(P, X + t * D, nn[j], q[j], v[j]);
        {
            WP<D> w[WPL];
            evaluate(q, v, true, ljl, w);
        }
        __syncthreads();
        if (tvalid) {
            const Fin f = finalize(lsg, t);
            const bool ok = sqrtf(f.a0) < P.eps_p && sqrtf(f.a1) < P.eps_p && sqrtf(f.b0) < P.eps_v &&
                            sqrtf(f.b1) < P.eps_v && f.tx <= P.pmax && f.tn >= P.pmin && f.va <= P.vmax;
            st.outer_iterations = 1;
            st.constraints_ok = ok ? 1 : 0;
        }
    }
    // (LF_GD2 / LF_BLS: every trajectory ended through LP_RESYNC — q, v are α's exact trajectory;
    // kHelp: written when the trajectory finished)
    if (!PL::kHelp && !PL::kQueue && tvalid) write_out();
    if (tid == 0) prof.flush(P.prof);
}

}  // namespace irm

// the kernels and launchers in headers of their own (they follow the optimiser kernels they launch)
#include "irm_k_forward.hpp"  // k_forward: the α-space evaluation kernel
#include "irm_launch.hpp"     // the per-shape launchers
