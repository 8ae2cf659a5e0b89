// irm_lean_plan.hpp — k_lean's control flows (LeanFlow, LeanPhase) and LeanPlan, the one record of every
// compile-time decision of an instantiation k_lean<S, MAXT, WPL, FULL, FLOW, QUE>: the flow flags, the tile
// and quad counts, where operands live, the schedule switches with the measurements behind them, and the
// kernel's static_asserts.  The kernel reads PL::x; the launchers read the same plan for the LDS request and
// the launch description.  The plans of the named instantiations are stated at the end.
// No HIP type beyond what irm_opt_common.hpp needs (its shapes carry a __device__ constructor).
// Included by irm_kernels_impl.hpp (k_lean) and irm_launch.hpp.
#pragma once
#include "irm_layout.hpp"      // lean_vlds, lean_zsplit, lean_bls_nzp, kEpS, kLeanKeep
#include "irm_opt_common.hpp"  // the shapes, kS1Q, kS2T

namespace irm {

// Control flows of the lean kernel: the GD single loop (optimizer_GD.py:68-97, the bench path), the
// GD dual loop (optimizer_GD.py:173-232) and the BLS dual loop (optimizer_BLS.py:127-213).
enum LeanFlow : int { LF_GD1 = 0, LF_GD2 = 1, LF_BLS = 2 };
// Per-trajectory phase (LF_GD2 / LF_BLS): a GD step or BLS trial this round, the end of an inner
// loop (α's exact trajectory, constraintsFulfilled, λ escalation), done.
enum LeanPhase : int { LP_STEP = 0, LP_RESYNC = 1, LP_DONE = 2, LP_LOAD = 3 };

template <class S, int MAXT, int WPL, bool FULL, int FLOW, bool QUE>
struct LeanPlan {
    // ------------------------------------------------------------------ the flow
    static constexpr bool GD1 = FLOW == LF_GD1, BLS = FLOW == LF_BLS;
    static_assert(!QUE || (FLOW != LF_GD1 && WPL == 1 && FULL && !S::kDense),
                  "the work queue serves the dual-loop / BLS flows of the fixed shapes, one waypoint per lane");
    static constexpr int D = S::D;
    // the dense operator (DenseShape: R = N, F = L, V_R = I) runs the GD single loop with its own stages
    static constexpr bool DENSE = S::kDense;
    static_assert(S::RP == 32 || (DENSE && GD1 && WPL == 1 && FULL),
                  "k_lean runs at operator rank 32 (stage 2's kR24 slot skip), or the dense operator's GD loop");
    static_assert(D <= kEpS, "endpoint rows fit their slots");
    // 256-thread workgroups of one waypoint per lane fit two per CU (≤ 256 VGPRs): __launch_bounds__' second argument
    static constexpr int kBlocksPerCU = (MAXT <= 256 && WPL == 1) ? 2 : 1;

    // ------------------------------------------------------------------ lanes, waves, tiles
    static constexpr int NWL = S::NW / WPL;  // lanes per trajectory
    static constexpr int WPTL = NWL / 64;    // waves per trajectory
    static_assert(NWL % 64 == 0, "whole waves per trajectory");
    static_assert(WPL == 1 || (WPL == 2 && S::kNW > 0 && S::kNW == S::NK),
                  "two waypoints per lane: every lane's waypoints exist (N a multiple of 64)");
    static constexpr int kSlots = (MAXT / 64) / WPTL;  // trajectory slots of a workgroup
    // waves of the launch where it has exactly MAXT threads (FULL; 0: read from the launch), so tile guards fold
    static constexpr int kWaves = FULL ? MAXT / 64 : 0;
    // one waypoint per lane: its evaluation in one call; two: both waypoints' obstacle terms in one pass
    static constexpr bool kEvalOne = WPL == 1, kEvalPair = WPL == 2;
    static constexpr bool kQueue = QUE;  // the work queue's kernel: a finished slot claims the next problem
    // every lane of a valid trajectory holds waypoints when N fills whole waves: wherever only valid
    // trajectories run (evaluation, gradient inputs, the α update), the waypoint guards fold away
    static constexpr bool kAllLive = S::kNW > 0 && S::kNW == S::N;
    static constexpr int S1Q = kS1Q(MAXT);
    // stage-2 tiles per wave: all of this shape's tiles over the workgroup's waves (N = 256: 4)
    static constexpr int S2X = (S::MP / 16 + MAXT / 64 - 1) / (MAXT / 64);
    static constexpr int S2T = (FULL || S2X > kS2T(MAXT)) ? S2X : kS2T(MAXT);

    // ------------------------------------------------------------------ where operands live
    // velocity half of stage 1 register-resident too — except in the dual-loop / BLS flows beyond C3's
    // shape, whose extra state leaves no room (read from L2 in the dense rounds there)
    static constexpr bool RV = (MAXT > 256 || WPL > 1) && (GD1 || (D == 3 && S::NK <= 128));
    static constexpr bool VL = lean_vlds(S::NK, D, MAXT);  // V_R fragments staged in LDS (else read from L2)
    // 9-12 obstacles (the reference's 11): the padded table in VGPRs for the whole launch (24 floats),
    // so the per-round evaluation does not wait on its LDS reads
    // (and the 3-joint GD dual loop: C3 faithful 3.70 -> 3.60 ms; the BLS flow with it measured C3-BLS
    // −0.5 % but C2 +2.7 %, not used; the 7-DoF dual loop spills with it)
    static constexpr bool OREG = GD1 || (D <= 3 && !BLS);
    static constexpr bool kQueOreg = QUE && OREG;  // a loaded problem's table is copied to the registers too
    // BLS line-search helpers: when one trajectory of a workgroup is left, the first done slot
    // evaluates its next trial (lr·β₋) in the same round.  D ≤ 3, one waypoint per lane, N ≤ 128 in
    // 512-thread workgroups (or N ≤ 64): where the exchange regions fit the LDS at full occupancy.
    // (helpers read t*'s α, T, V from SS: t* publishes them at the top of each helper round rather than
    // after every accepted trial of every trajectory: C3-BLS −1 %, its faithful line −0.6 %; bit-identical)
    static constexpr bool kHelp =
        FLOW == LF_BLS && S::D <= 3 && WPL == 1 && FULL && S::kNW > 0 && (S::NK <= 64 || (S::NK <= 128 && MAXT > 256));

    // ------------------------------------------------------------------ rare paths of the 7-DoF shapes
    // 7-DoF shapes: a lane index laundered at a rare path's use, so that the path's per-lane addresses are
    // formed there instead of being held across the round loop (the 7-DoF dual-loop / BLS variants spilled
    // them); the 3-joint shapes have the registers, and measured 3 % slower on C3-BLS with it
    static constexpr bool kLaunder = D > 3;
    // the 7-DoF BLS flow forms the endpoint MFMA's B address again at its use (held across the round loop it was spilled)
    static constexpr bool kEpAtUse = BLS && D > 3 && MAXT > 256;
    // the operator fragments loaded again (from L2) after a resync: so they are not live across the resync's
    // exact evaluation, whose register peak spilled them (the 7-DoF dual-loop / BLS kernels)
    static constexpr bool kReloadOps = D > 3 && MAXT > 256;
    // the resync's exact evaluation: eval_exact's batches (else eval_exact_loop, whose register peak is lower)
    static constexpr bool kResyncBatch = D <= 3;
    // K / dK rows per software-pipelined batch of the resync's eval_exact: the loads are latency-bound
    // (one L2 round trip per batch), so D = 3 with one waypoint per lane takes 8 rows per batch — no extra
    // spills there (C3 faithful 4.57 -> 4.42 ms, C3 BLS faithful 5.68 -> 5.60, C2 0.706 -> 0.689, same
    // box, same sums in the same order); the D = 7 / two-waypoint variants keep 2 (register peak)
    static constexpr int kResyncU = (D <= 3 && WPL == 1) ? 8 : 2;
    // BLS: the per-trajectory counters in VGPRs (the compiler would keep these wave-uniform values in SGPRs,
    // and the BLS flow's scalar state spills SGPRs to VGPR lanes — readlane / writelane on the round's path):
    // C3-BLS −0.9 %, its faithful line −0.4 %, C2 −0.7 %; the GD dual loop 1-1.6 % slower with it, not used
    // (the 7-DoF BLS variants have no VGPRs to spare)
    static constexpr bool kStatVgpr = BLS && D <= 3;
    // BLS: ‖G‖²'s D column sums by in-row DPP shifts (the slot's columns sit in the lane's row: same adds in
    // the same order as the bpermute gather of the 7-DoF shapes, without its LDS round trips)
    static constexpr bool kNormShift = D <= 3;

    // ------------------------------------------------------------------ latency-hiding load batches
    // Latency-hiding load batches (finalize's records and start/goal terms, stage 2's split-K partial
    // sums, the z unit's operands) hold more values live at once: stage 2's and the z unit's only for
    // N <= 128, where they fit without spills; at N = 256 (four splits, eight z ranges) they pushed the
    // spill-free GD single-loop variants into scratch (C5: 14 spilled VGPRs)
    // finalize's batch: fixed shapes with one waypoint per lane (C4's two-waypoints-per-lane kernel, one
    // wave record per trajectory, measured 2 % slower with it; C5 / C7 1.5-2 % faster)
    static constexpr bool kLatF = S::kNW > 0 && WPL == 1;
    static constexpr bool kLatS = S::kNW > 0 && S::NK <= 128;   // stage 2's and the z unit's: N <= 128

    // ------------------------------------------------------------------ stage 1
    // fixed shapes with an even split: the k-quads of a wave's stage-1 unit are known (else checked per quad)
    static constexpr bool kFix1 = S::KQU > 0 && S::KQU <= S1Q;
    static constexpr int KQU1 = kFix1 ? S::KQU : S1Q;
    // GD single loop, fixed-shape launches: stage 1's B operand (both halves; the velocity half is used
    // in dense rounds only) is read at the top of the round, before the flag word (X was written before
    // the previous barrier), so the flag and operand LDS round trips overlap; same values, same MFMA
    // order (bit-identical, tools/sched_check.py).  C3 0.769 -> 0.759 ms; the position half alone: no gain.
    // (the GD dual loop with the same prefetch: 4.33 -> 4.47 ms, 242 VGPRs there; not used)
    static constexpr bool kPre1 = GD1 && FULL && kFix1;
    static constexpr bool kPreW = kPre1 && RV;
    // C3's kernel (N = 128 in 512-thread workgroups): the round's LDS reads issued in the order of their use —
    // the round top and the decision.  Issue order only: same loads, same MFMAs, same order per chain
    // (bit-identical, tools/sched_check.py).  Alternating 300-step bench runs against the parent build: stage
    // 1's order alone −0.6 %, the G words alone −0.7 %, both −1.6 % (profiles/gd1_top_ab.txt); the z unit's
    // e' quads read at the round top as well measured +0.8 % alone and is not done
    // (kTopC3 also selects the all-live loop, the round loop of a workgroup whose every slot is stepping)
    static constexpr bool kTopC3 = kPreW && D <= 3 && WPL == 1 && MAXT > 256 && WPTL > 1 && kLatS;
    static constexpr bool kS1Ord = kTopC3;  // flag word first, stage 1's operands in use order
    static constexpr bool kGFin = kTopC3;   // the α update's G words read with finalize's records

    // ------------------------------------------------------------------ the z unit and the G tiles
    // FULL launches of a fixed shape with an even split: the z unit's operator and e' loads are issued
    // up front (one wait), then the MFMAs — the same accumulation order as the general loop
    static constexpr int kZS = lean_zsplit(S::NSPLIT, VL), kKQa = S::NK / 16;
    static constexpr bool kZFix = FULL && S::kNW > 0 && kKQa % kZS == 0 && kZS <= MAXT / 64;
    static constexpr int kKQZ = kZFix ? kKQa / kZS : 1;
    static constexpr int kMTG = S::NK / 16, kGT = (kMTG + MAXT / 64 - 1) / (MAXT / 64);
    // FULL launches of a fixed shape: the G tiles of a wave are known at compile time; their operator
    // fragments are loaded with the partial sums and their MFMAs interleave with the F tiles' (same
    // accumulation order per tile as the general form)
    static constexpr bool kS2Fix = FULL && S::kNW > 0;
    // GD flows of the fixed shapes: the z unit's V_Rᵀ fragments and the G tiles' V_R fragments are the same
    // every round — held in VGPRs for the launch instead of re-read from LDS / L2 each round
    // (C3 faithful 3.93 -> 3.75 ms, C3 even; from L2 too: C7 1.33 -> 1.27 ms, C7 faithful 7.52 -> 7.30 ms,
    // C5 1.405 -> 1.326 ms, C4 even; bit-identical.  Not the 7-DoF N = 256 dual loop / 256-thread
    // variants, which spill with them)
    static constexpr bool kVReg = !BLS && !DENSE && kZFix && kS2Fix && (VL || !(D > 3 && S::NK > 128) || (GD1 && MAXT > 256));
    // otherwise (C5's dual loop) the z unit's V_Rᵀ fragments are loaded at the round's top, so their L2
    // latency passes under stage 1 instead of holding the z waves at the stage-1 barrier
    // (C5 faithful −1.4 %, C4 even; bit-identical)
    static constexpr bool kZPre = !BLS && !DENSE && kZFix && !kVReg;
    static constexpr bool kS2Batch = kS2Fix && kLatS;  // stage 2's partial sums read in one batch
    // the GD single loop's G tiles issued after the stage-2 barrier (their MFMAs under the update and
    // evaluation; C3 -2.0 %, bit-identical)
    // (the same in every non-BLS flow measured neutral on C4, C5, C7 and +1.2 % on the 3-joint GD dual loop,
    // profiles/r05_glate_ab.txt: not kept)
    // (WPTL > 1 only: glate_tiles' waves write G rows of trajectories they do not own, and with one wave per
    // trajectory — N ≤ 64 — only a wave barrier would sit between that write and the owner's read: a race)
    static constexpr bool kGLate = GD1 && D <= 3 && kS2Fix && kS2Batch && WPTL > 1;
    // the GD single loop's G rows of the α update read with the direction (stage 2 wrote both), so their
    // LDS round trip is off the decision's path: C3 −1.3 %; the dual loop, C5 and C7 measured 0.8-1 %
    // slower with it (bit-identical either way)
    static constexpr bool kGPre = GD1 && D <= 3 && !kGLate;
    static_assert(!kGFin || (kGLate && !kGPre), "kGFin: G is read after the evaluation's barrier");

    // ------------------------------------------------------------------ the BLS trial stages
    static constexpr int kNZP = lean_bls_nzp(S::kNW > 0 ? S::NK : 256);
    // (fixed shapes up to N = 128: at N = 256 the batch's per-tile operands — four tiles per wave at 256
    // threads — pushed the BLS variants into scratch; those take the per-tile loop, same sums in the same order)
    static constexpr bool kBFix = FULL && S::kNW > 0 && S::NK <= 128;
    static constexpr int kNZc = kBFix ? (MAXT / 64 < S::NK / 16 ? MAXT / 64 : S::NK / 16) : 1;
    static_assert(!BLS || !kBFix || kNZc <= kNZP, "z partials fit their region");
    static constexpr int kTB = kBFix ? (S::NK / 16 + MAXT / 64 - 1) / (MAXT / 64) : 1;  // tiles per wave
    // V_R staged in LDS: the G-tile waves' V_R / V_Rᵀ fragments held in VGPRs for the launch (as kVReg)
    // (C3-BLS faithful 7.21 -> 7.17 ms, C3-BLS 1.426 -> 1.419 ms; bit-identical)
    static constexpr bool kVRegB = BLS && VL && kBFix;
    // BLS: this slot's trial iterate α_j read with the direction (bls_gz wrote it), off the accept's path
    static constexpr bool kAjPre = BLS;

    // ------------------------------------------------------------------ the dense operator's stages
    static constexpr int kDW = MAXT / 64;
    static constexpr int kD1 = DENSE ? (S::RP / 16 + kDW - 1) / kDW : 1;  // stage-1 row tiles per wave
    static constexpr int kD2 = DENSE ? (S::MP / 16 + kDW - 1) / kDW : 1;  // stage-2 row tiles per wave
    static constexpr int kDQ = DENSE ? S::NK / 16 : 1;                    // k-quads per half
    static constexpr int kDPF = 2;  // prefetch depth (k-quads; 3 and 4 measured the same: the stages are MFMA-bound)

    // ------------------------------------------------------------------ the all-live loop (kTopC3)
    static constexpr int kW1 = (S::RP / 16) * S::NSPLIT;  // the stage-1 waves; the z unit's are all the others
    static constexpr unsigned kAllW = (1u << (MAXT / 64)) - 1u;  // every wave's bit of the flag word
    static_assert(!kTopC3 || (kW1 + kZS == MAXT / 64 && kZFix && !kZPre && kGLate && kGFin && kLatF && kAllLive && kLeanKeep<D>),
                  "the all-live loop is written for C3's kernel");
};

// The plans of the instantiations that the resource tests name (tests/test_kernel_resources.py,
// test_gd1_fastpath_resources.py, test_work_queue_resources.py, test_dense_resources.py), as the
// expressions above give them: a change of a switch's condition that moves one of these kernels shows here.
namespace lean_plan_check {
using C3 = FixShape<3, 128, 32>;
using C7 = FixShape<7, 128, 32>;
using C4 = FixShape<3, 256, 32>;
using C5d = DenseShape<7, 256>;
// C3's kernels at 512 threads (four trajectories of two waves)
using C3gd1 = LeanPlan<C3, 512, 1, true, LF_GD1, false>;
using C3gd2 = LeanPlan<C3, 512, 1, true, LF_GD2, false>;
using C3bls = LeanPlan<C3, 512, 1, true, LF_BLS, false>;
static_assert(C3gd1::kBlocksPerCU == 1 && C3gd1::kSlots == 4 && C3gd1::S1Q == 4 && C3gd1::S2T == 2 && C3gd1::KQU1 == 4 &&
              C3gd1::kZS == 4 && C3gd1::kKQZ == 2 && C3gd1::kGT == 1 && C3gd1::kW1 == 4);
static_assert(C3gd1::RV && C3gd1::VL && C3gd1::OREG && C3gd1::kAllLive && C3gd1::kLatF && C3gd1::kLatS && C3gd1::kVReg &&
              !C3gd1::kZPre && C3gd1::kS2Batch);
static_assert(C3gd1::kPre1 && C3gd1::kPreW && C3gd1::kTopC3 && C3gd1::kGLate && !C3gd1::kGPre && !C3gd1::kHelp);
static_assert(C3gd2::RV && C3gd2::VL && C3gd2::OREG && C3gd2::kVReg && C3gd2::kS2Batch && !C3gd2::kPre1 && !C3gd2::kTopC3 &&
              !C3gd2::kGLate && !C3gd2::kGPre && !C3gd2::kHelp && C3gd2::kResyncU == 8);
static_assert(C3bls::RV && C3bls::VL && !C3bls::OREG && C3bls::kHelp && !C3bls::kVReg && !C3bls::kZPre && C3bls::kBFix &&
              C3bls::kNZc == 8 && C3bls::kTB == 1 && C3bls::kVRegB && C3bls::kAjPre && C3bls::kStatVgpr);
// C7's kernels at 256 threads (two trajectories of two waves, two workgroups per CU): operators from L2
using C7gd1 = LeanPlan<C7, 256, 1, true, LF_GD1, false>;
using C7gd2 = LeanPlan<C7, 256, 1, true, LF_GD2, false>;
using C7bls = LeanPlan<C7, 256, 1, true, LF_BLS, false>;
static_assert(C7gd1::kBlocksPerCU == 2 && C7gd1::kSlots == 2 && C7gd1::S1Q == 8 && C7gd1::S2T == 4 && C7gd1::KQU1 == 4 &&
              C7gd1::kZS == 2 && C7gd1::kKQZ == 4 && C7gd1::kGT == 2);
static_assert(!C7gd1::RV && !C7gd1::VL && C7gd1::OREG && C7gd1::kPre1 && !C7gd1::kPreW && !C7gd1::kTopC3 && C7gd1::kVReg &&
              !C7gd1::kGLate && !C7gd1::kGPre && C7gd1::kLaunder && !C7gd1::kReloadOps && C7gd1::kResyncU == 2);
static_assert(!C7gd2::OREG && C7gd2::kVReg && !C7gd2::kZPre && !C7bls::kHelp && !C7bls::kVReg && C7bls::kBFix &&
              !C7bls::kVRegB && !C7bls::kEpAtUse && !C7bls::kStatVgpr);
// C4's two-waypoints-per-lane kernel (N = 256, four trajectories of two waves in 512 threads; not FULL)
using C4gd1 = LeanPlan<C4, 512, 2, false, LF_GD1, false>;
static_assert(C4gd1::kBlocksPerCU == 1 && C4gd1::NWL == 128 && C4gd1::kSlots == 4 && C4gd1::S2T == 4 && C4gd1::KQU1 == 4 &&
              C4gd1::RV && !C4gd1::VL && C4gd1::kAllLive && !C4gd1::kLatF && !C4gd1::kLatS && C4gd1::kFix1 && !C4gd1::kPre1 &&
              !C4gd1::kZFix && !C4gd1::kS2Fix && !C4gd1::kVReg && !C4gd1::kZPre && !C4gd1::kGLate && C4gd1::kGPre &&
              C4gd1::kResyncU == 2);
// the dense operator's kernel (7-DoF, N = 256: two trajectories of four waves in 512 threads)
using C5dense = LeanPlan<C5d, 512, 1, true, LF_GD1, false>;
static_assert(C5dense::DENSE && C5dense::kD1 == 2 && C5dense::kD2 == 4 && C5dense::kDQ == 16 && C5dense::kDPF == 2 &&
              C5dense::kSlots == 2 && !C5dense::VL && !C5dense::kFix1 && !C5dense::kPre1 && !C5dense::kVReg &&
              !C5dense::kZPre && !C5dense::kGLate && C5dense::kAllLive);
// the work queue's kernels: the plan of the static launch's kernel of the same shape, threads and flow
using C3qgd2 = LeanPlan<C3, 512, 1, true, LF_GD2, true>;
using C3qbls = LeanPlan<C3, 512, 1, true, LF_BLS, true>;
using C7qgd2 = LeanPlan<C7, 256, 1, true, LF_GD2, true>;
using C7qbls = LeanPlan<C7, 256, 1, true, LF_BLS, true>;
static_assert(C3qgd2::OREG && C3qgd2::kVReg && !C3qgd2::kHelp && C3qbls::kHelp && C3qbls::kVRegB && !C3qbls::OREG);
static_assert(C7qgd2::kBlocksPerCU == 2 && C7qgd2::kVReg && !C7qgd2::OREG && !C7qbls::kHelp && !C7qbls::kVRegB);
}  // namespace lean_plan_check

}  // namespace irm
