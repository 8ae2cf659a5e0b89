// irm_kernels.hpp — launch-side interface between the C-ABI host code
// (irm_host.cpp) and the gfx950 kernels (irm_kernels.hip).  Everything that needs no
// HIP type (KParams, the fragment and LDS layouts, LaunchDesc) is in irm_layout.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/irm.h"
#include "irm_layout.hpp"

namespace irm {

// launchers (return hipError_t)
hipError_t launch_init_alpha(const KParams& p, float* alpha_out, hipStream_t s);
hipError_t launch_optimize(const KParams& p, hipStream_t s, LaunchDesc* desc = nullptr);
hipError_t launch_forward(const KParams& p, int mode, hipStream_t s);  // mode: 0 evaluate, 1 cost, 2 cost+grad, 3 constraints
hipError_t launch_fk(const KParams& p, const float* traj, float* pos, float* jac, hipStream_t s);
hipError_t launch_fk_joints(const KParams& p, const float* traj, float* pos, hipStream_t s);
hipError_t launch_cost_vg(const KParams& p, const float* f, float* cv, float* cg, hipStream_t s);
// IK seed of an end-effector goal (irm_ik_seed): p.B problems, start B×D, goal_xy B×2, joint range [lo, hi];
// q_out B×D, res_out B (nullable), device pointers
hipError_t launch_ik_seed(const KParams& p, const float* start, const float* goal_xy, float lo, float hi, float* q_out,
                          float* res_out, hipStream_t s);
// irm_dense.hip — evaluation at arbitrary times.  mT / kqT / dkqT: query matrices on the device, transposed
// ([N][M]); α from p.alpha0 (B×N×D), obstacles from p.obstacles / p.O / p.obs_stride.
hipError_t launch_eval_any(const KParams& p, const float* mT, int M, float* out, hipStream_t s);
hipError_t launch_dense_check(const KParams& p, const float* kqT, const float* dkqT, int M, irm_dense_report* rep,
                              float* cost, hipStream_t s);
// irm_clearance.hip — link-against-disc clearance on the evaluation times (irm_clearance).  radius: the obstacle
// radii on the device (nullable; radius_stride floats between the problems' tables, 0 shared); rep B, clear B×M,
// link B×D, joints B×M×D×2 (the last three nullable); a moving launch reads p.obs_vel and p.tsup (the evaluation times).
hipError_t launch_clearance(const KParams& p, const float* kqT, int M, const float* radius, int radius_stride,
                            float link_radius, irm_clearance_report* rep, float* clear, float* link, float* joints,
                            hipStream_t s);
// irm_self_clearance.hip — link-against-link clearance on the evaluation times (irm_self_clearance).  α from
// p.alpha0; rep B, clear B×M, pair B×(D−1)(D−2)/2, joints B×M×D×2 (the last three nullable).
hipError_t launch_self_clearance(const KParams& p, const float* kqT, int M, float link_radius,
                                 irm_self_clearance_report* rep, float* clear, float* pair, float* joints,
                                 hipStream_t s);
// irm_fit.hip — fitting and re-timing.  wT / tT: the fit / transfer operator on the device in fp64, transposed
// ([source row m][waypoint n], n_src × N; W is N × N); kq0: the fp32 query row of the source grid at t0 (n_src);
// p.B problems of p.N waypoints.  start_out nullable.
hipError_t launch_fit_alpha(const KParams& p, const double* wT, const float* traj, float* alpha_out, hipStream_t s);
hipError_t launch_transfer_alpha(const KParams& p, const double* tT, int n_src, const float* kq0, const float* alpha_src,
                                 float* alpha_out, float* start_out, hipStream_t s);
// irm_multistart.hip — multi-start planning.  Candidate s of problem b is row b·S + s.
// Seeds: p.B problems, S candidates each; wT as launch_fit_alpha's; cphi: the smooth step c (N) then the bump φ
// (N) on the device; start / goal B×D; [lo, hi] the joint range of the clamp; alpha_out B·S×N×D, way_out nullable.
hipError_t launch_seed_ensemble(const KParams& p, const double* wT, const float* cphi, const float* start,
                                const float* goal, int S, uint32_t seed, float amplitude, uint32_t problem_offset,
                                float lo, float hi, float* alpha_out, float* way_out, hipStream_t s);
// out[(b·S + s)·w + j] = in[b·in_stride + j]
hipError_t launch_replicate(const float* in, float* out, int B, int S, int w, int in_stride, hipStream_t s);
// stats B·S, rep B·S (nullable); winner B, rank B·S (nullable)
hipError_t launch_rank_candidates(const irm_stats* stats, const irm_clearance_report* rep, int B, int S,
                                  int32_t* winner, int32_t* rank, hipStream_t s);
// row b·S + winner[b] of cand_* (nd floats per row; one irm_stats) into row b of the outputs (each nullable)
hipError_t launch_gather_winner(const int32_t* winner, int B, int S, int nd, const float* cand_alpha,
                                const float* cand_traj, const irm_stats* cand_stats, float* alpha, float* traj,
                                irm_stats* stats, hipStream_t s);

}  // namespace irm
