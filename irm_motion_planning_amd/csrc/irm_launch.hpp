// irm_launch.hpp — the host-side launchers of the optimiser kernels and k_forward: which kernel serves a
// launch (lean / work queue / dense / general), its LDS request and what irm_optimize_plan reports of it.
// Defines the templates irm_launch_decl.hpp declares.  Included by irm_kernels_impl.hpp, after the kernels it launches
// (it is not a header to include on its own).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <type_traits>

#include "irm_dispatch.hpp"     // dispatch_t, launch_lds
#include "irm_k_forward.hpp"    // k_forward
#include "irm_launch_decl.hpp"  // per-shape launcher declarations and the shape lists
#include "irm_lean_plan.hpp"    // LeanFlow, LeanPlan

namespace irm {

// ------------------------------------------------------------- launchers
// LDS of k_lean: the optimiser head + obstacles, no staged F fragments, the lean regions of the launch's
// plan PL (the helpers' exchange regions, PL::kHelp; the BLS and dense layouts).
template <class PL>
inline size_t lean_lds(const KParams& p) {
    KParams q = p;
    q.regops = 1;
    return (size_t)lean_extra(plan_lds(q, false, true, true).total, p.MP, p.NK, p.RP, p.nsplit, lean_vlds(p.NK, p.D, p.BT),
                              p.D, PL::kHelp ? p.BT : 0, PL::BLS, PL::DENSE).total * 4;
}

// The optimiser's control flow in LeanFlow terms (k_optimize runs every flow in one instantiation): the GD
// single loop (dualOptimization = max_outer_iteration > 1, optimizer_GD.py:18) without extended-vis
// snapshots is the bench flow; GD with snapshots or a dual loop, and BLS, the full flows.
inline int optimizer_flow(const KParams& p) {
    if (p.optimizer == IRM_OPT_BLS) return LF_BLS;
    return (p.max_outer <= 1 && !p.record_series) ? LF_GD1 : LF_GD2;
}
// The lean kernel's control flow for a launch (-1: the general kernel serves it).
inline int lean_flow(const KParams& p) { return p.lean_ok ? optimizer_flow(p) : -1; }
// PL: the plan of the instantiation that would serve the launch, so the check sees the LDS the launch will
// request (per-problem obstacle tables grow the base with TB·O)
template <class PL>
inline bool lean_fits(const KParams& p) {
    return (p.RP / 16) * p.nsplit <= p.BT / 64 && p.NK / 16 <= 4 * p.nsplit && lean_lds<PL>(p) <= 160 * 1024;
}

// k_optimize<Shape> with the MAXT / operator-placement / optimiser variants (one shape per
// instantiation unit, irm_opt_inst.hip).
template <class Sh>
hipError_t launch_general_shape(const KParams& p, hipStream_t s, LaunchDesc* desc);

template <class Sh>
inline int shape_name(char* buf, size_t n) {
    if constexpr (Sh::kDense) return snprintf(buf, n, "DenseShape<%d,%d>", Sh::D, Sh::N);
    else if constexpr (Sh::kNW > 0) return snprintf(buf, n, "FixShape<%d,%d,%d>", Sh::D, Sh::N, Sh::RP);
    else return snprintf(buf, n, "DynShape<%d>", Sh::D);
}
inline const char* flow_name(int flow) { return flow == LF_GD1 ? "GD1" : flow == LF_GD2 ? "GD2" : "BLS"; }
// What the launch of k_lean<Sh, TT, WPL, FULL, FLOW, QUE> records in `desc` besides run_optimizer's fields: the
// instantiation's name, its flow, waypoints per lane and per-stage ranks.
template <class Sh, int TT, int WPL, bool FULL, int FLOW, bool QUE>
inline void describe_lean(LaunchDesc* desc) {
    if (!desc) return;
    char sn[48];
    shape_name<Sh>(sn, sizeof(sn));
    snprintf(desc->kernel, sizeof(desc->kernel), "k_lean<%s,%d,%d,%s,%s%s>", sn, TT, WPL, FULL ? "FULL" : "PART",
             flow_name(FLOW), QUE ? ",QUEUE" : "");
    desc->lean = 1;
    desc->flow = FLOW;
    desc->wpl = WPL;
    desc->rank_z = desc->rank_dir = 16;  // k_lean's per-stage ranks at RP = 32
    desc->rank_g = 24;
    if constexpr (Sh::kDense) {  // V_R = I: G is y'' and z is e' (no MFMAs), the direction at rank N
        desc->rank_z = desc->rank_g = 0;
        desc->rank_dir = Sh::RP;
    }
}

// The one place an optimiser kernel is launched: records what runs in `desc` (irm_optimize_plan) and
// launches unless desc->describe_only.
template <class K>
inline hipError_t run_optimizer(LaunchDesc* desc, K kernel, int grid, int threads, size_t lds, hipStream_t s,
                                const KParams& p) {
    if (desc) {
        desc->grid = grid;
        desc->threads = threads;
        desc->lds_bytes = (int)lds;
        desc->traj_per_block = p.TB;
        if (desc->describe_only) return hipSuccess;
    }
    return launch_lds(kernel, grid, threads, lds, s, p);
}

template <class Sh, int TT, int WPL, bool FULL, int FLOW>
hipError_t launch_lean_one(const KParams& p, int grid, hipStream_t s, LaunchDesc* desc) {
    describe_lean<Sh, TT, WPL, FULL, FLOW, false>(desc);
    return run_optimizer(desc, k_lean<Sh, TT, WPL, FULL, FLOW>, grid, p.BT,
                         lean_lds<LeanPlan<Sh, TT, WPL, FULL, FLOW, false>>(p), s, p);
}

template <class Sh, int TT, int WPL, bool FULL>
hipError_t launch_lean_flow(const KParams& p, int flow, int grid, hipStream_t s, LaunchDesc* desc) {
    switch (flow) {
        case LF_GD1: return launch_lean_one<Sh, TT, WPL, FULL, LF_GD1>(p, grid, s, desc);
        case LF_GD2: return launch_lean_one<Sh, TT, WPL, FULL, LF_GD2>(p, grid, s, desc);
        default: return launch_lean_one<Sh, TT, WPL, FULL, LF_BLS>(p, grid, s, desc);
    }
}

// The work queue's instantiations k_lean<Sh, 256 / 512, 1, FULL, GD2 / BLS, QUE> (units of their own,
// irm_opt_inst.hip IRM_INST_FIXQ_*): one waypoint per lane.
template <class Sh>
constexpr bool lean_queue_shape() {
    if constexpr (Sh::kNW > 0 && !Sh::kDense && !Sh::kVariants) {  // (a fixed shape: N is a constant)
#define IRM_IS_SHAPE(D_, N_) || (Sh::D == D_ && Sh::N == N_)
        return false IRM_QUEUE_SHAPES(IRM_IS_SHAPE);
#undef IRM_IS_SHAPE
    } else {
        return false;
    }
}
// Auto (irm_set_work_queue(ctx, -1)) selects the queue only where it measured faster than the static launch
// by more than the spread of repeated launches (profiles/work_queue_ab.json): the C3 shape's
// four-trajectory 512-thread workgroups, BLS −16 %, GD dual loop −7.5 % at B = 8,192.  (7-DoF N = 128 won
// 7 % with two workgroups per CU and lost 35 % with one; it and the unmeasured shapes stay explicit.)
constexpr bool lean_queue_auto(int D, int N, int threads, int flow) {
    return D == 3 && N == 128 && threads == 512 && (flow == LF_BLS || flow == LF_GD2);
}
// Serves a launch whose context asks for the queue (p.queue_groups != 0) with G < `grid` persistent
// workgroups: sets the problem counter to G·TB on the stream, then launches.  *served = false leaves the
// launch to the static dispatch (the request covers every workgroup, auto does not select this flow).
template <class Sh>
hipError_t launch_lean_queue(const KParams& p, int flow, int grid, hipStream_t s, LaunchDesc* desc, bool* served);

template <class Sh, int TT, int FLOW>
hipError_t launch_lean_queue_flow(const KParams& p, int grid, hipStream_t s, LaunchDesc* desc, bool* served) {
    auto kernel = k_lean<Sh, TT, 1, true, FLOW, true>;
    const size_t lds = lean_lds<LeanPlan<Sh, TT, 1, true, FLOW, true>>(p);
    int G = p.queue_groups;
    if (G < 0) {  // auto: every CU full of resident workgroups, as the runtime counts them for this LDS request
        if (!lean_queue_auto(Sh::D, Sh::N, TT, FLOW)) return hipSuccess;
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        int per_cu = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, TT, lds);
        if (e != hipSuccess) return e;
        G = p.num_cus * per_cu;
    }
    if (G <= 0 || G >= grid || !p.queue) return hipSuccess;
    *served = true;
    describe_lean<Sh, TT, 1, true, FLOW, true>(desc);
    if (desc) desc->queue_groups = G;
    if (!desc || !desc->describe_only) {
        const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)p.queue, G * p.TB, 1, s);
        if (e != hipSuccess) return e;
    }
    return run_optimizer(desc, kernel, G, p.BT, lds, s, p);
}

template <class Sh>
hipError_t launch_lean_queue(const KParams& p, int flow, int grid, hipStream_t s, LaunchDesc* desc, bool* served) {
    *served = false;
    if (p.BT == 512) {
        if (flow == LF_GD2) return launch_lean_queue_flow<Sh, 512, LF_GD2>(p, grid, s, desc, served);
        if (flow == LF_BLS) return launch_lean_queue_flow<Sh, 512, LF_BLS>(p, grid, s, desc, served);
    } else if (p.BT == 256) {
        if (flow == LF_GD2) return launch_lean_queue_flow<Sh, 256, LF_GD2>(p, grid, s, desc, served);
        if (flow == LF_BLS) return launch_lean_queue_flow<Sh, 256, LF_BLS>(p, grid, s, desc, served);
    }
    return hipSuccess;
}
// (the shapes of lean_queue_shape, IRM_QUEUE_SHAPES in irm_launch_decl.hpp.  Declared here so that the dispatch
// units call the queue units' instantiations instead of compiling their own)
#define IRM_EXTERN_FIXQ(D_, N_)                                                                                   \
    extern template hipError_t launch_lean_queue<FixShape<D_, N_, 32>>(const KParams&, int, int, hipStream_t, \
                                                                       LaunchDesc*, bool*);
IRM_QUEUE_SHAPES(IRM_EXTERN_FIXQ)

template <class Sh>
hipError_t launch_optimize_shape(const KParams& p, hipStream_t s, LaunchDesc* desc) {
    const int grid = (p.B + p.TB - 1) / p.TB;
    if (grid <= 0) return hipSuccess;
    return dispatch_t(p.BT, [&](auto tc) {
        constexpr int TT = decltype(tc)::value;
        const int flow = lean_flow(p);
        if constexpr (!Sh::kVariants && TT == 512) {
            if constexpr (Sh::kNW == 128) {
                // diagnostic (IRM_LEAN_WPL=2): one wave per trajectory, two waypoints per lane
                KParams q = p;
                q.BT = p.BT / 2;
                q.NW = p.NW / 2;
                if (p.lean_wpl == 2 && flow == LF_GD1 && lean_fits<LeanPlan<Sh, 256, 2, false, LF_GD1, false>>(q))  // (GD only)
                    return launch_lean_one<Sh, 256, 2, false, LF_GD1>(q, grid, s, desc);
            }
        }
        if constexpr (!Sh::kVariants && TT <= 512) {  // the lean kernel (F operators register-resident:
            // one stage-1 unit per wave; workgroups are padded to TT threads by choose_shape)
            // (the GD flows' plans request the same LDS: no helpers, the GD layout)
            const bool fits = flow == LF_BLS ? lean_fits<LeanPlan<Sh, TT, 1, true, LF_BLS, false>>(p)
                                             : lean_fits<LeanPlan<Sh, TT, 1, true, LF_GD1, false>>(p);
            if (flow >= 0 && p.BT == TT && fits) {
                if constexpr (lean_queue_shape<Sh>()) {
                    // the work queue, where the context asks for it (series launches keep the static launch)
                    if (p.queue_groups != 0 && flow != LF_GD1 && !p.record_series) {
                        bool served = false;
                        const hipError_t e = launch_lean_queue<Sh>(p, flow, grid, s, desc, &served);
                        if (served || e != hipSuccess) return e;
                    }
                }
                return launch_lean_flow<Sh, TT, 1, true>(p, flow, grid, s, desc);
            }
        }
        if constexpr (!Sh::kVariants && TT == 1024) {
            if constexpr (Sh::kNW == 256 && Sh::D * 3 <= kCols) {  // ≥ 3 trajectories fit the MFMA columns
                // N = 256 with more than two trajectories per workgroup: two waypoints per lane
                KParams q = p;
                q.BT = p.BT / 2;
                q.NW = p.NW / 2;
                const bool fits = flow == LF_BLS ? lean_fits<LeanPlan<Sh, 512, 2, false, LF_BLS, false>>(q)
                                                 : lean_fits<LeanPlan<Sh, 512, 2, false, LF_GD1, false>>(q);
                if (flow >= 0 && fits) return launch_lean_flow<Sh, 512, 2, false>(q, flow, grid, s, desc);
            }
        }
        return launch_general_shape<Sh>(p, s, desc);
    });
}

// The general optimiser k_optimize<Shape, …> (every optimiser / control flow).  Instantiated in its
// own unit (irm_opt_inst.hip, IRM_INST_GEN_*) so that build.py can compile it with the
// iterative-ILP machine scheduler, which measured 10 % faster on it (faithful C3) while the lean
// kernels keep the default scheduler.
// The dense operator's k_lean (DenseShape, GD single loop, one 512-thread workgroup of TB trajectories):
// *served = false leaves the launch to the general kernel (another workgroup size, LDS).
template <class Sh>
hipError_t launch_dense_shape(const KParams& p, hipStream_t s, LaunchDesc* desc, bool* served) {
    *served = false;
    if (p.BT != 512 || p.TB * Sh::D > kCols || lean_flow(p) != LF_GD1) return hipSuccess;
    KParams q = p;
    q.nsplit = 1;  // one split: every wave's stage-1 row tiles over the whole k range
    if (lean_lds<LeanPlan<Sh, 512, 1, true, LF_GD1, false>>(q) > 160 * 1024) return hipSuccess;
    *served = true;
    const int grid = (p.B + p.TB - 1) / p.TB;
    if (grid <= 0) return hipSuccess;
    return launch_lean_one<Sh, 512, 1, true, LF_GD1>(q, grid, s, desc);
}

template <class Sh>
hipError_t launch_general_shape(const KParams& p, hipStream_t s, LaunchDesc* desc) {
    const bool stage = p.ops_in_lds != 0;
    const Plan L = plan_lds(p, stage, true, false, Sh::kVariants && p.moving != 0, Sh::kVariants && p.via != 0);
    const size_t lds = (size_t)L.total * 4;
    const int grid = (p.B + p.TB - 1) / p.TB;
    if (grid <= 0) return hipSuccess;
    return dispatch_t(p.BT, [&](auto tc) {
        constexpr int TT = decltype(tc)::value;
        auto name = [&](bool ops_lds, bool regops, bool bls, bool full) {
            if (!desc) return;
            char sn[48];
            shape_name<Sh>(sn, sizeof(sn));
            snprintf(desc->kernel, sizeof(desc->kernel), "k_optimize<%s,%d,%s,%s,%s%s>", sn, TT,
                     ops_lds ? "OPS_LDS" : "OPS_L2", regops ? "REGOPS" : "-", bls ? "BLS" : "GD", full ? ",FULL" : "");
            desc->lean = 0;
            desc->flow = optimizer_flow(p);
            desc->wpl = 1;
            desc->rank_z = desc->rank_dir = desc->rank_g = p.RP;
            if (p.v_ident) desc->rank_g = desc->rank_z = 0;  // V_R = I: G is y'', z is e' (no MFMAs)
        };
        auto go = [&](auto bc) {
            constexpr bool BB = decltype(bc)::value;
            if constexpr (TT <= 512) {
                if constexpr (!Sh::kVariants) {
                    if (p.regops && p.BT == TT) {
                        name(true, true, BB, true);
                        return run_optimizer(desc, k_optimize<Sh, TT, true, true, BB, true>, grid, p.BT, lds, s, p);
                    }
                }
                if (p.regops) {
                    name(true, true, BB, false);
                    return run_optimizer(desc, k_optimize<Sh, TT, true, true, BB>, grid, p.BT, lds, s, p);
                }
            }
            name(stage, false, BB, false);
            return stage ? run_optimizer(desc, k_optimize<Sh, TT, true, false, BB>, grid, p.BT, lds, s, p)
                         : run_optimizer(desc, k_optimize<Sh, TT, false, false, BB>, grid, p.BT, lds, s, p);
        };
        return p.optimizer == IRM_OPT_BLS ? go(std::integral_constant<bool, true>{})
                                          : go(std::integral_constant<bool, false>{});
    });
}

template <int D>
hipError_t launch_forward_dim(const KParams& p, int mode, hipStream_t s) {
    const Plan L = plan_lds(p, false, false, false, p.moving != 0, p.via != 0);
    const size_t lds = (size_t)L.total * 4;
    const int grid = (p.B + p.TB - 1) / p.TB;
    if (grid <= 0) return hipSuccess;
    return dispatch_t(p.BT, [&](auto tc) {
        constexpr int TT = decltype(tc)::value;
        return launch_lds(k_forward<D, TT>, grid, p.BT, lds, s, p, mode);
    });
}

}  // namespace irm
