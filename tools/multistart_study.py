"""The nine-scene study of multi-start planning (scenes in tests/multistart_cases.py), reported, not a
target: one disc obstacle at nine positions inside the arm's sweep, the single seed against S = 12 seeds of amplitude
1.2, ranked by (constraints ok, collision-free on 257 samples, loss).

    python tools/multistart_study.py cpu     the fp64 restatement of the BLS loop (tests/bls_cases.py) on the
                                             library's operators, from the numpy twin's seeds; no GPU
    python tools/multistart_study.py gpu     Context.optimize_multistart on the device

The cpu mode forms α of candidate s ≥ 1 as fp32(W·(Q·J⁻¹)) with the library's W (irm_fit_operator) and numpy's
inverse of J, and candidate 0 with the CPU oracle's initTrajectory: the device's seeds up to rounding, not to the bit.
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import multistart_cases as mc  # noqa: E402

f32 = np.float32


def report(mode, ok, ncol, loss):
    """ok, ncol, loss: (scenes, S).  Ranks with the twin and prints the counts."""
    winner, _ = mc.rank_lexsort(ok, loss, ncol)
    rows = np.arange(ok.shape[0])
    single = mc.study_counts(ok[:, 0], ncol[:, 0])
    multi = mc.study_counts(ok[rows, winner], ncol[rows, winner])
    out = {"mode": mode, "scenes": int(ok.shape[0]), "n_seeds": int(ok.shape[1]), "amplitude": mc.STUDY_A,
           "single_collision_free": single[0], "single_ok_and_free": single[1],
           "multi_collision_free": multi[0], "multi_ok_and_free": multi[1],
           "collision_free_candidates_per_scene": (ncol == 0).sum(axis=1).tolist(),
           "ok_and_free_candidates_per_scene": ((ncol == 0) & (ok != 0)).sum(axis=1).tolist(),
           "winner": winner.tolist()}
    print(json.dumps(out), flush=True)
    return out


def run_gpu():
    from irm_motion_planning_amd import main as irm_main
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args
    c = Context(params_from_args(irm_main.parse_args(["--n-timesteps", str(mc.STUDY_N)])))
    c.set_eval_times(np.linspace(0, 1, mc.STUDY_M, dtype=f32))
    nb = mc.STUDY_SCENES.shape[0]
    _, _, _, info = c.optimize_multistart(np.broadcast_to(mc.STUDY_START, (nb, 3)), np.broadcast_to(mc.STUDY_GOAL, (nb, 3)),
                                          mc.STUDY_SCENES[:, None, :], mc.STUDY_S, seed=mc.STUDY_SEED,
                                          amplitude=mc.STUDY_A, rank_clearance=True, obstacle_radius=mc.STUDY_RADIUS,
                                          candidates=True)
    return report("gpu", info["stats"]["constraints_ok"], info["reports"]["n_colliding"], info["stats"]["final_loss"])


def run_cpu():
    import bls_cases as bc
    import clearance_cases as cc
    import via_cases as vc
    from irm_motion_planning_amd.context import fit_operator
    from test_gpu_dense import query_matrices
    R, o = vc.restatement("--n-timesteps", str(mc.STUDY_N))
    p = o.params
    t, K, dK, J = o.kernel_matrices()
    N, S, nb = mc.STUDY_N, mc.STUDY_S, mc.STUDY_SCENES.shape[0]
    lo, hi = mc.clamp_bounds(p.joint_safety_limit, p.min_joint_position, p.max_joint_position)
    start, goal = np.broadcast_to(mc.STUDY_START, (nb, 3)), np.broadcast_to(mc.STUDY_GOAL, (nb, 3))
    way = mc.waypoints(start, goal, S, mc.STUDY_SEED, mc.STUDY_A, lo, hi, t)  # scenes × S × N × D
    W = fit_operator(N, float(p.rbf_variance))
    J64 = np.asarray(J, np.float64)
    Jinv = np.linalg.inv(J64)
    kq, _ = query_matrices(N, np.linspace(0, 1, mc.STUDY_M, dtype=f32), float(p.rbf_variance))
    links = [float(p.link_length[i]) for i in range(3)]
    a0 = np.asarray(o.init_alpha(mc.STUDY_START, mc.STUDY_GOAL), f32).reshape(N, 3)
    ok, ncol, loss = (np.zeros((nb, S), dt) for dt in (np.int32, np.int32, f32))
    for b in range(nb):
        table = mc.STUDY_SCENES[b][None, :]
        for s in range(S):
            alpha0 = a0 if s == 0 else (W @ (way[b, s].astype(np.float64) @ Jinv)).astype(f32)
            run = bc.bls_log(R, alpha0, table, mc.STUDY_START, mc.STUDY_GOAL)
            q = (kq.astype(np.float64) @ run.alpha.astype(np.float64)) @ J64
            g = cc.clearance64(q, links, np.broadcast_to(table, (mc.STUDY_M, 1, 2)), np.array([mc.STUDY_RADIUS]))[0]
            ok[b, s], loss[b, s] = run.stats["constraints_ok"], run.stats["final_loss"]
            ncol[b, s] = int((g.min(axis=(1, 2)) < 0).sum())
        print(f"scene {b}: ok {ok[b].tolist()} colliding samples {ncol[b].tolist()}", flush=True)
    return report("cpu", ok, ncol, loss)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    res = run_gpu() if mode == "gpu" else run_cpu()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
