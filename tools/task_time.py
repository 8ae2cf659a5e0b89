"""Time of an end-effector-goal BLS launch on the C3-shaped problem (reported, not a target).

    python tools/task_time.py [--reps 20] [--warmup 3] [--rounds 3] [--inner 50] [--out profiles/task_time.json]

The problem is bench.py's c3bls in bench mode (1024 problems, N = 128, D = 3, 11 shared obstacles, one outer
iteration of `inner` BLS iterations), launched through irm_optimize_batch_*_dev on device buffers, three ways:

  a  joint goal, k_lean                        the static launch (bench.py's c3bls line)
  b  joint goal, k_optimize<DynShape<3>>       a moving launch with zero velocities: the static result to the
                                               bit, on the kernel every task launch runs (IRM_GENERAL_KERNEL=1
                                               would select k_optimize<FixShape<3,128,32>>, another instantiation)
  c  task goal, k_optimize<DynShape<3>>        the same launch with goal_xy = FK(goal): the same kernel, with
                                               zero velocities too, so that c − b is the feature alone

The two objectives differ, so the line searches take other numbers of trials: next to the time per launch the
cost evaluations per launch (irm_stats.cost_evals, summed over the batch) are recorded, and the time per
evaluation round is what compares.  Timing as tools/moving_time.py: device events around each launch after
`warmup` launches per variant, the variants alternating within each round.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="BLS inner iterations per launch")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "task_time.json"))
    a = ap.parse_args()

    import torch

    import bench
    from irm_motion_planning_amd._abi import STATS_FIELDS
    from irm_motion_planning_amd.context import Context, batch_dev
    from irm_motion_planning_amd.params import params_from_args

    desc, B, N, D, O, opt = bench.CONFIGS["c3bls"]
    args = bench.make_args("c3bls", False, a.inner)
    start, goal, obstacles = bench.make_problem("c3bls", 1, 0)
    links = np.asarray(args.link_length, np.float64)
    ang = np.cumsum(goal.astype(np.float64), axis=1)
    goal_xy = np.stack([(links * np.cos(ang)).sum(1), (links * np.sin(ang)).sum(1)], axis=1).astype(np.float32)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    ctx = Context(params_from_args(args, device=0))
    f32 = dict(dtype=torch.float32, device=dev)
    start_t, goal_t = torch.from_numpy(start).to(dev), torch.from_numpy(goal).to(dev)
    xy_t = torch.from_numpy(goal_xy).to(dev)
    obs_t = torch.from_numpy(np.ascontiguousarray(obstacles, np.float32)).to(dev)
    zero_t = torch.zeros_like(obs_t)
    alpha_t = torch.empty((B, N, D), **f32)
    traj_t = torch.empty_like(alpha_t)
    stats_t = torch.zeros((B, len(STATS_FIELDS)), dtype=torch.int32, device=dev)

    def batch(vel):
        return batch_dev(start=start_t.data_ptr(), goal=goal_t.data_ptr(), obstacles=obs_t.data_ptr(), n_obstacles=O,
                         batch=B, alpha_out=alpha_t.data_ptr(), traj_out=traj_t.data_ptr(),
                         stats_out=stats_t.data_ptr(), obstacle_velocity=vel)

    variants = [("a_joint_k_lean", batch(0), 0, ctx.launch_plan(B, O)),
                ("b_joint_general", batch(zero_t.data_ptr()), 0, ctx.launch_plan(B, O, obstacle_velocity=True)),
                ("c_task_general", batch(zero_t.data_ptr()), xy_t.data_ptr(), ctx.launch_plan(B, O, goal_xy=True))]
    ms = {name: [] for name, _, _, _ in variants}
    evals = {}
    for name, bd, xy, _ in variants:
        for _ in range(a.warmup):
            ctx.optimize_dev(bd, stream.cuda_stream, goal_xy_dev=xy)
        torch.cuda.synchronize(dev)
        evals[name] = int(stats_t.cpu().numpy()[:, STATS_FIELDS.index("cost_evals")].sum())
    for _ in range(a.rounds):
        for name, bd, xy, _ in variants:
            evs = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.optimize_dev(bd, stream.cuda_stream, goal_xy_dev=xy)
                e1.record(stream)
                evs.append((e0, e1))
            torch.cuda.synchronize(dev)
            ms[name].append([e0.elapsed_time(e1) for e0, e1 in evs])
    info = ctx.info()
    result = {"problem": desc, "batch": B, "N": N, "D": D, "obstacles": O, "bls_inner_iterations": a.inner,
              "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup, "device": info["device_name"],
              "build_id": info["build_id"], "variants": {}}
    for name, _, _, plan in variants:
        x = np.array(ms[name])
        q1, q3 = np.percentile(x, [25, 75])
        result["variants"][name] = {
            "kernel": plan["kernel"], "threads": plan["threads"], "grid": plan["grid"], "lds_bytes": plan["lds_bytes"],
            "cost_evals_per_launch": evals[name], "median_ms": float(np.median(x)), "min_ms": float(x.min()),
            "max_ms": float(x.max()), "iqr_ms": float(q3 - q1), "round_medians_ms": [float(np.median(r)) for r in x],
            "launches": int(x.size)}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
