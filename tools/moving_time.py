"""Time of the moving-obstacle path on the C3-shaped problem (reported, not a target).

    python tools/moving_time.py [--reps 30] [--warmup 5] [--rounds 3] [--out profiles/moving_time.json]

The problem is bench.py's c3 in bench mode (1024 problems, N = 128, D = 3, 11 shared obstacles, 200 GD steps
each), launched through irm_optimize_batch(_moving)_dev on device buffers, three ways:

  a  static                      the shape-specialised k_lean (bench.py's headline)
  b  moving, zero velocities     k_optimize<DynShape<3>> (the kernel every moving launch runs)
  c  moving, non-zero velocities the same kernel

c − b is what the feature itself costs (it should be nothing but the two packed FMAs per obstacle pair),
b − a is the known gap between the general and the lean kernel, the argument for a later lean variant.

Timing: device events around each launch on the caller's stream, after `warmup` launches per variant; the
variants alternate within each of `rounds` rounds (a, b, c, a, b, c, …) so that drift of the machine falls on
all three alike.  Per variant: the median over all timed launches, the minimum, the maximum and the
interquartile range; per round the medians, whose spread is the run-to-run noise a difference has to exceed.
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
    ap.add_argument("--reps", type=int, default=30, help="timed launches per variant and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "moving_time.json"))
    a = ap.parse_args()

    import torch

    import bench
    from irm_motion_planning_amd.context import Context, batch_dev
    from irm_motion_planning_amd.params import params_from_args

    desc, B, N, D, O, opt = bench.CONFIGS["c3"]
    args = bench.make_args("c3", False, 200)
    start, goal, obstacles = bench.make_problem("c3", 1, 0)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    ctx = Context(params_from_args(args, device=0))
    f32 = dict(dtype=torch.float32, device=dev)
    start_t, goal_t = torch.from_numpy(start).to(dev), torch.from_numpy(goal).to(dev)
    obs_t = torch.from_numpy(np.ascontiguousarray(obstacles, np.float32)).to(dev)
    zero_t = torch.zeros_like(obs_t)
    rng = np.random.default_rng(5)
    drift_t = torch.from_numpy(rng.uniform(-1.0, 1.0, tuple(obs_t.shape)).astype(np.float32)).to(dev)
    alpha_t = torch.empty((B, N, D), **f32)
    traj_t = torch.empty_like(alpha_t)
    stats_t = torch.zeros((B, 8), dtype=torch.int32, device=dev)

    def batch(vel):
        return batch_dev(start=start_t.data_ptr(), goal=goal_t.data_ptr(), obstacles=obs_t.data_ptr(), n_obstacles=O,
                         batch=B, alpha_out=alpha_t.data_ptr(), traj_out=traj_t.data_ptr(),
                         stats_out=stats_t.data_ptr(), obstacle_velocity=vel)

    variants = [("a_static_k_lean", batch(0), ctx.launch_plan(B, O)),
                ("b_moving_zero_velocity", batch(zero_t.data_ptr()), ctx.launch_plan(B, O, obstacle_velocity=True)),
                ("c_moving_nonzero_velocity", batch(drift_t.data_ptr()), ctx.launch_plan(B, O, obstacle_velocity=True))]
    ms = {name: [] for name, _, _ in variants}
    iters = {}
    for name, bd, _ in variants:
        for _ in range(a.warmup):
            ctx.optimize_dev(bd, stream.cuda_stream)
        torch.cuda.synchronize(dev)
        iters[name] = int(stats_t.cpu().numpy()[:, 2].sum())  # grad_evals of one launch
    for _ in range(a.rounds):
        for name, bd, _ in variants:
            evs = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.optimize_dev(bd, stream.cuda_stream)
                e1.record(stream)
                evs.append((e0, e1))
            torch.cuda.synchronize(dev)
            ms[name].append([e0.elapsed_time(e1) for e0, e1 in evs])
    info = ctx.info()
    result = {"problem": desc, "batch": B, "N": N, "D": D, "obstacles": O, "gd_steps": 200, "reps": a.reps,
              "rounds": a.rounds, "warmup": a.warmup, "device": info["device_name"], "build_id": info["build_id"],
              "variants": {}}
    for name, _, plan in variants:
        x = np.array(ms[name])
        q1, q3 = np.percentile(x, [25, 75])
        result["variants"][name] = {
            "kernel": plan["kernel"], "threads": plan["threads"], "grid": plan["grid"], "lds_bytes": plan["lds_bytes"],
            "grad_evals_per_launch": iters[name], "median_ms": float(np.median(x)), "min_ms": float(x.min()),
            "max_ms": float(x.max()), "iqr_ms": float(q3 - q1), "round_medians_ms": [float(np.median(r)) for r in x],
            "launches": int(x.size)}
    v = result["variants"]
    result["feature_cost_ms_c_minus_b"] = v["c_moving_nonzero_velocity"]["median_ms"] - v["b_moving_zero_velocity"]["median_ms"]
    result["general_vs_lean_gap_ms_b_minus_a"] = v["b_moving_zero_velocity"]["median_ms"] - v["a_static_k_lean"]["median_ms"]
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
