"""Time of a via launch next to the end-effector-goal launch of the same shape (reported, not a target).

    python tools/via_time.py [--reps 20] [--warmup 3] [--rounds 3] [--inner 50] [--out profiles/via_time.json]

The problem is bench.py's C3 shape (1024 problems, N = 128, D = 3, 11 shared obstacles) in two flows — BLS (one
outer iteration of `inner` BLS iterations, bench.py's c3bls in bench mode) and the GD dual loop (3 outer iterations
of `inner` steps, every step accepted) — launched through irm_optimize_batch_*_dev on device buffers, three ways,
all on k_optimize<DynShape<3>>:

  task   goal_xy = FK(goal)                      the end-effector-goal launch
  via1   the same plus one end-effector via-point at row N/2
  via4   the same plus four via-points, rows (1, N/2, N/2 + 1, N − 2), kinds joint / xy / joint / xy

Every via target is what the straight line between start and goal has at that row (its configuration, or its
end-effector position), so the objectives stay close and the launches do comparable work; the cost evaluations
per launch (irm_stats.cost_evals, summed over the batch) are recorded next to the time.  Timing as
tools/task_time.py: device events around each launch after `warmup` launches per variant, the variants alternating
within each round.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def fk(links, q):
    ang = np.cumsum(q.astype(np.float64), axis=-1)
    return np.stack([(links * np.cos(ang)).sum(-1), (links * np.sin(ang)).sum(-1)], axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50, help="inner iterations per outer iteration")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "via_time.json"))
    a = ap.parse_args()

    import torch

    import bench
    from irm_motion_planning_amd import main as irm_main
    from irm_motion_planning_amd._abi import STATS_FIELDS
    from irm_motion_planning_amd.context import Context, batch_dev
    from irm_motion_planning_amd.params import params_from_args
    from irm_motion_planning_amd.via import ViaPoints

    desc, B, N, D, O, _ = bench.CONFIGS["c3bls"]
    start, goal, obstacles = bench.make_problem("c3bls", 1, 0)
    links = np.asarray(bench.make_args("c3bls", False, a.inner).link_length, np.float64)
    goal_xy = fk(links, goal).astype(np.float32)
    rows4, kinds4 = [1, N // 2, N // 2 + 1, N - 2], [0, 1, 0, 1]

    def targets(rows, kinds):
        out = np.zeros((B, len(rows), D), np.float32)
        for i, (m, k) in enumerate(zip(rows, kinds)):
            q = start + (goal - start) * np.float32(m / (N - 1.0))
            if k:
                out[:, i, :2] = fk(links, q)
            else:
                out[:, i] = q
        return out

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    start_t, goal_t = torch.from_numpy(start).to(dev), torch.from_numpy(goal).to(dev)
    xy_t = torch.from_numpy(goal_xy).to(dev)
    obs_t = torch.from_numpy(np.ascontiguousarray(obstacles, np.float32)).to(dev)
    alpha_t = torch.empty((B, N, D), **f32)
    traj_t = torch.empty_like(alpha_t)
    stats_t = torch.zeros((B, len(STATS_FIELDS)), dtype=torch.int32, device=dev)
    bd = batch_dev(start=start_t.data_ptr(), goal=goal_t.data_ptr(), obstacles=obs_t.data_ptr(), n_obstacles=O, batch=B,
                   alpha_out=alpha_t.data_ptr(), traj_out=traj_t.data_ptr(), stats_out=stats_t.data_ptr())
    via1 = ViaPoints([N // 2], [1], targets([N // 2], [1]))
    via4 = ViaPoints(rows4, kinds4, targets(rows4, kinds4))
    tg1, tg4 = torch.from_numpy(via1.padded(B, D)).to(dev), torch.from_numpy(via4.padded(B, D)).to(dev)
    flows = {
        "bls": bench.make_args("c3bls", False, a.inner),
        "gd2": irm_main.parse_args(["--optimizer-name", "gd", "--n-timesteps", str(N), "--n-joints", str(D),
                                    "--loop-loss-reduction=-1e30", "--max-outer-iteration=3",
                                    f"--max-inner-iteration={a.inner}", "--gd-lr", "2e-3", "1e-4", "1e-5"]),
    }
    result = {"problem": desc, "batch": B, "N": N, "D": D, "obstacles": O, "inner_iterations": a.inner, "reps": a.reps,
              "rounds": a.rounds, "warmup": a.warmup, "flows": {}}
    for flow, args in flows.items():
        ctx = Context(params_from_args(args, device=0))
        variants = [("task", None, 0, ctx.launch_plan(B, O, goal_xy=True)),
                    ("via1", via1, tg1.data_ptr(), ctx.launch_plan(B, O, goal_xy=True, via=via1)),
                    ("via4", via4, tg4.data_ptr(), ctx.launch_plan(B, O, goal_xy=True, via=via4))]

        def launch(via, tg):
            ctx.optimize_dev(bd, stream.cuda_stream, goal_xy_dev=xy_t.data_ptr(), via=via, via_target_dev=tg)

        ms = {name: [] for name, _, _, _ in variants}
        evals = {}
        for name, via, tg, _ in variants:
            for _ in range(a.warmup):
                launch(via, tg)
            torch.cuda.synchronize(dev)
            evals[name] = int(stats_t.cpu().numpy()[:, STATS_FIELDS.index("cost_evals")].sum())
        for _ in range(a.rounds):
            for name, via, tg, _ in variants:
                evs = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    launch(via, tg)
                    e1.record(stream)
                    evs.append((e0, e1))
                torch.cuda.synchronize(dev)
                ms[name].append([e0.elapsed_time(e1) for e0, e1 in evs])
        info = ctx.info()
        result["device"], result["build_id"] = info["device_name"], info["build_id"]
        out = {}
        for name, _, _, plan in variants:
            x = np.array(ms[name])
            q1, q3 = np.percentile(x, [25, 75])
            out[name] = {"kernel": plan["kernel"], "threads": plan["threads"], "grid": plan["grid"],
                         "lds_bytes": plan["lds_bytes"], "cost_evals_per_launch": evals[name],
                         "median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
                         "iqr_ms": float(q3 - q1), "round_medians_ms": [float(np.median(r)) for r in x],
                         "launches": int(x.size)}
        result["flows"][flow] = out
        ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
