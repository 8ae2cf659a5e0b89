"""Time of a multi-start call next to the optimiser launch inside it (reported, not a target).

    python tools/multistart_time.py [--reps 10] [--warmup 2] [--rounds 3] [--out profiles/multistart_time.json]

The shape is bench.py's C3 (N = 128, D = 3, 11 shared obstacles, GD in bench mode: every problem runs
--max-inner-iteration steps), B = 128 of its problems with S = 8 seeds each: 1024 candidates, C3's batch.  On device
buffers through the enqueue-only entry points:

  plain   irm_optimize_batch_dev       C3's own 1024 problems from the straight line (what bench.py times)
  inner   irm_optimize_batch_dev       the 1024 replicated problems from the seeds: the launch inside the call
  multi   irm_optimize_multistart_dev  seeds, replicate, that launch, rank, gather
  seeds   irm_seed_ensemble_dev        the seeds alone
  rank    irm_rank_candidates_dev      the ranking alone

multi − inner is what the ensemble costs.  Timing as tools/clearance_time.py: device events around each call after
`warmup` calls per variant, the variants alternating within each round.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, S = 128, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed calls per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-inner", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multistart_time.json"))
    a = ap.parse_args()

    import torch

    import bench
    from irm_motion_planning_amd.context import Context, batch_dev
    from irm_motion_planning_amd.params import params_from_args

    desc, B0, N, D, O, _ = bench.CONFIGS["c3"]
    start, goal, obstacles = bench.make_problem("c3", 1, 0)
    ctx = Context(params_from_args(bench.make_args("c3", False, a.max_inner), device=0))
    seeds = ctx.seed_ensemble(start[:B], goal[:B], S, seed=1, amplitude=1.0).reshape(B * S, N, D)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)  # noqa: E731
    s_t, g_t, o_t = up(start), up(goal), up(obstacles)
    sr_t, gr_t, a0_t = up(np.repeat(start[:B], S, axis=0)), up(np.repeat(goal[:B], S, axis=0)), up(seeds)
    big = lambda: torch.empty((B0, N, D), dtype=torch.float32, device=dev)  # noqa: E731
    a_out, t_out, st_out = big(), big(), torch.zeros((B0, 8), dtype=torch.int32, device=dev)
    wa_out, wt_out = torch.empty((B, N, D), device=dev), torch.empty((B, N, D), device=dev)
    wst_out = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    winner = torch.zeros(B, dtype=torch.int32, device=dev)
    nbytes = ctx.multistart_workspace(B, S, O, 0)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    bd_plain = batch_dev(start=s_t.data_ptr(), goal=g_t.data_ptr(), obstacles=o_t.data_ptr(), n_obstacles=O, batch=B0,
                         alpha_out=a_out.data_ptr(), traj_out=t_out.data_ptr(), stats_out=st_out.data_ptr())
    bd_inner = batch_dev(alpha0=a0_t.data_ptr(), start=sr_t.data_ptr(), goal=gr_t.data_ptr(), obstacles=o_t.data_ptr(),
                         n_obstacles=O, batch=B * S, alpha_out=a_out.data_ptr(), traj_out=t_out.data_ptr(),
                         stats_out=st_out.data_ptr())
    bd_multi = batch_dev(start=s_t.data_ptr(), goal=g_t.data_ptr(), obstacles=o_t.data_ptr(), n_obstacles=O, batch=B,
                         alpha_out=wa_out.data_ptr(), traj_out=wt_out.data_ptr(), stats_out=wst_out.data_ptr())
    cs = stream.cuda_stream
    variants = [
        ("plain", lambda: ctx.optimize_dev(bd_plain, stream=cs)),
        ("inner", lambda: ctx.optimize_dev(bd_inner, stream=cs)),
        ("multi", lambda: ctx.optimize_multistart_dev(bd_multi, S, winner.data_ptr(), ws.data_ptr(), nbytes, seed=1,
                                                      amplitude=1.0, stream=cs)),
        ("seeds", lambda: ctx.seed_ensemble_dev(s_t.data_ptr(), g_t.data_ptr(), B, S, a0_t.data_ptr(), seed=1, stream=cs)),
        ("rank", lambda: ctx.rank_candidates_dev(st_out.data_ptr(), B, S, winner.data_ptr(), stream=cs)),
    ]
    ms = {name: [] for name, _ in variants}
    for _, launch in variants:
        for _ in range(a.warmup):
            launch()
    torch.cuda.synchronize(dev)
    for _ in range(a.rounds):
        for name, launch in variants:
            evs = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                evs.append((e0, e1))
            torch.cuda.synchronize(dev)
            ms[name].append([e0.elapsed_time(e1) for e0, e1 in evs])
    info = ctx.info()
    result = {"problem": desc, "batch": B, "n_seeds": S, "N": N, "D": D, "obstacles": O, "max_inner": a.max_inner,
              "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup, "device": info["device_name"],
              "build_id": info["build_id"], "workspace_bytes": nbytes, "variants": {}}
    for name, _ in variants:
        x = np.array(ms[name])
        q1, q3 = np.percentile(x, [25, 75])
        result["variants"][name] = {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
                                    "iqr_ms": float(q3 - q1), "round_medians_ms": [float(np.median(r)) for r in x]}
    v = result["variants"]
    result["ensemble_overhead_ms"] = v["multi"]["median_ms"] - v["inner"]["median_ms"]
    result["ensemble_overhead_fraction"] = result["ensemble_overhead_ms"] / v["inner"]["median_ms"]
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
