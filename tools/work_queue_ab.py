"""A/B of the work queue against the static launch, same build, same process, alternating launches.

    python tools/work_queue_ab.py [--batch 8192] [--reps 12] [--warmup 2] [--configs c3bls c3 c7]
                                  [--out profiles/work_queue_ab.json]

For each faithful flow the batch is the eight shards bench.make_problem(cfg, 8, r) concatenated.  Modes:
"off" (the static launch: the baseline, the code path of a build without the queue), "auto" (what
irm_set_work_queue(ctx, -1) resolves to — the static launch where the policy does not select the
queue) and "cus" / "cus2" (one / two persistent workgroups per CU, explicitly, so that flows the policy
leaves out are still measured; 256-thread workgroups are resident two per CU).  Launches are timed with
device events around optimize_dev; after the timed launches every mode's α, trajectory and statistics are
compared with "off" bit for bit.
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
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", nargs="+", default=["c3bls", "c3", "c7"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "work_queue_ab.json"))
    a = ap.parse_args()

    import torch
    import bench
    from irm_motion_planning_amd.context import Context, batch_dev
    from irm_motion_planning_amd.params import params_from_args

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    result = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "flows": {}}
    for cfg in a.configs:
        _, _, N, D, O, opt = bench.CONFIGS[cfg]
        args = bench.make_args(cfg, True, 200)
        shards = [bench.make_problem(cfg, 8, r) for r in range(8)]
        start = np.concatenate([s[0] for s in shards])[:a.batch]
        goal = np.concatenate([s[1] for s in shards])[:a.batch]
        obstacles = shards[0][2]
        B = len(start)
        ctx = Context(params_from_args(args))
        info = ctx.info()
        start_t, goal_t = torch.from_numpy(start).to(dev), torch.from_numpy(goal).to(dev)
        obs_t = torch.from_numpy(obstacles).to(dev)
        modes = {"off": 0, "auto": "auto", "cus": info["num_cus"], "cus2": 2 * info["num_cus"]}
        out = {m: (torch.empty((B, N, D), dtype=torch.float32, device=dev),
                   torch.empty((B, N, D), dtype=torch.float32, device=dev),
                   torch.zeros((B, 8), dtype=torch.int32, device=dev)) for m in modes}
        bds = {m: batch_dev(start=start_t.data_ptr(), goal=goal_t.data_ptr(), obstacles=obs_t.data_ptr(), n_obstacles=O,
                            batch=B, alpha_out=o[0].data_ptr(), traj_out=o[1].data_ptr(), stats_out=o[2].data_ptr())
               for m, o in out.items()}
        groups, plans = {}, {}
        for m, req in modes.items():
            ctx.set_work_queue(req)
            groups[m] = ctx.work_queue_groups(B, O)
            plans[m] = ctx.launch_plan(B, O)

        def launch(m):
            ctx.set_work_queue(modes[m])
            ctx.optimize_dev(bds[m], stream.cuda_stream)

        for _ in range(a.warmup):
            for m in modes:
                launch(m)
        torch.cuda.synchronize(dev)
        evs = {m: [] for m in modes}
        for _ in range(a.reps):
            for m in modes:  # alternating: every mode sees the same clocks and neighbours
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch(m)
                e1.record(stream)
                evs[m].append((e0, e1))
        torch.cuda.synchronize(dev)
        ctx.set_work_queue(0)
        flow = {"optimizer": opt, "N": N, "D": D, "obstacles": O, "batch": B,
                "traj_per_block": plans["off"]["traj_per_block"], "static_grid": plans["off"]["grid"],
                "working_share": None,  # tools/faithful_rounds.py counts rounds per launch slot, not per loaded problem
                "modes": {}}
        ref = [t.cpu().numpy() for t in out["off"]]
        for m in modes:
            ms = np.array([e0.elapsed_time(e1) for e0, e1 in evs[m]])
            got = [t.cpu().numpy() for t in out[m]]
            flow["modes"][m] = {
                "groups": groups[m], "kernel": plans[m]["kernel"], "grid": plans[m]["grid"],
                "median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                "p25_ms": float(np.percentile(ms, 25)), "p75_ms": float(np.percentile(ms, 75)), "launches": len(ms),
                "bit_equal_to_off": bool(all(np.array_equal(x, y) for x, y in zip(got, ref))),
            }
        off = flow["modes"]["off"]
        flow["inner_iterations"] = {"min": int(ref[2][:, 0].min()), "mean": float(ref[2][:, 0].mean()),
                                    "max": int(ref[2][:, 0].max())}
        for m in modes:
            flow["modes"][m]["vs_off"] = flow["modes"][m]["median_ms"] / off["median_ms"]
        result["flows"][cfg] = flow
        print(cfg, json.dumps(flow["modes"]), flush=True)
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    bad = [(c, m) for c, fl in result["flows"].items() for m, r in fl["modes"].items() if not r["bit_equal_to_off"]]
    if bad:
        print("NOT bit-equal:", bad)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
