"""Time of the self-clearance check next to the obstacle clearance check of the same shape (reported, not a target).

    python tools/self_clearance_time.py [--reps 20] [--warmup 3] [--rounds 3] [--out profiles/self_clearance_time.json]

The problem is bench.py's C7 shape (1024 problems, N = 128, D = 7, the reference's 11 shared obstacles), the
trajectories the initial plans between its seeded starts and goals, evaluated on linspace(0, 1, 300), on device
buffers through the enqueue-only entry points:

  clearance       irm_clearance_dev        q of every sample, FK, the distance of every link to every obstacle; report only
  self            irm_self_clearance_dev   q of every sample, FK, the 15 link pairs (four distances, four orientations each)
  self_full       irm_self_clearance_dev   the same with clear_out, pair_out and joints_out written

Both kernels share the sampling (the fp64 contraction of Kq with α) and the FK prefix; they differ in the D passes over
the obstacle table against the P = 15 pairs.  Timing as tools/clearance_time.py: device events around each launch after
`warmup` launches per variant, the variants alternating within each round.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

M = 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "self_clearance_time.json"))
    a = ap.parse_args()

    import torch

    import bench
    from irm_motion_planning_amd.clearance import IrmClearanceReport, IrmSelfClearanceReport, self_pairs
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args

    desc, B, N, D, O, _ = bench.CONFIGS["c7"]
    start, goal, obstacles = bench.make_problem("c7", 1, 0)
    ctx = Context(params_from_args(bench.make_args("c7", False, 1), device=0))
    alpha = ctx.init_alpha(start, goal)
    ctx.set_eval_times(np.linspace(0, 1, M, dtype=np.float32))

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    alpha_t = torch.from_numpy(alpha).to(dev)
    obs_t = torch.from_numpy(np.ascontiguousarray(obstacles, np.float32)).to(dev)
    clear_rep = torch.zeros((B, ctypes.sizeof(IrmClearanceReport) // 4), dtype=torch.int32, device=dev)
    self_rep = torch.zeros((B, ctypes.sizeof(IrmSelfClearanceReport) // 4), dtype=torch.int32, device=dev)
    clear_t = torch.empty((B, M), dtype=torch.float32, device=dev)
    pair_t = torch.empty((B, len(self_pairs(D))), dtype=torch.float32, device=dev)
    joints_t = torch.empty((B, M, D, 2), dtype=torch.float32, device=dev)
    info = ctx.info()
    result = {"problem": desc, "batch": B, "N": N, "D": D, "M": M, "obstacles": O, "pairs": len(self_pairs(D)),
              "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup, "device": info["device_name"],
              "build_id": info["build_id"]}

    def clearance():
        ctx.clearance_dev(alpha_t.data_ptr(), obs_t.data_ptr(), O, 0, B, clear_rep.data_ptr(), stream=stream.cuda_stream)

    def self_():
        ctx.self_clearance_dev(alpha_t.data_ptr(), B, self_rep.data_ptr(), stream=stream.cuda_stream)

    def self_full():
        ctx.self_clearance_dev(alpha_t.data_ptr(), B, self_rep.data_ptr(), link_radius=0.05, clear_dev=clear_t.data_ptr(),
                               pair_dev=pair_t.data_ptr(), joints_dev=joints_t.data_ptr(), stream=stream.cuda_stream)

    variants = [("clearance", clearance), ("self", self_), ("self_full", self_full)]
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
    for name, _ in variants:
        x = np.array(ms[name])
        q1, q3 = np.percentile(x, [25, 75])
        result[name] = {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
                        "iqr_ms": float(q3 - q1), "round_medians_ms": [float(np.median(r)) for r in x],
                        "ns_per_problem_sample": 1e6 * float(np.median(x)) / (B * M), "launches": int(x.size)}
    result["self_over_clearance"] = result["self"]["median_ms"] / result["clearance"]["median_ms"]
    recs = self_rep.cpu().numpy()
    result["self_colliding_problems_full"] = int(np.count_nonzero(recs[:, 6] == 0))  # (link radius 0.05)
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
