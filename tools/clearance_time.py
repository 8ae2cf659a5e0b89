"""Time of the clearance check next to the dense check of the same shape (reported, not a target).

    python tools/clearance_time.py [--reps 20] [--warmup 3] [--rounds 3] [--out profiles/clearance_time.json]

The problem is bench.py's C3 shape (1024 problems, N = 128, D = 3, 11 shared obstacles), the trajectories the initial
plans between its seeded starts and goals, evaluated on linspace(0, 1, M) for M = 128 and 1024, on device buffers
through the enqueue-only entry points, three ways:

  dense      irm_dense_check_dev      q and v of every sample, FK, the obstacle potential at the end effector, the limits
  clearance  irm_clearance_dev        q of every sample, FK, the distance of every link to every obstacle; report only
  full       irm_clearance_dev        the same with radii, clear_out, link_out and joints_out written

The clearance kernel skips the velocity operator (half of the dense check's fp64 contraction) and does D passes
over the obstacle table, each with a clamped projection and a correctly rounded square root per obstacle, where the
potential does one pass with one reciprocal per obstacle.  Timing as tools/via_time.py: device events around each
launch after `warmup` launches per variant, the variants alternating within each round.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GRIDS = (128, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clearance_time.json"))
    a = ap.parse_args()

    import torch

    import bench
    from irm_motion_planning_amd import _abi
    from irm_motion_planning_amd.clearance import IrmClearanceReport
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args

    desc, B, N, D, O, _ = bench.CONFIGS["c3bls"]
    start, goal, obstacles = bench.make_problem("c3bls", 1, 0)
    ctx = Context(params_from_args(bench.make_args("c3bls", False, 1), device=0))
    alpha = ctx.init_alpha(start, goal)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    fp = _abi.c_float_p
    alpha_t = torch.from_numpy(alpha).to(dev)
    obs_t = torch.from_numpy(np.ascontiguousarray(obstacles, np.float32)).to(dev)
    rad_t = torch.full((O,), 0.2, dtype=torch.float32, device=dev)
    dense_rep = torch.zeros((B, ctypes.sizeof(_abi.IrmDenseReport) // 4), dtype=torch.int32, device=dev)
    clear_rep = torch.zeros((B, ctypes.sizeof(IrmClearanceReport) // 4), dtype=torch.int32, device=dev)
    link_t = torch.empty((B, D), dtype=torch.float32, device=dev)
    info = ctx.info()
    result = {"problem": desc, "batch": B, "N": N, "D": D, "obstacles": O, "reps": a.reps, "rounds": a.rounds,
              "warmup": a.warmup, "device": info["device_name"], "build_id": info["build_id"], "grids": {}}
    for M in GRIDS:
        ctx.set_eval_times(np.linspace(0, 1, M, dtype=np.float32))
        clear_t = torch.empty((B, M), dtype=torch.float32, device=dev)
        joints_t = torch.empty((B, M, D, 2), dtype=torch.float32, device=dev)

        def dense():
            _abi.check(ctx.lib.irm_dense_check_dev(
                ctx.handle, ctypes.cast(alpha_t.data_ptr(), fp), ctypes.cast(obs_t.data_ptr(), fp), O, 0, B,
                ctypes.cast(dense_rep.data_ptr(), ctypes.POINTER(_abi.IrmDenseReport)), None,
                ctypes.c_void_p(stream.cuda_stream)))

        def clearance():
            ctx.clearance_dev(alpha_t.data_ptr(), obs_t.data_ptr(), O, 0, B, clear_rep.data_ptr(),
                              stream=stream.cuda_stream)

        def full():
            ctx.clearance_dev(alpha_t.data_ptr(), obs_t.data_ptr(), O, 0, B, clear_rep.data_ptr(),
                              obstacle_radius_dev=rad_t.data_ptr(), link_radius=0.05, clear_dev=clear_t.data_ptr(),
                              link_dev=link_t.data_ptr(), joints_dev=joints_t.data_ptr(), stream=stream.cuda_stream)

        variants = [("dense", dense), ("clearance", clearance), ("full", full)]
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
        out = {}
        for name, _ in variants:
            x = np.array(ms[name])
            q1, q3 = np.percentile(x, [25, 75])
            out[name] = {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
                         "iqr_ms": float(q3 - q1), "round_medians_ms": [float(np.median(r)) for r in x],
                         "ns_per_problem_sample": 1e6 * float(np.median(x)) / (B * M), "launches": int(x.size)}
        free = int(np.count_nonzero(clear_rep.cpu().numpy()[:, 6]))
        out["collision_free_problems_full"] = free  # (what the last launch reported: radius 0.2, link radius 0.05)
        result["grids"][str(M)] = out
    ctx.close()
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
