"""Timing of irm_dense_check_dev (evaluation + checks at M arbitrary times) on device buffers.

    python tools/dense_check_bench.py [--batch 1024] [--reps 20] [--warmup 3] [--out profiles/dense_check.json]

Shapes: C3 (N = 128, D = 3, 10 obstacles) at M = 128, 1024, 4096 and C7 (N = 128, D = 7) at M = 1024, a batch
of 1024 trajectories each.  Launches are timed with device events around irm_dense_check_dev on the caller's
stream (tools/work_queue_ab.py's scheme: warm-up launches, then `reps` timed ones, the median reported).
Per shape: ms per call, ns per problem-sample, and the fp64 FMAs of the two contractions (B·M·N·D·2) over
that time.  The vector fp64 peak of the device is not measured here, so no share of peak is given.

For scale only, in the same process: the wall time of the host-pointer calls irm_eval_cost (the existing
evaluation of the N support waypoints) and irm_dense_check at M = N on the same batch — both include their
host-to-device copies and the synchronisation, so they bound the kernels from above and compare like with like.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [("c3", 128, 3, 128), ("c3", 128, 3, 1024), ("c3", 128, 3, 4096), ("c7", 128, 7, 1024)]
N_OBSTACLES = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dense_check.json"))
    a = ap.parse_args()

    import torch
    from irm_motion_planning_amd import _abi
    from irm_motion_planning_amd import main as irm_main
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.environment import OBSTACLES
    from irm_motion_planning_amd.params import params_from_args

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    fp = _abi.c_float_p
    B = a.batch
    obs = OBSTACLES[:N_OBSTACLES].astype(np.float32)
    obs_t = torch.from_numpy(obs).to(dev)
    result = {"batch": B, "reps": a.reps, "warmup": a.warmup, "obstacles": N_OBSTACLES,
              "share_of_fp64_peak": "not measured", "shapes": []}
    ctxs = {}
    for name, N, D, M in SHAPES:
        if (N, D) not in ctxs:
            argv = ["--n-timesteps", str(N), "--n-joints", str(D)]
            if D != 3:
                argv += ["--link-length"] + [str(3.0 / D)] * D
            ctx = Context(params_from_args(irm_main.parse_args(argv)))
            rng = np.random.default_rng(17)
            alpha = (rng.standard_normal((B, N, D)) * 0.2).astype(np.float32)
            s = rng.uniform(-0.5, 0.5, (B, D)).astype(np.float32)
            g = rng.uniform(0.2, 1.6, (B, D)).astype(np.float32)
            # scale: the host-pointer calls on the support grid (copies and synchronisation included)
            ctx.set_eval_times(ctx.kernel_matrices()[0])
            host = {}
            cost_h = np.zeros(B, np.float32)
            rep_h = (_abi.IrmDenseReport * B)()
            p = lambda x: x.ctypes.data_as(fp)  # noqa: E731  (the C calls themselves, preallocated buffers)
            for label, call in (
                    ("eval_cost", lambda: _abi.check(ctx.lib.irm_eval_cost(
                        ctx.handle, p(alpha), p(s), p(g), p(obs), N_OBSTACLES, B, 0.5, 0.1, 0.5, p(cost_h)))),
                    ("dense_check", lambda: _abi.check(ctx.lib.irm_dense_check(
                        ctx.handle, p(alpha), p(obs), N_OBSTACLES, 0, B, rep_h, None)))):
                call()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    call()
                    ts.append(1e3 * (time.perf_counter() - t0))
                host[label] = float(np.median(ts))
            ctxs[(N, D)] = (ctx, torch.from_numpy(alpha).to(dev), host)
        ctx, alpha_t, host = ctxs[(N, D)]
        ctx.set_eval_times(np.linspace(0, 1, M, dtype=np.float32))
        rep_t = torch.zeros((B, 10), dtype=torch.int32, device=dev)
        cost_t = torch.empty((B, M), dtype=torch.float32, device=dev)

        def launch():
            _abi.check(ctx.lib.irm_dense_check_dev(
                ctx.handle, ctypes.cast(alpha_t.data_ptr(), fp), ctypes.cast(obs_t.data_ptr(), fp), N_OBSTACLES, 0, B,
                ctypes.cast(rep_t.data_ptr(), ctypes.POINTER(_abi.IrmDenseReport)), ctypes.cast(cost_t.data_ptr(), fp),
                ctypes.c_void_p(stream.cuda_stream)))

        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize(dev)
        evs = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            evs.append((e0, e1))
        torch.cuda.synchronize(dev)
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in evs])
        med = float(np.median(ms))
        fma = B * M * N * D * 2
        row = {"config": name, "N": N, "D": D, "M": M, "median_ms": med, "min_ms": float(ms.min()),
               "max_ms": float(ms.max()), "launches": len(ms), "ns_per_problem_sample": 1e6 * med / (B * M),
               "fp64_fma": fma, "fp64_gfma_per_s": fma / (med * 1e-3) / 1e9,
               "scale_host_calls_on_support_grid": {
                   "eval_cost_ms": host["eval_cost"], "dense_check_ms": host["dense_check"],
                   "eval_cost_ns_per_problem_waypoint": 1e6 * host["eval_cost"] / (B * N),
                   "dense_check_ns_per_problem_sample": 1e6 * host["dense_check"] / (B * N)}}
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    for ctx, _, _ in ctxs.values():
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
