"""Timing of irm_transfer_alpha_dev and irm_fit_alpha_dev on device buffers, next to the optimiser launch they precede.

    python tools/fit_bench.py [--batch 1024] [--reps 50] [--warmup 5] [--out profiles/fit_bench.txt]

Shapes: B = 1024 problems at N = 128 and N = 256, D = 3 and 7.  The transfer is the receding-horizon one
(n_src = N, t0 = 0.25, t1 = 1, with start_out); the fit takes the waypoints of the same α.  Launches are timed with
device events around the enqueue on the caller's stream (tools/dense_check_bench.py's scheme: warm-up launches, then
`reps` timed ones, median, min and max reported; then one event pair around `reps` back-to-back launches).  Per row: ms per call, the fp64 FMAs of the operator product
(B·N·n_src·D) over that time, and the bytes the kernel must move at least (α in and out once; the operator once per
workgroup is L2 traffic and not counted).  The vector fp64 peak of the device is not measured here, so no share of
peak is given.

For scale, measured in the same run: the optimiser launch a transfer precedes — bench.py's C3 step, irm_optimize_batch_dev
for 1024 problems at N = 128, D = 3, 11 obstacles, 200 fixed GD iterations — timed the same way.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(128, 3), (128, 7), (256, 3), (256, 7)]
TAU = 0.25


def timed(torch, stream, launch, warmup, reps):
    for _ in range(warmup):
        launch()
    stream.synchronize()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        evs.append((e0, e1))
    stream.synchronize()
    # one window around `reps` back-to-back launches: launch gaps included, event resolution excluded
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        launch()
    t1.record(stream)
    stream.synchronize()
    return np.array([e0.elapsed_time(e1) for e0, e1 in evs]), t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fit_bench.txt"))
    a = ap.parse_args()

    import torch
    from irm_motion_planning_amd import main as irm_main
    from irm_motion_planning_amd.context import Context, batch_dev
    from irm_motion_planning_amd.environment import OBSTACLES
    from irm_motion_planning_amd.params import params_from_args

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    B = a.batch
    lines = [f"fit_bench: batch {B}, {a.warmup} warm-up + {a.reps} timed launches per row, device events, "
             f"{torch.cuda.get_device_name(dev)}"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    def shape_args(N, D, extra=()):
        argv = ["--n-timesteps", str(N), "--n-joints", str(D)] + list(extra)
        if D != 3:
            argv += ["--link-length"] + [str(3.0 / D)] * D
        return irm_main.parse_args(argv)

    for N, D in SHAPES:
        ctx = Context(params_from_args(shape_args(N, D)))
        rng = np.random.default_rng(1)
        s = rng.uniform(-0.5, 0.5, (B, D)).astype(np.float32)
        g = rng.uniform(0.2, 1.6, (B, D)).astype(np.float32)
        alpha = ctx.init_alpha(s, g)
        ctx.set_transfer(N, t0=TAU, t1=1.0)
        a_t = torch.from_numpy(alpha).to(dev)
        q_t = torch.from_numpy(ctx.evaluate(alpha, 0)).to(dev)
        out_t = torch.empty_like(a_t)
        start_t = torch.empty((B, D), dtype=torch.float32, device=dev)
        calls = {
            "transfer_alpha_dev": lambda: ctx.transfer_alpha_dev(a_t.data_ptr(), B, out_t.data_ptr(), start_t.data_ptr(),
                                                                 stream.cuda_stream),
            "fit_alpha_dev": lambda: ctx.fit_alpha_dev(q_t.data_ptr(), B, out_t.data_ptr(), stream.cuda_stream),
        }
        for name, launch in calls.items():
            ms, train = timed(torch, stream, launch, a.warmup, a.reps)
            med = float(np.median(ms))
            fma = B * N * N * D
            emit(f"{name:20s} N={N:3d} D={D}: median {med:.4f} ms (min {ms.min():.4f}, max {ms.max():.4f}; "
                 f"{train:.4f} ms per launch back to back), "
                 f"{fma / (med * 1e-3) / 1e9:.1f} fp64 GFMA/s, {2 * B * N * D * 4 / (med * 1e-3) / 1e9:.1f} GB/s of alpha in + out")
        ctx.close()

    # the launch a transfer precedes: bench.py's C3 step
    N, D, O, iters = 128, 3, 11, 200
    args = shape_args(N, D, ["--optimizer-name", "gd", "--loop-loss-reduction=-1e30", "--max-outer-iteration=1",
                             f"--max-inner-iteration={iters}"])
    ctx = Context(params_from_args(args))
    rng = np.random.default_rng(1)
    s_t = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, D)).astype(np.float32)).to(dev)
    g_t = torch.from_numpy(rng.uniform(0.2, 1.6, (B, D)).astype(np.float32)).to(dev)
    obs_t = torch.from_numpy(OBSTACLES[:O].astype(np.float32)).to(dev)
    ao_t = torch.empty((B, N, D), dtype=torch.float32, device=dev)
    to_t = torch.empty((B, N, D), dtype=torch.float32, device=dev)
    st_t = torch.zeros((B, 8), dtype=torch.int32, device=dev)
    bd = batch_dev(start=s_t.data_ptr(), goal=g_t.data_ptr(), obstacles=obs_t.data_ptr(), n_obstacles=O, batch=B,
                   alpha_out=ao_t.data_ptr(), traj_out=to_t.data_ptr(), stats_out=st_t.data_ptr())
    ms, train = timed(torch, stream, lambda: ctx.optimize_dev(bd, stream.cuda_stream), a.warmup, min(a.reps, 20))
    emit(f"{'optimize_batch_dev':20s} N={N:3d} D={D}: median {float(np.median(ms)):.4f} ms (min {ms.min():.4f}, max {ms.max():.4f}; "
         f"{train:.4f} ms per launch back to back), "
         f"C3: {O} obstacles, {iters} fixed GD iterations, kernel {ctx.launch_plan(B, O)['kernel']}")
    ctx.close()
    emit("share of the fp64 peak: not measured")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
