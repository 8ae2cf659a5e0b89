"""Time the faithful GD single loop of the C3 line (default loop_loss_reduction, --max-outer-iteration 1):
the launch in which C3's GD1 kernel leaves its all-live loop in mid-launch, workgroup by workgroup, and
finishes in the general loop — the hand-over's cost, which bench.py's lines do not reach (its faithful
mode runs the dual loop).  Timed as bench.py times a step (events around optimize_dev).

    [IRM_LIB=…/libirm_hip_parent.so] python tools/gd1_handover.py [--steps 100] [--warmup 3] [--max-inner 200]

Prints one line: ms per launch (mean of the events), and the launch's gradient evaluations per trajectory."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from irm_motion_planning_amd import main as irm_main  # noqa: E402
from irm_motion_planning_amd.context import Context, batch_dev  # noqa: E402
from irm_motion_planning_amd.params import params_from_args  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--max-inner", type=int, default=200)
a = ap.parse_args()

start, goal, obstacles = bench.make_problem("c3", 1, 0)
B, N, D, O = len(start), 128, 3, len(obstacles)
args = irm_main.parse_args(["--optimizer-name", "gd", "--n-timesteps", str(N), "--max-outer-iteration", "1",
                            "--max-inner-iteration", str(a.max_inner)])
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
t = {k: torch.from_numpy(v).to(dev) for k, v in (("s", start), ("g", goal), ("o", obstacles))}
alpha = torch.empty((B, N, D), dtype=torch.float32, device=dev)
traj = torch.empty_like(alpha)
stats = torch.zeros((B, 8), dtype=torch.int32, device=dev)
ctx = Context(params_from_args(args, device=0))
plan = ctx.launch_plan(B, O)
bd = batch_dev(start=t["s"].data_ptr(), goal=t["g"].data_ptr(), obstacles=t["o"].data_ptr(), n_obstacles=O, batch=B,
               alpha_out=alpha.data_ptr(), traj_out=traj.data_ptr(), stats_out=stats.data_ptr())
stream = torch.cuda.current_stream(dev)
for _ in range(a.warmup):
    ctx.optimize_dev(bd, stream.cuda_stream)
torch.cuda.synchronize(dev)
evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
for e0, e1 in evs:
    e0.record(stream)
    ctx.optimize_dev(bd, stream.cuda_stream)
    e1.record(stream)
torch.cuda.synchronize(dev)
ms = float(np.mean([e0.elapsed_time(e1) for e0, e1 in evs]))
ge = stats.cpu().numpy()[:, 2]  # irm_stats.grad_evals (bench.py reads the same column)
print(f"gd1 faithful single loop: {plan['kernel']} ms_per_launch {ms:.4f} grad_evals min {ge.min()} "
      f"mean {ge.mean():.1f} max {ge.max()} checksum {int(ge.astype(np.int64).sum())}")
