"""Drop-in CLI: the reference's main.py (main.py:13-153) on the HIP backend.

Keeps every flag of the reference argparser with its default and meaning,
the stdout lines ("setup object, jit-compile took", "took X ms",
"runtimes in ms: mean M stddev S", the constraint report and
"result cost: ( avg A , max M ). constraint fulfiled F") and the output
files trajectory_result.txt / trajectory_series.txt (np.savetxt defaults).

Additive flags (no reference counterpart): --batch-size, --seed,
--operator-rank, --device, --whole-robot-cost, --work-queue, --dense-check
(which adds one stdout line and trajectory_result_dense.txt),
--coarse-n-timesteps (coarse-to-fine: two stdout lines per optimize()),
--obstacle-velocity (obstacles that drift at a constant velocity over the plan),
--goal-xy (an end-effector target instead of a goal configuration; the goal number of the
"start goal position" line is then the Cartesian distance) and --via-joint / --via-xy (via-points:
interior support rows held to joint or end-effector targets; one stdout line names the chosen rows
and one reports the via distances), --clearance (the signed clearance between the arm's links and the obstacles as
discs on M samples: one stdout line, on the batched path a second one and a min_clearance column in the
summary file) with --obstacle-radius and --link-radius, --self-clearance (the same for the arm's links against each
other: one stdout line, on the batched path a second one and a min_self_clearance column), and --multi-start (S seeds per problem in one launch, the
best kept; ranked with the clearance check when --clearance is given, and with the self-clearance check when
--self-clearance is; prints the winner and the candidate table)
with --multi-start-amplitude and --multi-start-seed.
"""
import argparse
import os
import time

import numpy as np

from . import batch_io, distributed
from .optimizer_BLS import BacktrackingLineSearchOptimizer
from .optimizer_GD import GradientDescentOptimizer


def _bool(x):
    return str(x).lower() == "true"


def _work_queue(x):
    """--work-queue: off, auto, or a number of persistent workgroups (> 0)."""
    word = str(x).strip().lower()
    if word in ("off", "auto"):
        return word
    if not word.isdigit() or int(word) <= 0:
        raise argparse.ArgumentTypeError(f"expected off, auto or a positive workgroup count, got {x!r}")
    return int(word)


def build_parser():
    parser = argparse.ArgumentParser()
    # Profiling (main.py:16-23)
    parser.add_argument('--profiling', type=_bool, default=False,
                        help="Print per-call HIP timing breakdown (default: False)")
    parser.add_argument('--extended-vis', type=_bool, default=False,
                        help="Record the per-iteration trajectory series (default: False)")
    parser.add_argument('--n-measurements', type=int, default=1,
                        help="Number of measurements to be taken during one time measurement (default: 1)")
    parser.add_argument('--n-times', type=int, default=1,
                        help="Number of times the process is repeated to generate mean and stddev(default: 1)")
    # Optimizer (main.py:26-29)
    parser.add_argument('--optimizer-name', choices=['gd', 'bls'], default='bls',
                        help="Choose the optimizer: 'gd' for Gradient Descent, 'bls' for Backtracking Line Search")
    parser.add_argument('--jit-loop', type=_bool, default=True,
                        help="Run the whole loop as one persistent kernel (default: True)")
    # Trajectory (main.py:32-37)
    parser.add_argument('--n-timesteps', type=float, default=50,
                        help="Number of timesteps in the trajectory (default: 50)")
    parser.add_argument('--rbf-variance', type=float, default=0.1,
                        help="Variance parameter for Radial Basis Function (RBF) kernel (default: 0.1)")
    parser.add_argument('--jac-gaussian-mean', type=float, default=0.15,
                        help="Mean value for the Gaussian noise of the matrix J (default: 0.15)")
    # Minimization (main.py:40-43)
    parser.add_argument('--max-inner-iteration', type=int, default=200,
                        help="Maximum number of iterations for the inner optimization loop (default: 200)")
    parser.add_argument('--loop-loss-reduction', type=float, default=1e-3,
                        help="Minimum loss reduction threshold for each loop iteration (default: 1e-3)")
    # Constraint dual optimization (main.py:46-59)
    parser.add_argument('--max-outer-iteration', type=int, default=10,
                        help="Maximum number of iterations for the outer optimization loop (default: 10)")
    parser.add_argument('--lambda-constraint-increase', type=int, default=10,
                        help="Increase factor for lambda-sg-constraint and lambda-jl-constraint (default: 10)")
    parser.add_argument('--lambda-sg-constraint', type=float, default=0.5,
                        help="Initial weight for the SG (Start Goal) constraint (default: 0.5)")
    parser.add_argument('--lambda-jl-constraint', type=float, default=0.1,
                        help="Initial weight for the JL (Joint Limit) constraint (default: 0.1)")
    parser.add_argument('--eps-position', type=float, default=0.01,
                        help="Tolerance for start goal position constraints (default: 0.01)")
    parser.add_argument('--eps-velocity', type=float, default=0.01,
                        help="Tolerance for start goal velocity constraints (default: 0.01)")
    # Loss (main.py:62-69)
    parser.add_argument('--lambda-max-cost', type=float, default=0.5,
                        help="Maximum cost weight in the obstacle loss function (default: 0.5)")
    parser.add_argument('--lambda-reg', type=float, default=1e-4,
                        help="Regularization weight in the gradient update (default: 1e-4)")
    parser.add_argument('--constraint-violating-dependant-loss', type=_bool, default=True,
                        help="Enable or disable the loss dependency on constraint violations (default: True)")
    parser.add_argument('--joint-safety-limit', type=float, default=0.98,
                        help="Safety limit for the joint positions (default: 0.98)")
    # BLS (main.py:72-81)
    parser.add_argument('--max-bls-iteration', type=int, default=20,
                        help="Maximum number of iterations for the Backtracking Line Search (default: 20)")
    parser.add_argument('--bls-lr-start', type=float, default=0.2, help="Initial learning rate for BLS (default: 0.2)")
    parser.add_argument('--bls-alpha', type=float, default=0.01,
                        help="Alpha parameter for BLS, sufficient decrease condition (default: 0.01)")
    parser.add_argument('--bls-beta_plus', type=float, default=1.2,
                        help="Multiplicative factor to increase the learning rate in BLS (default: 1.2)")
    parser.add_argument('--bls-beta_minus', type=float, default=0.5,
                        help="Multiplicative factor to decrease the learning rate in BLS (default: 0.5)")
    # GD (main.py:84-85)
    parser.add_argument('--gd-lr', type=float, nargs='+',
                        default=[2e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-8, 1e-8, 1e-8, 1e-8],
                        help="Learning rates for the dual optimization in Gradient Descent")
    # Robot (main.py:88-97)
    parser.add_argument('--n-joints', type=int, default=3, help="Number of joints in the robot (default: 3)")
    parser.add_argument('--link-length', type=float, nargs='+', default=[1.5, 1.0, 0.5],
                        help="Lengths of the robot's links, provided as a list (default: [1.5, 1.0, 0.5])")
    parser.add_argument('--max-joint-velocity', type=float, default=7,
                        help="Maximum velocity for the robot's joints (default: 7)")
    parser.add_argument('--max-joint-position', type=float, default=2,
                        help="Maximum allowable position for the robot's joints (default: 2)")
    parser.add_argument('--min-joint-position', type=float, default=-1,
                        help="Minimum allowable position for the robot's joints (default: -1)")
    # Additive (this build)
    parser.add_argument('--batch-size', type=int, default=1,
                        help="Optimise this many problems in one launch (>1: problem 0 is the reference "
                             "environment, the rest random start/goal; writes the batch files of batch_io.py)")
    parser.add_argument('--seed', type=int, default=1, help="Seed of the random batch problems (default: 1)")
    parser.add_argument('--operator-rank', type=int, default=0,
                        help="Kernel-operator rank inside the loop: 0 auto, -1 dense exact (default: 0)")
    parser.add_argument('--device', type=int, default=0, help="HIP device ordinal (default: 0)")
    parser.add_argument('--whole-robot-cost', type=_bool, default=False,
                        help="Obstacle cost summed over every joint position instead of the end effector only "
                             "(blog 'Complete Robot Obstacle Avoidance'; default: False)")
    parser.add_argument('--work-queue', type=_work_queue, default='off', metavar='{off,auto,N}',
                        help="Batched path: run N persistent workgroups (auto: as many as the GPU holds) whose "
                             "finished slots claim the next problem, instead of one workgroup per fixed group of "
                             "problems; same results (default: off)")
    parser.add_argument('--dense-check', type=_sample_count, default=0, metavar='M',
                        help="After the report, evaluate the result on linspace(0, 1, M) — between the waypoints "
                             "the optimiser looked at — and print its obstacle cost, joint and velocity limits "
                             "there; writes trajectory_result_dense.txt (default: 0 = off)")
    parser.add_argument('--coarse-n-timesteps', type=_sample_count, default=0, metavar='Nc',
                        help="Coarse-to-fine: optimise on Nc support times first, carry that solution onto the "
                             "--n-timesteps grid (transfer_alpha) and optimise from it; the output files are the "
                             "fine stage's (default: 0 = off)")
    parser.add_argument('--obstacle-velocity', type=float, nargs=2, default=None, metavar=('VX', 'VY'),
                        help="Every obstacle of every problem drifts by (VX, VY) over the plan (t in [0, 1]): the "
                             "optimiser and --dense-check see obstacle o at p + t*(VX, VY) at plan time t "
                             "(default: absent = static obstacles)")
    parser.add_argument('--goal-xy', type=float, nargs=2, default=None, metavar=('X', 'Y'),
                        help="Plan to an end-effector target instead of a goal configuration: the end effector "
                             "of the last waypoint is held to (X, Y); the goal configuration (the initial line) is "
                             "the IK seed from the start.  With --batch-size, problem 0 takes (X, Y) and every "
                             "seeded problem the end-effector position of its seeded goal configuration "
                             "(default: absent = joint goal)")
    parser.add_argument('--via-joint', type=float, nargs='+', action='append', default=None, metavar='T_Q',
                        help="Via-point: at plan time T (0 < T < 1, snapped to the nearest support row) the robot "
                             "is held to the joint configuration q1 ... qD — given as T q1 ... qD; repeatable, at "
                             "most 4 via-points with --via-xy; every problem of a batch takes them "
                             "(default: absent)")
    parser.add_argument('--via-xy', type=float, nargs=3, action='append', default=None, metavar=('T', 'X', 'Y'),
                        help="Via-point: at plan time T the end effector is held to (X, Y); it passes through "
                             "and does not stop; repeatable (default: absent)")
    parser.add_argument('--clearance', type=_sample_count, default=0, metavar='M',
                        help="After the report (and --dense-check), evaluate the result on linspace(0, 1, M) and print "
                             "the smallest signed distance between the arm's links and the obstacles, taken as discs "
                             "of --obstacle-radius, where it occurs and how many samples collide; honours "
                             "--obstacle-velocity (default: 0 = off)")
    parser.add_argument('--obstacle-radius', type=_radius, default=0.0, metavar='R',
                        help="--clearance: the radius of every obstacle (default: 0 = points)")
    parser.add_argument('--link-radius', type=_radius, default=0.0, metavar='R',
                        help="--clearance: the arm's links as capsules of this radius (default: 0 = segments)")
    parser.add_argument('--self-clearance', type=_sample_count, default=0, metavar='M',
                        help="After the report (and --clearance), evaluate the result on linspace(0, 1, M) and print the "
                             "smallest signed distance between two links of the arm that share no joint, taken as "
                             "capsules of --link-radius, where it occurs and how many samples collide; with "
                             "--multi-start the candidates are also ranked with it, on --clearance's samples when "
                             "that is given too (default: 0 = off)")
    parser.add_argument('--multi-start', type=_seed_count, default=0, metavar='S',
                        help="Run S seeds per problem in one launch — the straight line plus S-1 smooth random bumps — "
                             "and keep the best by (constraints fulfilled, collision-free, loss); collisions count when "
                             "--clearance M is given, with its radii; prints the winner and the candidate table "
                             "(default: 0 = off)")
    parser.add_argument('--multi-start-amplitude', type=_radius, default=1.0, metavar='A',
                        help="--multi-start: the bumps' amplitudes are uniform in [-A, A) per joint (default: 1.0)")
    parser.add_argument('--multi-start-seed', type=int, default=0, metavar='K',
                        help="--multi-start: seed of the bumps' hash (default: 0)")
    return parser


def _seed_count(x):
    """--multi-start: 0 (off) or a number of seeds in [1, 64]."""
    word = str(x).strip()
    if not word.isdigit() or int(word) > 64:
        raise argparse.ArgumentTypeError(f"expected a seed count in [0, 64], got {x!r}")
    return int(word)


def multistart_report(info):
    """--multi-start: the winner and the candidate table of problem 0 (Context.optimize_multistart's info)."""
    first = np.ndim(info["winner"]) == 0
    pick = (lambda a: np.asarray(a)) if first else (lambda a: np.asarray(a)[0])  # noqa: E731
    winner, rank, st = int(pick(info["winner"])), pick(info["rank"]), {k: pick(v) for k, v in info["stats"].items()}
    ncol = pick(info["reports"]["n_colliding"]) if "reports" in info else None
    if "self_reports" in info:  # --self-clearance: the ranking saw both checks' counts
        ncol = pick(info["self_reports"]["n_colliding"]) + (0 if ncol is None else ncol)
    print("multi-start:", info["n_seeds"], "seeds, winner candidate", winner,
          "(ranked by constraints" + (", collisions" if ncol is not None else "") + ", loss)")
    for s in range(len(rank)):
        print("  candidate", s, ": rank", int(rank[s]), ", constraint fulfiled", bool(st["constraints_ok"][s]),
              *((", colliding samples", int(ncol[s])) if ncol is not None else ()),
              ", final loss", np.float32(st["final_loss"][s]), ", inner iterations", int(st["inner_iterations"][s]))
    if not first:
        w = np.asarray(info["winner"])
        print("multi-start: the winner is candidate 0 (the plain seed) in", int(np.sum(w == 0)), "of", len(w), "problems")


def _radius(x):
    """--obstacle-radius / --link-radius: a finite length ≥ 0."""
    try:
        r = float(x)
    except ValueError:
        r = -1.0
    if not (0.0 <= r < float("inf")):
        raise argparse.ArgumentTypeError(f"expected a radius >= 0, got {x!r}")
    return r


def _sample_count(x):
    """--dense-check: a number of samples ≥ 0."""
    word = str(x).strip()
    if not word.isdigit():
        raise argparse.ArgumentTypeError(f"expected a sample count >= 0, got {x!r}")
    return int(word)


def parse_args(argv=None):
    return build_parser().parse_args(argv)


DENSE_RESULT = "trajectory_result_dense.txt"


def coarse_context(args):
    """--coarse-n-timesteps Nc: a second context with the hyper-parameters of `args` on Nc support times."""
    import copy

    from .context import Context
    from .params import params_from_args
    ca = copy.copy(args)
    ca.n_timesteps = args.coarse_n_timesteps
    knobs = {k: getattr(args, k) for k in ("operator_rank", "device") if hasattr(args, k)}
    return Context(params_from_args(ca, record_series=0, **knobs))


def print_stages(stages):
    """Both stages' statistics of a coarse-to-fine optimize(), one line each (sums over the batch)."""
    for name in ("coarse", "fine"):
        st = {k: np.atleast_1d(v) for k, v in stages[name]["stats"].items()}
        print(name, "stage, N =", stages[name]["n_timesteps"], ": inner iterations", int(np.sum(st["inner_iterations"])),
              ", outer iterations", int(np.sum(st["outer_iterations"])), ", gradient evaluations",
              int(np.sum(st["grad_evals"])), ", constraint fulfiled", int(np.sum(st["constraints_ok"])), "of",
              len(st["constraints_ok"]), ", final loss mean", float(np.mean(st["final_loss"])))


def dense_report(context, alpha, obstacles, M, obstacle_velocity=None):
    """--dense-check M: the result on linspace(0, 1, M).  Prints problem 0's line, writes its M×D positions
    and returns the batch's report (Context.dense_check; obstacle_velocity: the --obstacle-velocity table)."""
    t = np.linspace(0, 1, M, dtype=np.float32)
    context.set_eval_times(t)
    alpha = np.asarray(alpha, np.float32)
    rep = context.dense_check(alpha, obstacles, obstacle_velocity=obstacle_velocity)
    first = {k: (v if alpha.ndim == 2 else v[0]) for k, v in rep.items()}
    f32 = np.float32
    print(f"dense check ({M} samples): max cost", f32(first["max_cost"]), "at t=" + str(t[int(first["argmax_cost"])]) + ";",
          "joint limit", "ok" if first["position_ok"] else "exceeded", "with", f32(first["max_position"]),
          str(f32(first["min_position"])) + ";",
          "velocity limit", "ok" if first["velocity_ok"] else "exceeded", "with", f32(first["max_abs_velocity"]))
    np.savetxt(DENSE_RESULT, context.eval_any(alpha if alpha.ndim == 2 else alpha[0], 0))
    return rep


def clearance_report(context, alpha, obstacles, args, obstacle_velocity=None):
    """--clearance M: the links' clearance on linspace(0, 1, M).  Prints problem 0's line and returns the batch's
    report (Context.clearance; obstacle_velocity: the --obstacle-velocity table)."""
    M = args.clearance
    t = np.linspace(0, 1, M, dtype=np.float32)
    context.set_eval_times(t)
    alpha = np.asarray(alpha, np.float32)
    rep = context.clearance(alpha, obstacles, obstacle_velocity=obstacle_velocity,
                            obstacle_radius=args.obstacle_radius, link_radius=args.link_radius)
    first = {k: (v if alpha.ndim == 2 else v[0]) for k, v in rep.items()}
    if int(first["argmin_time"]) < 0:
        where = "no obstacles"
    else:
        where = ("at t=" + str(t[int(first["argmin_time"])]) + " link " + str(int(first["argmin_link"])) + " obstacle " +
                 str(int(first["argmin_obstacle"])))
    if first["collision_free"]:
        verdict = "collision-free"
    else:
        verdict = (str(int(first["n_colliding"])) + " colliding samples, the first at t=" +
                   str(t[int(first["first_colliding"])]))
    print(f"clearance ({M} samples): min", np.float32(first["min_clearance"]), where + ";", verdict)
    return rep


def self_clearance_report(context, alpha, args):
    """--self-clearance M: the clearance of the links against each other on linspace(0, 1, M).  Prints problem 0's
    line and returns the batch's report (Context.self_clearance)."""
    M = args.self_clearance
    t = np.linspace(0, 1, M, dtype=np.float32)
    context.set_eval_times(t)
    alpha = np.asarray(alpha, np.float32)
    rep = context.self_clearance(alpha, link_radius=args.link_radius)
    first = {k: (v if alpha.ndim == 2 else v[0]) for k, v in rep.items()}
    if int(first["argmin_time"]) < 0:
        where = "no link pairs"
    else:
        where = ("at t=" + str(t[int(first["argmin_time"])]) + " link " + str(int(first["argmin_link_a"])) + " link " +
                 str(int(first["argmin_link_b"])))
    if first["collision_free"]:
        verdict = "collision-free"
    else:
        verdict = (str(int(first["n_colliding"])) + " colliding samples (" + str(int(first["n_crossing"])) +
                   " crossing), the first at t=" + str(t[int(first["first_colliding"])]))
    print(f"self-clearance ({M} samples): min", np.float32(first["min_clearance"]), where + ";", verdict)
    return rep


def run_batch(optimizer, args):
    """--batch-size B > 1: B problems in one launch per optimize().

    Timing lines as main.py:118-128 (one "took" per measurement, for the whole batch); the
    reference's report and files for problem 0 (the reference environment); batch files
    and a one-line batch summary (batch_io.py).

    Under torchrun (WORLD_SIZE > 1, one process per GPU) the batch is sharded:
    rank 0's environment and problems are broadcast, every rank optimises its rows
    [lo, hi), the results are gathered to rank 0, which reports and writes the files."""
    env, tr = optimizer.env, optimizer.trajectory
    world, rank, _ = distributed.world_info()
    B = args.batch_size
    start, goal = batch_io.batch_problems(B, tr.robot.N_joints, args.seed)
    goal_xy = None
    if optimizer.goal_xy is not None:
        # --goal-xy: every seeded problem is planned to the end-effector position of its seeded goal
        # configuration, problem 0 (the environment's) to the flag's target from its IK seed
        links = np.asarray(tr.robot.link_length, np.float64)[:tr.robot.N_joints]
        angles = np.cumsum(goal.astype(np.float64), axis=1)
        goal_xy = np.stack([(links * np.cos(angles)).sum(1), (links * np.sin(angles)).sum(1)], axis=1).astype(np.float32)
        goal_xy[0] = optimizer.goal_xy
        goal = np.array(goal, np.float32)
        goal[0] = env.goal_config
    lo, hi = 0, B
    dev = "cpu"
    if world > 1:
        import torch
        dev = torch.device("cuda", args.device) if torch.distributed.get_backend() == "nccl" else "cpu"
        if goal_xy is None:
            obs, start, goal = distributed.broadcast_environment(env.obstacles, start, goal, dev)
        else:  # the targets are sharded with the goals
            obs, start, goal, goal_xy = distributed.broadcast_environment(env.obstacles, start, goal, dev, goal_xy=goal_xy)
        env.obstacles = obs
        lo, hi = distributed.shard(B, world, rank)
    xy = None if goal_xy is None else goal_xy[lo:hi]
    wq = getattr(args, "work_queue", "off")
    if wq != "off":  # this process's launch (single GPU, or this rank's shard)
        ctx = optimizer.context
        ctx.set_work_queue(wq)
        n_obs = int(np.asarray(env.obstacles).reshape(-1, 2).shape[0])
        if ctx.work_queue_groups(hi - lo, n_obs, args.extended_vis) == 0 and rank == 0:
            print("work queue", wq, "ignored: this launch runs one workgroup per group of problems")
    coarse = coarse_context(args) if getattr(args, "coarse_n_timesteps", 0) > 0 else None
    runtimes = []
    res = None
    for _ in range(args.n_measurements):
        st = time.time()
        for _ in range(args.n_times):
            if coarse is not None:  # this process's problems (single GPU, or this rank's shard)
                res = optimizer.coarse_to_fine(coarse, start[lo:hi], goal[lo:hi], env.obstacles, series=args.extended_vis,
                                               goal_xy=xy)
            else:
                res = optimizer.optimize_batch(start[lo:hi], goal[lo:hi], env.obstacles, series=args.extended_vis,
                                               goal_xy=xy, problem_offset=distributed.problem_offset(B, world, rank))
        et = time.time()
        if world > 1:
            et = st + distributed.reduce_timing(et - st, 0, dev)[0]
        runtimes.append(1000 * (et - st) / args.n_times)
        if rank == 0:
            print("took", 1000 * (et - st) / args.n_times, "ms")
    if args.n_measurements > 1 and rank == 0:
        print("runtimes in ms: mean", np.mean(runtimes), "stddev", np.std(runtimes))
    if coarse is not None and rank == 0:
        print_stages(optimizer.last_stages)
    alpha, traj, stats = res[:3]
    series = res[3] if args.extended_vis else None
    if optimizer.multi_start and rank == 0:  # (under torchrun: rank 0's shard)
        multistart_report(optimizer.last_multistart)
    if world > 1:
        parts = {"alpha": alpha, "traj": traj}
        parts.update({"stat_" + k: np.asarray(v) for k, v in stats.items()})
        if series is not None:
            parts["series"] = series
        full = distributed.gather_batch(parts, B, dev)  # rank 0 only
        if rank != 0:
            return alpha  # this rank's shard
        alpha, traj = full["alpha"], full["traj"]
        stats = {k[5:]: v for k, v in full.items() if k.startswith("stat_")}
        series = full.get("series")
    avg = tr.compute_trajectory_cost(alpha, env.obstacles, start, goal, 0, 0, 0)
    mx = tr.compute_trajectory_cost(alpha, env.obstacles, start, goal, 0, 0, 1)
    if optimizer.via is None:
        ok, _ = optimizer.context.constraints(alpha, start, goal, goal_xy=goal_xy)
    else:
        ok, _, vdist = optimizer.context.constraints(alpha, start, goal, goal_xy=goal_xy, via=optimizer.via)
        print("via distances: max over the batch", [float(d) for d in np.max(vdist, axis=0)])
    print("batch of", len(alpha), "problems" + (f" on {world} GPUs" if world > 1 else "") +
          ": constraint fulfiled", int(np.sum(ok)), "of", len(alpha),
          "; avg cost mean", float(np.mean(avg)), ", max cost mean", float(np.mean(mx)),
          "; inner iterations", int(np.sum(stats["inner_iterations"])))
    ok0 = tr.constraintsFulfilledVerbose(alpha[0], start[0], goal[0], verbose=True,
                                         goal_xy=None if goal_xy is None else goal_xy[0])
    print("result cost: ( avg", avg[0], ", max", mx[0], "). constraint fulfiled", ok0)
    if getattr(args, "dense_check", 0) > 0:
        rep = dense_report(optimizer.context, alpha, env.obstacles, args.dense_check, optimizer.obstacle_velocity)
        dense_ok = rep["position_ok"] & rep["velocity_ok"]
        print("dense check:", int(np.sum(np.asarray(ok, bool) & ~dense_ok)), "of", int(np.sum(ok)),
              "problems that fulfil the constraints on the support grid exceed a joint or velocity limit between "
              "the waypoints")
    batch_io.write_result(batch_io.RESULT, traj[0])
    batch_io.write_result_batch(batch_io.RESULT_BATCH, traj)
    min_clearance = None
    if getattr(args, "clearance", 0) > 0:
        rep = clearance_report(optimizer.context, alpha, env.obstacles, args, optimizer.obstacle_velocity)
        print("clearance:", int(np.sum(np.asarray(ok, bool) & ~rep["collision_free"])), "of", int(np.sum(ok)),
              "problems that fulfil the constraints on the support grid collide")
        min_clearance = rep["min_clearance"]
    if getattr(args, "self_clearance", 0) > 0:
        rep = self_clearance_report(optimizer.context, alpha, args)
        print("self-clearance:", int(np.sum(np.asarray(ok, bool) & ~rep["collision_free"])), "of", int(np.sum(ok)),
              "problems that fulfil the constraints on the support grid self-collide")
        batch_io.write_summary(batch_io.SUMMARY_BATCH, avg, mx, ok, stats, min_clearance=min_clearance,
                               min_self_clearance=rep["min_clearance"])
    else:
        batch_io.write_summary(batch_io.SUMMARY_BATCH, avg, mx, ok, stats, min_clearance=min_clearance)
    if series is not None:
        lens = stats["series_len"]
        frames0 = series[0][: int(lens[0])]
        print(frames0.shape)
        batch_io.write_series(batch_io.SERIES, frames0, tr.N_timesteps, tr.robot.N_joints)
        batch_io.write_series_batch(batch_io.SERIES_BATCH, series, lens)
    return alpha


def main(argv=None):
    args = parse_args(argv)
    world, _, local = distributed.world_info()
    if world > 1:  # torchrun: one process per GPU
        import torch
        import torch.distributed as dist
        # IRM_DIST_BACKEND=gloo: host-side collectives (e.g. several ranks sharing one GPU in tests)
        backend = os.environ.get("IRM_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
        ngpu = torch.cuda.device_count()
        args.device = local % max(1, ngpu)
        if not dist.is_initialized():
            if backend == "nccl":
                torch.cuda.set_device(args.device)
                dist.init_process_group("nccl", device_id=torch.device("cuda", args.device))
            else:
                dist.init_process_group("gloo")
    if args.optimizer_name == 'bls':
        optimizer = BacktrackingLineSearchOptimizer(args)
    elif args.optimizer_name == 'gd':
        optimizer = GradientDescentOptimizer(args)
    else:  # unreachable (argparse choices); kept for parity with main.py:113-115
        print("FATAL: not defined optimizer", args.optimizer_name)
        raise SystemExit(-1)
    if args.batch_size > 1:
        return run_batch(optimizer, args)

    coarse = coarse_context(args) if args.coarse_n_timesteps > 0 else None

    def coarse_to_fine():
        """optimizer.optimize() through the coarse stage: α, or (α, series) with --extended-vis."""
        env = optimizer.env
        res = optimizer.coarse_to_fine(coarse, env.start_config, env.goal_config, series=args.extended_vis,
                                       goal_xy=optimizer.goal_xy)
        if args.extended_vis:
            return res[0][0], [np.array(f) for f in res[3][0][: int(res[2]["series_len"][0])]]
        return res[0][0]

    def multiple_optimizations():
        runtimes = []
        result = None
        for _ in range(args.n_measurements):
            st = time.time()
            for _ in range(args.n_times):
                result = optimizer.optimize() if coarse is None else coarse_to_fine()
            et = time.time()
            runtimes.append(1000 * (et - st) / args.n_times)
            print("took", 1000 * (et - st) / args.n_times, "ms")
        if args.n_measurements > 1:
            print("runtimes in ms: mean", np.mean(runtimes), "stddev", np.std(runtimes))
        return result

    if args.extended_vis:
        result_alpha, p = multiple_optimizations()
    else:
        result_alpha = multiple_optimizations()
    if coarse is not None:
        print_stages(optimizer.last_stages)
    if optimizer.multi_start:
        multistart_report(optimizer.last_multistart)
    if args.profiling:
        for k, v in optimizer.last_profile.items():
            print("profile", k, v)

    env, tr = optimizer.env, optimizer.trajectory
    avg_result_cost = tr.compute_trajectory_cost(result_alpha, env.obstacles, env.start_config, env.goal_config, 0, 0, 0)
    max_result_cost = tr.compute_trajectory_cost(result_alpha, env.obstacles, env.start_config, env.goal_config, 0, 0, 1)
    ok = tr.constraintsFulfilledVerbose(result_alpha, env.start_config, env.goal_config, verbose=True,
                                        goal_xy=optimizer.goal_xy)
    if optimizer.via is not None:  # the via constraint joins the flag; the reference-style report stays
        vok, _, vdist = optimizer.context.constraints(result_alpha, env.start_config, env.goal_config,
                                                      goal_xy=optimizer.goal_xy, via=optimizer.via)
        print("via distances:", [float(d) for d in vdist], "(eps_position", args.eps_position, ")")
        ok = bool(ok) and bool(vok)
    print("result cost: ( avg", avg_result_cost, ", max", max_result_cost, "). constraint fulfiled", ok)

    np_trajectory = np.array(tr.evaluate(result_alpha, tr.km, tr.jac))
    np.savetxt("trajectory_result.txt", np_trajectory)
    if args.dense_check > 0:
        dense_report(optimizer.context, result_alpha, env.obstacles, args.dense_check, optimizer.obstacle_velocity)
    if args.clearance > 0:
        clearance_report(optimizer.context, result_alpha, env.obstacles, args, optimizer.obstacle_velocity)
    if args.self_clearance > 0:
        self_clearance_report(optimizer.context, result_alpha, args)
    if args.extended_vis:
        p_np = np.array(p)
        print(p_np.shape)
        np.savetxt("trajectory_series.txt", p_np.reshape((-1, tr.robot.N_joints * tr.N_timesteps)))
    return result_alpha


if __name__ == "__main__":
    main()
