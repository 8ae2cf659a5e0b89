"""Shared body of the two optimizer classes (one persistent HIP launch per optimize())."""
import time

import numpy as np

from .environment import Environment
from .trajectory import Trajectory
from .via import via_from_args


class _PersistentOptimizer:
    """Reference object API: Optimizer(args); .optimize() -> α; .env; .trajectory.

    optimize() runs the whole outer/inner(/line-search) loop of the reference's
    jit variant in one persistent launch (k_lean or k_optimize, Context.launch_plan).
    With --extended-vis it also returns the per-iteration trajectory series the reference's plain loop
    records (in both loop modes — the reference supports it only with
    --jit-loop false).
    """

    kind = None

    def __init__(self, args, **overrides):
        self.args = args
        self.jitLoop = args.jit_loop
        self.extendedVis = args.extended_vis
        self.max_inner_iteration = args.max_inner_iteration
        self.max_outer_iteration = args.max_outer_iteration
        self.loop_loss_reduction = args.loop_loss_reduction
        self.lambda_constraint_increase = args.lambda_constraint_increase
        self.lambda_sg_constraint = args.lambda_sg_constraint
        self.lambda_jl_constraint = args.lambda_jl_constraint
        self.lambda_max_cost = args.lambda_max_cost
        self.lambda_reg = args.lambda_reg
        overrides.setdefault("record_series", 1 if self.extendedVis else 0)
        for knob in ("operator_rank", "device"):
            if hasattr(args, knob):
                overrides.setdefault(knob, getattr(args, knob))
        self.env = Environment()
        # --obstacle-velocity VX VY: every obstacle drifts by (VX, VY) over the plan (None: static obstacles)
        self.obstacle_velocity = None
        if getattr(args, "obstacle_velocity", None) is not None:
            self.obstacle_velocity = np.broadcast_to(np.asarray(args.obstacle_velocity, np.float32),
                                                     np.asarray(self.env.obstacles).shape).copy()
        self.trajectory = Trajectory(args, **overrides)
        self.context = self.trajectory.context
        # --goal-xy X Y: the environment's problem is planned to that end-effector target; its goal
        # configuration (the straight-line initialisation) becomes the IK seed from the start (None: joint goal)
        self.goal_xy = None
        if getattr(args, "goal_xy", None) is not None:
            self.goal_xy = np.asarray(args.goal_xy, np.float32)
            self.env.goal_config = self.context.ik_seed(self.env.start_config, self.goal_xy)[0]
        # --via-joint / --via-xy: interior support rows held to joint or end-effector targets, the same for every
        # problem of a batch (None: no via-point — the calls below are then the existing ones)
        self.via = via_from_args(args, self.context.N, self.context.D)
        if self.via is not None:
            print("via-points at support rows", self.via.rows, "of", self.context.N,
                  "(times", [float(t) for t in np.round(np.asarray(self.via.rows) / (self.context.N - 1), 4)], ")")
        # --multi-start S: every optimize() runs S seeds per problem and keeps the best (Context.optimize_multistart);
        # with --clearance M the candidates are ranked with the clearance check on linspace(0, 1, M) (0: off — the
        # calls below are then the existing ones)
        self.multi_start = int(getattr(args, "multi_start", 0) or 0)
        self.last_multistart = None
        if self.multi_start:
            if self.via is not None or self.extendedVis or getattr(args, "coarse_n_timesteps", 0) > 0:
                raise ValueError("--multi-start does not combine with via-points, --extended-vis or --coarse-n-timesteps")
            if getattr(args, "clearance", 0) > 0:
                self.context.set_eval_times(np.linspace(0, 1, args.clearance, dtype=np.float32))
            elif getattr(args, "self_clearance", 0) > 0:  # (both checks rank on one grid: --clearance's when given)
                self.context.set_eval_times(np.linspace(0, 1, args.self_clearance, dtype=np.float32))
        self.last_stats = None
        self.last_profile = {}
        t1 = time.time()
        self.optimize()  # the reference's warm-up (= XLA compile); here: first launch
        t2 = time.time()
        print("setup object, jit-compile took", 1000 * (t2 - t1), "ms")

    # ------------------------------------------------------------------ API
    def _multistart(self, start, goal, obstacles, vel, goal_xy, problem_offset=0):
        """optimize() through --multi-start: (alpha, traj, stats); self.last_multistart keeps the winner and the
        candidate table."""
        a = self.args
        ranked = getattr(a, "clearance", 0) > 0
        ranked_self = getattr(a, "self_clearance", 0) > 0
        if ranked_self:  # (the reports after the run set their own grids)
            self.context.set_eval_times(np.linspace(0, 1, a.clearance if ranked else a.self_clearance, dtype=np.float32))
        alpha, traj, stats, info = self.context.optimize_multistart(
            start, goal, obstacles, self.multi_start, seed=getattr(a, "multi_start_seed", 0),
            amplitude=getattr(a, "multi_start_amplitude", 1.0), problem_offset=problem_offset, rank_clearance=ranked,
            obstacle_radius=a.obstacle_radius if ranked else None,
            link_radius=a.link_radius if ranked or ranked_self else 0.0,
            obstacle_velocity=vel, goal_xy=goal_xy, candidates=True, rank_self_clearance=ranked_self)
        self.last_multistart = info
        return alpha, traj, stats

    def optimize(self):
        t0 = time.perf_counter()
        if self.multi_start:
            alpha, traj, stats = self._multistart(self.env.start_config, self.env.goal_config, self.env.obstacles,
                                                  self.obstacle_velocity, self.goal_xy)
            self.last_profile = {"optimize_ms": 1000 * (time.perf_counter() - t0)}
            self.last_stats = stats
            self.last_trajectory = traj
            return alpha
        res = self.context.optimize(self.env.start_config, self.env.goal_config, self.env.obstacles,
                                    series=self.extendedVis, obstacle_velocity=self.obstacle_velocity,
                                    goal_xy=self.goal_xy, via=self.via)
        self.last_profile = {"optimize_ms": 1000 * (time.perf_counter() - t0)}
        if self.extendedVis:
            alpha, traj, stats, series = res
            self.last_stats = stats
            return alpha, [np.array(s) for s in series]
        alpha, traj, stats = res
        self.last_stats = stats
        self.last_trajectory = traj
        return alpha

    def coarse_to_fine(self, coarse, start, goal, obstacles=None, series=False, goal_xy=None):
        """Coarse-to-fine optimize_batch(): solve the B problems on the support grid of `coarse` (a Context
        of the same hyper-parameters and another --n-timesteps), carry that solution onto this optimizer's
        grid (Context.set_transfer / transfer_alpha) and optimise from it.

        Returns optimize_batch()'s result of the fine stage; self.last_stages keeps both stages:
        {"coarse": {"n_timesteps", "alpha", "stats"}, "fine": {"n_timesteps", "alpha0", "stats"}}."""
        vel = self._velocity_for(obstacles)
        obstacles = self.env.obstacles if obstacles is None else obstacles
        D = self.trajectory.robot.N_joints
        start = np.asarray(start, np.float32).reshape(-1, D)
        goal = np.asarray(goal, np.float32).reshape(-1, D)
        # (the via-points of the coarse stage: the flags' times on the coarse grid)
        a_c, _, st_c = coarse.optimize(start, goal, obstacles, obstacle_velocity=vel, goal_xy=goal_xy,
                                       via=via_from_args(self.args, coarse.N, coarse.D))
        self.context.set_transfer(coarse.N, rbf_variance_src=coarse.params.rbf_variance)
        alpha0 = self.context.transfer_alpha(a_c)
        res = self.context.optimize(start, goal, obstacles, alpha0=alpha0, series=series, obstacle_velocity=vel,
                                    goal_xy=goal_xy, via=self.via)
        self.last_stats = res[2]
        self.last_stages = {"coarse": {"n_timesteps": coarse.N, "alpha": a_c, "stats": st_c},
                            "fine": {"n_timesteps": self.context.N, "alpha0": alpha0, "stats": res[2]}}
        return res

    def optimize_batch(self, start, goal, obstacles=None, alpha0=None, obstacle_stride=0, series=False, goal_xy=None,
                       problem_offset=0):
        """Batched optimize(): B independent start/goal problems (B×D each); goal_xy (B×2): end-effector
        targets instead of the goal configurations (which then only shape the initial line).

        Returns (alpha, traj, stats) — plus the B × S × N × D snapshot buffer with
        series=True (stats["series_len"] frames valid per problem)."""
        vel = self._velocity_for(obstacles)
        obstacles = self.env.obstacles if obstacles is None else obstacles
        start = np.asarray(start, np.float32).reshape(-1, self.trajectory.robot.N_joints)
        goal = np.asarray(goal, np.float32).reshape(-1, self.trajectory.robot.N_joints)
        if self.multi_start and alpha0 is None and not series:
            # problem_offset: the global index of start[0] (a shard's offset: the seeds then do not depend on the sharding)
            res = self._multistart(start, goal, obstacles, vel, goal_xy, problem_offset)
            self.last_stats = res[2]
            return res
        res = self.context.optimize(start, goal, obstacles, alpha0=alpha0, obstacle_stride=obstacle_stride,
                                    series=series, obstacle_velocity=vel, goal_xy=goal_xy, via=self.via)
        self.last_stats = res[2]
        return res

    def _velocity_for(self, obstacles):
        """The --obstacle-velocity table for `obstacles` (None: the environment's): the same drift for every
        obstacle of every problem; None without the flag."""
        if self.obstacle_velocity is None:
            return None
        if obstacles is None:
            return self.obstacle_velocity
        return np.broadcast_to(self.obstacle_velocity[0], np.asarray(obstacles).shape).copy()
