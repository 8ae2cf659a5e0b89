"""Dynamic environments: re-plan a batch as obstacles move.

In the reference, obstacles, start and goal are traced arguments of the jitted
optimiser (`jit_optimize(alpha, obstacles, start, goal)`, optimizer_BLS.py:127-131,
optimizer_GD.py:173-177), so a new environment re-uses the compiled loop
(DevBlog-Theme/blog-post.html:353-354), but every optimize() restarts from the
straight line of initTrajectory (optimizer_BLS.py:57-62).

`Replanner` is the MPC-style form of that on the device:

* one context (K, dK, the low-rank operator, J) and one set of HBM buffers serve
  every call; only the new obstacles / start / goal are copied in;
* with warm_start the next plan starts from the previous plan's α, which never
  leaves HBM (α_out of call k is α0 of call k+1, double-buffered);
* each call is one optimiser launch (k_lean / k_optimize) through irm_optimize_batch_dev on the
  caller's stream (torch provides device memory and the stream);
* advance(tau) re-times the remaining motion of the latest plan onto [0, 1] on the device and makes the
  plan's configuration at tau the new start (irm_transfer_alpha_dev), so a robot that has executed part
  of its plan warm-starts the next one from where it is.

* plan(..., obstacle_velocity=w) plans against obstacles that drift at a constant velocity over the
  plan (waypoint n sees obstacle o at p + t[n]·w); the velocity table lives on the device next to the
  obstacle table, and advance(tau) moves both to the new plan's time origin (advance_obstacles).

* plan(..., goal_xy=p) plans to end-effector targets (B×2 or 2) instead of goal configurations; the table
  lives on the device between plans (plan() without goal_xy and without goal keeps it), and advance(tau)
  carries it — the target is a point of the world, not of the plan's time.  Without a goal configuration the
  first such plan seeds its straight line with the IK seed (irm_ik_seed_dev), on the device.

* plan(..., via=ViaPoints(...)) holds interior support rows to joint or end-effector targets (via.py); the
  targets live on the device between plans, a plan that is not warm-started begins from Context.via_seed, and
  advance(tau) drops them — a re-timed via-point does not generally land on a support row, so the caller
  passes fresh ones.

The first call, or warm_start=False, is exactly Optimizer.optimize() for the batch.
A warm-started call equals irm_optimize_batch with alpha0 = the previous α_out bit for
bit (tests/test_gpu_parity.py::test_replanner_*).
"""
import numpy as np

from ._abi import STATS_FIELDS, IrmError
from .context import Context, batch_dev
from .params import params_from_args


def advance_obstacles(p, w, tau):
    """Obstacle tables of the plan that starts at plan time tau of the current one (Replanner.advance).

    In fp32, with tau rounded to fp32 and c = fl(1 − tau):
        p' = fl(p + fl(tau·w))      where each obstacle is at the old plan's time tau
        w' = fl(c·w)                the remaining motion is stretched to unit time
    so that an obstacle's position at the new plan's time s, p' + s·w', is its old position at
    tau + (1 − tau)·s.  Two roundings per element, no fused multiply-add.  Returns (p', w')."""
    p, w = np.asarray(p, np.float32), np.asarray(w, np.float32)
    tau = np.float32(tau)
    c = np.float32(1.0) - tau
    step = (tau * w).astype(np.float32)
    return (p + step).astype(np.float32), (c * w).astype(np.float32)


class Replanner:
    def __init__(self, args, batch, n_obstacles, per_problem_obstacles=False, device=None, **overrides):
        import torch
        dev = int(device if device is not None else getattr(args, "device", 0))
        overrides.setdefault("device", dev)
        # raises IrmError without a gfx950 device: there is no CPU fallback
        self.context = Context(params_from_args(args, **overrides))
        self.N, self.D, self.B, self.O = self.context.N, self.context.D, int(batch), int(n_obstacles)
        self.per_problem = bool(per_problem_obstacles)
        self.torch = torch
        self.device = torch.device("cuda", dev)
        f32 = dict(dtype=torch.float32, device=self.device)
        B, N, D, O = self.B, self.N, self.D, self.O
        self.start = torch.zeros((B, D), **f32)
        self.goal = torch.zeros((B, D), **f32)
        self.obstacles = torch.zeros(((B if self.per_problem else 1) * max(O, 1), 2), **f32)
        self.velocity = torch.zeros_like(self.obstacles)  # the obstacles' velocities (plan(obstacle_velocity=…))
        self.moving = False       # did the latest plan have velocities?
        self._have_obs = False    # is there a stored obstacle table (plan(obstacles=None))?
        self.goal_xy = torch.zeros((B, 2), **f32)  # end-effector targets (plan(goal_xy=…))
        self.task = False         # does the latest plan hold the end effector to goal_xy?
        self.via = None           # the stored via-points (plan(via=…)); None: no via-point
        self.via_target = None    # their targets on the device (B×V×D)
        self._alpha = [torch.zeros((B, N, D), **f32), torch.zeros((B, N, D), **f32)]
        self.traj = torch.zeros((B, N, D), **f32)
        self.stats = torch.zeros((B, len(STATS_FIELDS)), dtype=torch.int32, device=self.device)
        self.cur = 0          # index of the buffer holding the latest α
        self.planned = False  # is there a previous plan to warm-start from?
        self.calls = 0
        self._tau = None      # the tau of the transfer operator the context holds (advance)

    def _put(self, dst, x, shape):
        x = np.array(np.broadcast_to(np.asarray(x, np.float32), shape))  # writable copy
        dst.copy_(self.torch.from_numpy(x).reshape(dst.shape), non_blocking=False)

    def plan(self, obstacles=None, start=None, goal=None, warm_start=True, stream=None, obstacle_velocity=None,
             goal_xy=None, via=None):
        """Optimise the batch against `obstacles` (O×2, or B×O×2 per problem).

        start / goal (B×D or D) are kept from the previous call when None.  obstacles=None re-uses the
        stored table (as advance() left it; an IrmError on the first call) and, unless obstacle_velocity
        is given, the stored velocities; passing obstacles overrides the stored table, as fresh perception
        would, and then the obstacles are static unless obstacle_velocity (the obstacles' shape) says
        otherwise.  goal_xy (B×2 or 2): plan to these end-effector targets; a later plan() with neither
        goal nor goal_xy keeps them, one with a goal configuration alone goes back to the joint goal.  A
        first plan with goal_xy and no goal seeds the goal configuration with the IK seed from `start`.
        via (ViaPoints, via.py): hold interior support rows to joint or end-effector targets (V×D, or B×V×D per
        problem); a later plan() with via=None keeps them, an empty ViaPoints drops them, and advance() drops
        them too — a re-timed via-point does not generally land on a support row, so pass fresh ones after an
        advance.  A via plan that is not warm-started begins from Context.via_seed, as Context.optimize does.
        Returns the per-problem statistics (dict of numpy arrays, irm_stats fields); the plan
        stays on the device (alpha(), trajectory())."""
        torch = self.torch
        B, D, O = self.B, self.D, self.O
        want = (B, O, 2) if self.per_problem else (O, 2)
        if obstacles is None:
            if not self._have_obs:
                raise IrmError("the first plan() needs obstacles")
            obs = None
        else:
            obs = np.asarray(obstacles, np.float32)
            if obs.shape != want:
                raise IrmError(f"obstacles must have shape {want}, got {obs.shape}")
        vel = None
        if obstacle_velocity is not None:
            vel = np.asarray(obstacle_velocity, np.float32)
            if vel.shape != want:
                raise IrmError(f"obstacle_velocity must have shape {want}, got {vel.shape}")
            if not np.all(np.isfinite(vel)):
                raise IrmError("obstacle_velocity must be finite")
        if start is not None:
            self._put(self.start, start, (B, D))
        if goal is not None:
            self._put(self.goal, goal, (B, D))
        gxy = None
        if goal_xy is not None:
            gxy = np.asarray(goal_xy, np.float32)
            if gxy.shape not in ((B, 2), (2,)):
                raise IrmError(f"goal_xy must have shape {(B, 2)} or (2,), got {gxy.shape}")
            if not np.all(np.isfinite(gxy)):
                raise IrmError("goal_xy must be finite")
            self._put(self.goal_xy, gxy, (B, 2))
            self.task = True
        elif goal is not None:
            self.task = False
        if via is not None:
            if len(via) == 0:
                self.via, self.via_target = None, None
            else:
                via.check_rows(self.N)
                tg = via.padded(B, D)
                if not via.read_entries_finite(B, D):  # (the entries that are read, as the library checks them)
                    raise IrmError("via targets must be finite")
                self.via = via
                self.via_target = torch.from_numpy(tg).to(self.device)
        if self.calls == 0 and (start is None or (goal is None and gxy is None)):
            raise IrmError("the first plan() needs start and goal (or goal_xy)")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if self.calls == 0 and goal is None:  # no goal configuration yet: the IK seed of the targets
            self.context.ik_seed_dev(self.start.data_ptr(), self.goal_xy.data_ptr(), B, self.goal.data_ptr(), 0,
                                     s.cuda_stream)
        if O and obs is not None:
            self._put(self.obstacles, obs.reshape(-1, 2), self.obstacles.shape)
        if O and vel is not None:
            self._put(self.velocity, vel.reshape(-1, 2), self.velocity.shape)
        if vel is not None or obs is not None:
            self.moving = vel is not None and O > 0
        self._have_obs = True
        warm = bool(warm_start) and self.planned
        a_in, a_out = self._alpha[self.cur], self._alpha[self.cur ^ 1]
        if self.via is not None and not warm:  # the via seed (Context.via_seed) is this plan's α0
            s.synchronize()
            a0 = self.context.via_seed(self.start.cpu().numpy(), self.goal.cpu().numpy(), self.via,
                                       goal_xy=self.goal_xy.cpu().numpy() if self.task else None)
            a_in.copy_(torch.from_numpy(np.ascontiguousarray(a0, np.float32).reshape(a_in.shape)))
            torch.cuda.current_stream(self.device).synchronize()
            warm = True
        bd = batch_dev(alpha0=a_in.data_ptr() if warm else 0, start=self.start.data_ptr(),
                       goal=self.goal.data_ptr(), obstacles=self.obstacles.data_ptr(), n_obstacles=O,
                       obstacle_stride=2 * O if self.per_problem else 0, batch=B, alpha_out=a_out.data_ptr(),
                       traj_out=self.traj.data_ptr(), stats_out=self.stats.data_ptr(),
                       obstacle_velocity=self.velocity.data_ptr() if self.moving else 0)
        self.context.optimize_dev(bd, s.cuda_stream, goal_xy_dev=self.goal_xy.data_ptr() if self.task else 0,
                                  via=self.via, via_target_dev=self.via_target.data_ptr() if self.via is not None else 0)
        self.cur ^= 1
        self.planned = True
        self.calls += 1
        s.synchronize()
        st = self.stats.cpu().numpy()
        out = {name: st[:, i].copy() for i, name in enumerate(STATS_FIELDS)}
        out["final_loss"] = st[:, STATS_FIELDS.index("final_loss")].view(np.float32).copy()
        return out

    def advance(self, tau, stream=None):
        """Receding horizon: the robot has executed the first `tau` (0 < tau < 1) of the latest plan.

        The rest of that plan, re-timed onto [0, 1], becomes the α that the next
        plan(obstacles, warm_start=True) starts from, and the plan's configuration at tau becomes
        self.start — where the robot now is.  One irm_transfer_alpha_dev launch from the current α buffer
        into the other one (the buffers flip; α never leaves HBM), enqueue-only on `stream`.  The
        transfer operator is rebuilt only when tau changes.

        The remaining duration is stretched to unit time: velocities in the new parametrisation are
        (1 − tau) times the old ones (a plan that kept the velocity limit keeps it).  trajectory() and
        the statistics still describe the plan before the advance until the next plan().

        Where the latest plan had obstacle velocities, world time stays consistent: the stored tables
        become, in fp32 with c = fl(1 − tau),
            p' = fl(p + fl(tau·w)),   w' = fl(c·w)
        (advance_obstacles: the obstacles where they are at the old plan's time tau, their remaining
        motion stretched to unit time), so plan() with obstacles=None continues against the same moving
        scene.  Both updates are enqueued on `stream` with the transfer; nothing leaves HBM.

        Stored via-points are dropped: their rows name support times of the old plan, and a re-timed via-point
        does not generally land on a support row of the new one — pass fresh ones to the next plan()."""
        if not self.planned:
            raise IrmError("advance() needs a plan: call plan() first")
        self.via, self.via_target = None, None
        tau = float(tau)
        if self._tau != tau:
            self.context.set_transfer(self.N, t0=tau, t1=1.0)  # IrmError unless tau is finite and < 1
            self._tau = tau
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        a_in, a_out = self._alpha[self.cur], self._alpha[self.cur ^ 1]
        self.context.transfer_alpha_dev(a_in.data_ptr(), self.B, a_out.data_ptr(), self.start.data_ptr(), s.cuda_stream)
        self.cur ^= 1
        if self.moving:
            t32 = np.float32(tau)
            c32 = np.float32(1.0) - t32
            with self.torch.cuda.stream(s):  # (separate multiply and add: two roundings, as advance_obstacles)
                self.obstacles.add_(self.velocity * float(t32))
                self.velocity.mul_(float(c32))

    def alpha(self):
        """The latest plan's α (B×N×D, device tensor)."""
        return self._alpha[self.cur]

    def alpha_host(self):
        return self._alpha[self.cur].cpu().numpy()

    def trajectory(self):
        """K·α·J of the latest plan (B×N×D, device tensor)."""
        return self.traj

    def trajectory_host(self):
        return self.traj.cpu().numpy()

