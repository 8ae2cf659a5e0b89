"""The yardstick of the moving-obstacle tests: an fp64 restatement and the scenes.

`MovingRef64` is `oracle.ref64.Ref64` with one change: `cost_tv` / `grad_ab` take the obstacle table per
waypoint, obs[n] = p + t[n]·w (fp64, from the fp32 inputs; `table`).  The obstacle moves with time, not
with α, so the gradient is the parent's formula with each waypoint's own positions.  Everything else —
`cost`, `cost_g`, `gd_single` — is inherited and works on such a table unchanged.  A plain O×2 table is
the parent's case; with w = 0 the results equal the parent's to the bit (the same expressions on the same
numbers, tests/test_moving_host.py).

The reference has no moving obstacles: this restatement, and bit-identity at zero velocity, are what the
feature is measured against.  whole_robot=True sums the potential over every joint position (robot.py:39-72),
which the parent does not restate; every joint position of waypoint n sees the table at t[n].
"""
import numpy as np

from conftest import oracle_for
from oracle.ref64 import Ref64


class MovingRef64(Ref64):
    def __init__(self, params, t, K, dK, J, whole_robot=False):
        super().__init__(params, K, dK, J)
        self.t = np.asarray(t, np.float32).astype(np.float64)  # the fp32 support times, widened
        self.whole_robot = bool(whole_robot)

    def table(self, p, w):
        """obs[n] = p + t[n]·w, N×O×2 in fp64 from the fp32 tables p, w (O×2)."""
        p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 2)
        w = np.asarray(w, np.float32).astype(np.float64).reshape(-1, 2)
        return p[None] + self.t[:, None, None] * w[None]

    def _per_waypoint(self, obs):
        obs = np.asarray(obs, np.float64)
        if obs.ndim == 3:
            return obs
        return np.broadcast_to(obs.reshape(-1, 2)[None], (self.N,) + obs.reshape(-1, 2).shape)

    def _joints(self, q):
        """Joint positions px, py (N×D) and the link vectors' angle derivatives sx, cy (N×D)."""
        c = np.cumsum(q, axis=1)
        px = np.cumsum(self.link * np.cos(c), axis=1)
        py = np.cumsum(self.link * np.sin(c), axis=1)
        return px, py, -(self.link * np.sin(c)), self.link * np.cos(c)

    def _potential(self, x, y, obs):
        """cv, ∂cv/∂x, ∂cv/∂y per waypoint for points (x, y) (N) against obs (N×O×2) — the parent's expressions."""
        dx = x[:, None] - obs[:, :, 0]
        dy = y[:, None] - obs[:, :, 1]
        den = 0.5 + 0.5 * (dx ** 2 + dy ** 2)
        return (0.8 / den).sum(1), (-0.8 * dx / den ** 2).sum(1), (-0.8 * dy / den ** 2).sum(1)

    def waypoint_cost(self, T, obs):
        """The obstacle potential per waypoint (N)."""
        obs = self._per_waypoint(obs)
        if not self.whole_robot:
            x, y, _, _ = self._fk(T)
            d2 = (x[:, None] - obs[:, :, 0]) ** 2 + (y[:, None] - obs[:, :, 1]) ** 2
            return (0.8 / (0.5 + 0.5 * d2)).sum(1)
        px, py, _, _ = self._joints(T)
        return sum(self._potential(px[:, j], py[:, j], obs)[0] for j in range(self.D))

    def cost_tv(self, T, V, obs, s, g, lsg, ljl, lmax):
        p, N = self.p, self.N
        cv = self.waypoint_cost(T, obs)
        toc = lmax * cv.max() + (1 - lmax) * cv.mean()
        sgp = 0.5 * np.sum((T[0] - s) ** 2) + 0.5 * np.sum((T[-1] - g) ** 2)
        sgv = 0.5 * np.sum(V[0] ** 2) + 0.5 * np.sum(V[-1] ** 2)
        z = (T - self.mean) / self.std
        mp = (T > self.hi) | (T < self.lo)
        jp = 0.5 * z ** 2
        if p.constraint_violating_dependant_loss:
            jp = np.where(mp, jp, 0.0)
        zv = V / p.max_joint_velocity
        mv = np.abs(V) > self.vthr
        jv = 0.5 * zv ** 2
        if p.constraint_violating_dependant_loss:
            jv = np.where(mv, jv, 0.0)
        return toc + lsg * (sgp + sgv) + ljl * (jp.sum() / N + jv.sum() / N)

    def grad_ab(self, T, V, obs, s, g, lsg, ljl, lmax):
        p, N = self.p, self.N
        obs = self._per_waypoint(obs)
        if not self.whole_robot:
            x, y, jx, jy = self._fk(T)
            dx = x[:, None] - obs[:, :, 0]
            dy = y[:, None] - obs[:, :, 1]
            den = 0.5 + 0.5 * (dx ** 2 + dy ** 2)
            cv = (0.8 / den).sum(1)
            gx = (-0.8 * dx / den ** 2).sum(1)
            gy = (-0.8 * dy / den ** 2).sum(1)
            w = np.full(N, (1 - lmax) / N)
            w[int(np.argmax(cv))] += lmax
            a = (w * gx)[:, None] * jx + (w * gy)[:, None] * jy
        else:
            px, py, sx, cy = self._joints(T)
            cv = np.zeros(N)
            da = np.zeros_like(T)  # ∂cv/∂q_k = Σ_j Σ_{k ≤ l ≤ j} (sx_l·gx_j + cy_l·gy_j)
            for j in range(self.D):
                cj, gxj, gyj = self._potential(px[:, j], py[:, j], obs)
                cv += cj
                for k in range(j + 1):
                    da[:, k] += sx[:, k:j + 1].sum(1) * gxj + cy[:, k:j + 1].sum(1) * gyj
            w = np.full(N, (1 - lmax) / N)
            w[int(np.argmax(cv))] += lmax
            a = w[:, None] * da
        b = np.zeros_like(V)
        a[0] += lsg * (T[0] - s)
        a[-1] += lsg * (T[-1] - g)
        b[0] += lsg * V[0]
        b[-1] += lsg * V[-1]
        mp = (T > self.hi) | (T < self.lo)
        jpg = (T - self.mean) / self.std ** 2 / N
        mv = np.abs(V) > self.vthr
        jvg = V / p.max_joint_velocity ** 2 / N
        if p.constraint_violating_dependant_loss:
            jpg = np.where(mp, jpg, 0.0)
            jvg = np.where(mv, jvg, 0.0)
        return a + ljl * jpg, b + ljl * jvg

    def max_potential(self, alpha, obs):
        """The largest per-waypoint obstacle potential of α's trajectory."""
        T, _ = self.traj_vel(alpha)
        return float(self.waypoint_cost(T, obs).max())


def restatement(*argv, whole_robot=False, **overrides):
    """(MovingRef64, CPU oracle) of a configuration: the oracle's fp32 t, K, dK, J are the library's."""
    if whole_robot:
        overrides["whole_robot_cost"] = 1
    o = oracle_for(*argv, **overrides)
    t, K, dK, J = o.kernel_matrices()
    return MovingRef64(o.params, t, K, dK, J, whole_robot=whole_robot), o


# ----------------------------------------------------------------------------------------------- scenes
LINKS7 = [0.7, 0.6, 0.5, 0.4, 0.35, 0.3, 0.25]


def shape_argv(N, D):
    argv = ["--n-timesteps", str(N), "--n-joints", str(D)]
    if D == 7:
        argv += ["--link-length"] + [str(x) for x in LINKS7]
    return argv


def dyadic_scene(O, B=1, seed=0):
    """Obstacle tables whose motion is exact in fp32 on a dyadic time grid: p multiples of 2⁻¹⁰ in [−3, 3],
    w multiples of 2⁻⁸ in [−2, 2] (p + τ·w is exact for τ a multiple of 2⁻⁶ with |τ| ≤ 4: at most 2⁻¹⁴ steps
    below 16, 18 bits).  Shapes (B, O, 2); B = None: (O, 2)."""
    rng = np.random.default_rng(1000 + 17 * O + seed)
    n = 1 if B is None else B
    p = (rng.integers(-3 * 1024, 3 * 1024 + 1, (n, O, 2)) / 1024.0).astype(np.float32)
    w = (rng.integers(-2 * 256, 2 * 256 + 1, (n, O, 2)) / 256.0).astype(np.float32)
    return (p[0], w[0]) if B is None else (p, w)


def crossing_tables(B, O, reach, seed=0):
    """Per-problem obstacles that cross the workspace (a disc of radius `reach`) during the plan: each starts
    on one side and ends on the other, so the table at t = 0 and the table a waypoint sees differ by up to the
    workspace's size.  Shapes (B, O, 2)."""
    rng = np.random.default_rng(2000 + seed)
    p = rng.uniform(-reach, reach, (B, O, 2))
    q = -p + rng.uniform(-0.3 * reach, 0.3 * reach, (B, O, 2))
    return p.astype(np.float32), (q - p).astype(np.float32)


def well_conditioned_alpha(o, B, D, seed=0):
    """α of moderate size (as the golden `small` vectors the whole-robot tests use): initTrajectory's line
    between random configurations is a numerically singular solve with |α| ~ 1e3, so instead the ridge-free
    small random α whose trajectory K·α·J stays inside the joint range.  Returns (alpha B×N×D, start, goal)."""
    rng = np.random.default_rng(3000 + seed)
    N = int(o.N)
    alpha = (0.05 * rng.standard_normal((B, N, D))).astype(np.float32)
    s = rng.uniform(-0.5, 0.5, (B, D)).astype(np.float32)
    g = rng.uniform(0.2, 1.6, (B, D)).astype(np.float32)
    return alpha, s, g


# The crossing scene (N = 33, D = 3, the reference arm and start / goal): one obstacle sweeps across the
# end effector's straight-line path during the plan.  Frozen at t = 0 it sits off the path, so a plan made
# against the frozen table keeps the line; the moving obstacle comes closest to the line's middle at mid-plan.
CROSSING_ARGV = ["--optimizer-name", "gd", "--max-outer-iteration", "1", "--max-inner-iteration", "200",
                 "--loop-loss-reduction=-1e30", "--n-timesteps", "33"]
# (the line's end effector runs from (3, 0) over (1.98, 2.14) at t = 0.5 to (−0.21, 2.68); the obstacle runs
# from (0.5, 0.5) to (2.5, 2.5) and crosses that path.  200 fp64 GD steps: moving loss 0.460 against 0.694 for
# the plan made against the frozen table, largest per-waypoint potential 0.612 against 0.963, largest potential
# on 129 times 0.614 against 0.966.  An obstacle fast enough to start far outside the workspace does not serve:
# its track still crosses the path, 200 steps shift the meeting by less than the gap between two waypoints, and
# both plans then pass within 0.05 of it between waypoints — on 129 times both reach 1.60.)
CROSSING_P = np.array([[0.5, 0.5]], np.float32)
CROSSING_W = np.array([[2.0, 2.0]], np.float32)
CROSSING_M = 129  # the dense check's sample count for this scene
