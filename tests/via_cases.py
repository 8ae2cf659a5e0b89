"""The yardstick of the via-point tests: an fp64 restatement, the seed recipe and the scenes.

`ViaRef64` is `task_cases.TaskRef64` with a `via` list — entries (row m, cartesian, target) — that `cost_tv`,
`grad_ab` and `constraints` consult (include/irm.h):

    loss         += λsg · ½ · Σ_v r_v²
    a[m_v]       += λsg · ge_v                (position gradient input of row m_v only; b is untouched)
    constraints  :  ok &= r_v < eps_position  for every v

with r_v = ‖T[m_v] − c‖, ge_v = T[m_v] − c for a joint via-point and r_v = ‖f(T[m_v]) − p‖,
ge_v = J_ee(T[m_v])ᵀ·(f(T[m_v]) − p) for an end-effector one (the Jacobian is the end effector's also with
whole_robot).  With an empty list every method is the parent's, to the bit.  `cost`, `cost_g`, `gd_single` and
`bls` are inherited.  The reference has no via-points: this restatement, and bit-identity of the via-free calls,
are what the feature is measured against.
"""
import functools

import numpy as np

import moving_cases as mc
import task_cases as tc
from task_cases import TaskGoal, TaskRef64


class ViaRef64(TaskRef64):
    def __init__(self, *args, via=(), **kw):
        super().__init__(*args, **kw)
        self.via = list(via)

    def with_via(self, via):
        """A copy of this restatement with another via list."""
        R = ViaRef64(self.p, self.t.astype(np.float32), self.K, self.dK, self.J, whole_robot=self.whole_robot, via=via)
        return R

    def via_error(self, T, entry):
        """(e, ge) of one via-point on the trajectory T: r_v = ‖e‖."""
        m, cart, target = entry
        target = np.asarray(target, np.float32).astype(np.float64)
        if cart:
            e, Jee = self.ee_error(T[m], TaskGoal(target[:2]))
            return e, Jee.T @ e
        e = T[m] - target
        return e, e

    def via_dist(self, alpha):
        T, _ = self.traj_vel(alpha)
        return np.array([np.linalg.norm(self.via_error(T, v)[0]) for v in self.via])

    def cost_tv(self, T, V, obs, s, g, lsg, ljl, lmax):
        c = super().cost_tv(T, V, obs, s, g, lsg, ljl, lmax)
        for v in self.via:
            e, _ = self.via_error(T, v)
            c = c + lsg * 0.5 * float(e @ e)
        return c

    def grad_ab(self, T, V, obs, s, g, lsg, ljl, lmax):
        a, b = super().grad_ab(T, V, obs, s, g, lsg, ljl, lmax)
        for v in self.via:
            _, ge = self.via_error(T, v)
            a[v[0]] += lsg * ge
        return a, b

    def constraints(self, alpha, s, g):
        ok, rep = super().constraints(alpha, s, g)
        for r in self.via_dist(alpha):
            ok = ok and bool(r < self.p.eps_position)
        return ok, rep


def restatement(*argv, whole_robot=False, via=(), **overrides):
    """(ViaRef64, CPU oracle) of a configuration: the oracle's fp32 t, K, dK, J are the library's."""
    R, o = tc.restatement(*argv, whole_robot=whole_robot, **overrides)
    return ViaRef64(o.params, R.t.astype(np.float32), R.K, R.dK, R.J, whole_robot=whole_robot, via=via), o


def entries(rows, cartesian, targets):
    """The via list of one problem from rows, kinds and its V×D targets."""
    return [(int(m), int(c), np.asarray(t, np.float32)) for m, c, t in zip(rows, cartesian, targets)]


# ------------------------------------------------------------------------------------------- mutants
class RowShift(ViaRef64):
    """The via term on row m_v + shift."""

    def __init__(self, *a, shift=1, **kw):
        super().__init__(*a, **kw)
        self.via = [(m + shift, c, t) for m, c, t in self.via]


class WithVelocity(ViaRef64):
    """A velocity term ½·λsg·‖V[m_v]‖² added on the via row, as rows 0 and N−1 have."""

    def cost_tv(self, T, V, obs, s, g, lsg, ljl, lmax):
        return super().cost_tv(T, V, obs, s, g, lsg, ljl, lmax) + sum(lsg * 0.5 * float(V[m] @ V[m]) for m, _, _ in self.via)

    def grad_ab(self, T, V, obs, s, g, lsg, ljl, lmax):
        a, b = super().grad_ab(T, V, obs, s, g, lsg, ljl, lmax)
        for m, _, _ in self.via:
            b[m] += lsg * V[m]
        return a, b


class CartAsJoint(ViaRef64):
    """A Cartesian via-point read as a joint one."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.via = [(m, 0, t) for m, c, t in self.via]


def mutants(R):
    """name -> mutant restatement of R (same operators, same via list)."""
    args = (R.p, R.t.astype(np.float32), R.K, R.dK, R.J)
    kw = dict(whole_robot=R.whole_robot, via=R.via)
    out = {"dropped": ViaRef64(*args, whole_robot=R.whole_robot, via=()), "velocity": WithVelocity(*args, **kw)}
    if all(m + 1 <= R.N - 1 for m, _, _ in R.via):
        out["row+1"] = RowShift(*args, shift=1, **kw)
    if all(m - 1 >= 0 for m, _, _ in R.via):
        out["row-1"] = RowShift(*args, shift=-1, **kw)
    if any(c for _, c, _ in R.via):
        out["cart-as-joint"] = CartAsJoint(*args, **kw)
    return out


# ------------------------------------------------------------------------------------------- the seed recipe
def via_path(t, rows, knots, dtype=np.float32):
    """Piecewise-linear path (N×D) through the knot configurations at the support rows (0 … N−1), linear in the
    support times — the recipe of Context.via_seed for one problem."""
    t = np.asarray(t, dtype)
    knots = [np.asarray(k, dtype) for k in knots]
    path = np.zeros((t.shape[0], knots[0].shape[0]), dtype)
    for (r0, a), (r1, b) in zip(zip(rows, knots), zip(rows[1:], knots[1:])):
        w = ((t[r0:r1 + 1] - t[r0]) / (t[r1] - t[r0])).astype(dtype)
        path[r0:r1 + 1] = a[None] + w[:, None] * (b - a)[None]
    return path


def seed_knots(o, start, goal, via, goal_xy=None):
    """(rows, knots) of the seed of one problem: start, each via-point in row order (a Cartesian one through the
    numpy recipe of irm_ik_seed started at the previous knot), and the goal (chained IK with goal_xy)."""
    D = int(o.params.n_joints)
    links = [float(o.params.link_length[i]) for i in range(D)]
    lo, hi = tc.safety_range(o.params)
    knots, rows = [np.asarray(start, np.float32)], [0]
    for m, c, target in via:
        q = tc.ik_seed(links, knots[-1], np.asarray(target, np.float32)[:2], lo, hi)[0] if c else np.asarray(target, np.float32)
        knots.append(np.asarray(q, np.float32))
        rows.append(int(m))
    if goal_xy is not None:
        knots.append(np.asarray(tc.ik_seed(links, knots[-1], np.asarray(goal_xy, np.float32), lo, hi)[0], np.float32))
    else:
        knots.append(np.asarray(goal, np.float32))
    rows.append(int(o.N) - 1)
    return rows, knots


def ridge_fit64(R, path, ridge=1e-6):
    """α = (K + ρI)⁻¹·path·J⁻¹ in fp64: the fit of irm_fit_alpha restated."""
    K = np.asarray(R.K, np.float64)
    return np.linalg.solve(K + ridge * np.eye(K.shape[0]), np.asarray(path, np.float64)) @ np.linalg.inv(np.asarray(R.J, np.float64))


# ------------------------------------------------------------------------------------------- scenes
# the end-to-end scenes (BLS, default hyper-parameters, the reference arm and its obstacles, start 0): name ->
# (row fractions (numerator, denominator) of N, end-effector targets)
E2E_START = np.zeros(3, np.float32)
E2E_GOAL = np.array([1.2, 0.8, 0.3], np.float32)
E2E_SCENES = {
    "mid-a": (((1, 2),), np.array([[2.4, 1.2]], np.float32)),
    "mid-b": (((1, 2),), np.array([[1.0, 2.2]], np.float32)),
    "pair": (((1, 3), (2, 3)), np.array([[2.6, 1.0], [1.0, 2.2]], np.float32)),
}
E2E_N = (33, 50)
E2E_JOINT = np.array([0.2, 1.0, -0.3], np.float32)  # the joint via-point of the end-to-end test, at row N//2


def e2e_via(name, N):
    """(rows, cartesian, targets V×3) of an end-to-end scene on N support rows."""
    fr, xy = E2E_SCENES[name]
    rows = [(a * N) // b for a, b in fr]
    tg = np.zeros((len(rows), 3), np.float32)
    tg[:, :2] = xy
    return rows, [1] * len(rows), tg


def near_targets(R, alpha, rows, cartesian, seed=0, lo=0.1, hi=0.3):
    """Targets (V×D fp32) that sit between lo and hi from where row m of α's trajectory actually is — from its
    configuration for a joint via-point (a random direction in joint space), from its end effector for a
    Cartesian one (the rest of the row is filled with a value the library must ignore)."""
    rng = np.random.default_rng(6000 + seed)
    T, _ = R.traj_vel(alpha)
    out = np.zeros((len(rows), R.D), np.float32)
    for i, (m, c) in enumerate(zip(rows, cartesian)):
        r = rng.uniform(lo + 0.02, hi - 0.02)
        if c:
            x, y, _, _ = R._fk(T[m][None])
            phi = rng.uniform(0, 2 * np.pi)
            out[i, :2] = [x[0] + r * np.cos(phi), y[0] + r * np.sin(phi)]
            out[i, 2:] = 77.0
        else:
            d = rng.standard_normal(R.D)
            out[i] = T[m] + r * d / np.linalg.norm(d)
    return out


@functools.lru_cache(maxsize=None)
def forward_restatement(N, D, whole=False):
    return restatement(*mc.shape_argv(N, D), whole_robot=bool(whole))
