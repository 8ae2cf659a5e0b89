"""The yardstick of the end-effector-goal tests: an fp64 restatement, the IK recipe and the scenes.

`TaskRef64` is `moving_cases.MovingRef64` with one change: where the goal `g` of `cost_tv` / `grad_ab` is a
`TaskGoal(p)`, row N−1 is held to the Cartesian target p through the end-effector FK f and its Jacobian J_ee
(include/irm.h):

    loss                 ½‖f(T[N−1]) − p‖²                in place of ½‖T[N−1] − g‖²
    gradient input a     λsg·J_ee(T[N−1])ᵀ·(f(T[N−1]) − p)  in place of λsg·(T[N−1] − g)
    constraint           ‖f(T[N−1]) − p‖ < eps_position    in place of ‖T[N−1] − g‖ < eps_position

also with whole_robot (the Jacobian stays the end effector's).  Everything else — `cost`, `cost_g`,
`gd_single`, moving tables — is inherited and takes a TaskGoal wherever it took g.  `constraints` restates
constraintsFulfilled (trajectory.py:129-137, robot.py:90-113) with the report layout of irm_constraints, and
`bls` the jitted BLS loop (optimizer_BLS.py:127-211) as `Ref64.gd_single` restates GD.

The reference has no such goal: this restatement, and bit-identity of the joint-goal calls, are what the
feature is measured against.  `ik_seed` is the damped-least-squares recipe of irm_ik_seed in numpy.
"""
import numpy as np

from conftest import oracle_for
from moving_cases import MovingRef64


class TaskGoal:
    """An end-effector target (p_x, p_y) in the place of a goal configuration."""

    def __init__(self, p):
        self.p = np.asarray(p, np.float32).astype(np.float64).reshape(2)


class TaskRef64(MovingRef64):
    def ee_error(self, q_end, goal):
        """f(q_end) − p and J_ee(q_end) (2×D) in fp64."""
        x, y, jx, jy = self._fk(np.asarray(q_end, np.float64)[None])
        return np.array([x[0] - goal.p[0], y[0] - goal.p[1]]), np.stack([jx[0], jy[0]])

    def cost_tv(self, T, V, obs, s, g, lsg, ljl, lmax):
        if not isinstance(g, TaskGoal):
            return super().cost_tv(T, V, obs, s, g, lsg, ljl, lmax)
        # (the parent's joint-goal term with g = T[N−1] is exactly 0)
        base = super().cost_tv(T, V, obs, s, T[-1].copy(), lsg, ljl, lmax)
        e, _ = self.ee_error(T[-1], g)
        return base + lsg * 0.5 * float(e @ e)

    def grad_ab(self, T, V, obs, s, g, lsg, ljl, lmax):
        if not isinstance(g, TaskGoal):
            return super().grad_ab(T, V, obs, s, g, lsg, ljl, lmax)
        a, b = super().grad_ab(T, V, obs, s, T[-1].copy(), lsg, ljl, lmax)
        e, Jee = self.ee_error(T[-1], g)
        a[-1] += lsg * (Jee.T @ e)
        return a, b

    def constraints(self, alpha, s, g):
        """(ok, report): constraintsFulfilled with irm_constraints' report layout — ‖T0 − s‖, the goal distance
        (Cartesian for a TaskGoal), ‖V0‖, ‖V_{N−1}‖, max T, min T, max|V|, then the four sub-flags."""
        p = self.p
        T, V = self.traj_vel(alpha)
        ds = float(np.linalg.norm(T[0] - np.asarray(s, np.float64)))
        if isinstance(g, TaskGoal):
            dg = float(np.linalg.norm(self.ee_error(T[-1], g)[0]))
        else:
            dg = float(np.linalg.norm(T[-1] - np.asarray(g, np.float64)))
        vs, vg = float(np.linalg.norm(V[0])), float(np.linalg.norm(V[-1]))
        f0 = ds < p.eps_position and dg < p.eps_position
        f1 = vs < p.eps_velocity and vg < p.eps_velocity
        f2 = T.max() <= p.max_joint_position and T.min() >= p.min_joint_position
        f3 = np.abs(V).max() <= p.max_joint_velocity
        rep = np.array([ds, dg, vs, vg, T.max(), T.min(), np.abs(V).max(), f0, f1, f2, f3], np.float64)
        return bool(f0 and f1 and f2 and f3), rep

    def bls(self, alpha0, obs, s, g):
        """optimizer_BLS.py:127-211 in fp64.  Returns (alpha, ok, outer iterations run, inner iterations)."""
        p = self.p
        lsg, ljl, lmax = p.lambda_sg_constraint, p.lambda_jl_constraint, p.lambda_max_cost
        alpha = np.asarray(alpha0, np.float64).copy()
        ok, outers, inners = False, 0, 0
        for _ in range(int(p.max_outer_iteration)):
            lr = p.bls_lr_start
            for _ in range(int(p.max_inner_iteration)):
                loss = self.cost(alpha, obs, s, g, lsg, ljl, lmax)
                G = self.cost_g(alpha, obs, s, g, lsg, ljl, lmax)
                n = G / np.linalg.norm(G)
                anorm = np.sum(G.T @ n)
                new_loss = loss
                for _ in range(int(p.max_bls_iteration)):
                    na = (1 - p.lambda_reg * lr) * alpha - lr * n
                    nl = self.cost(na, obs, s, g, lsg, ljl, lmax)
                    if nl > loss - p.bls_alpha * lr * anorm:
                        lr *= p.bls_beta_minus
                    else:
                        alpha, new_loss = na, nl
                        lr *= p.bls_beta_plus
                        break
                if loss - new_loss < p.loop_loss_reduction:
                    break
                inners += 1
            outers += 1
            ok, _ = self.constraints(alpha, s, g)
            if ok:
                break
            lsg *= p.lambda_constraint_increase
            ljl *= p.lambda_constraint_increase
        return alpha, ok, outers, inners


def restatement(*argv, whole_robot=False, **overrides):
    """(TaskRef64, CPU oracle) of a configuration: the oracle's fp32 t, K, dK, J are the library's."""
    if whole_robot:
        overrides["whole_robot_cost"] = 1
    o = oracle_for(*argv, **overrides)
    t, K, dK, J = o.kernel_matrices()
    return TaskRef64(o.params, t, K, dK, J, whole_robot=whole_robot), o


def fk64(links, q):
    """End-effector position of configurations q (…×D) in fp64 — independent of the restatement."""
    c = np.cumsum(np.asarray(q, np.float64), axis=-1)
    L = np.asarray(links, np.float64)
    return np.stack([(L * np.cos(c)).sum(-1), (L * np.sin(c)).sum(-1)], axis=-1)


def ik_seed(links, start, goal_xy, lo, hi, dtype=np.float32, iters=32, mu=0.1, step=0.5):
    """The recipe of irm_ik_seed for one problem in numpy (`dtype` arithmetic): `iters` damped-least-squares
    steps from `start`, each scaled to max|dq| ≤ step and clamped to [lo, hi].  Returns (q, residual, the
    residual before every iteration)."""
    f = dtype
    L = np.asarray(links, f)
    q = np.asarray(start, f).copy()
    p = np.asarray(goal_xy, f)
    lo, hi, mu2 = f(lo), f(hi), f(mu) * f(mu)

    def err(q):
        c = np.cumsum(q, dtype=f)
        sx, cy = -(L * np.sin(c)).astype(f), (L * np.cos(c)).astype(f)
        e = np.array([cy.sum(dtype=f) - p[0], -sx.sum(dtype=f) - p[1]], f)
        jx = (sx + sx.sum(dtype=f) - np.cumsum(sx, dtype=f)).astype(f)
        jy = (cy + cy.sum(dtype=f) - np.cumsum(cy, dtype=f)).astype(f)
        return e, jx, jy

    hist = []
    for _ in range(iters):
        e, jx, jy = err(q)
        hist.append(float(np.hypot(e[0], e[1])))
        a11, a12, a22 = f(jx @ jx) + mu2, f(jx @ jy), f(jy @ jy) + mu2
        det = f(a11 * a22 - a12 * a12)
        y0 = f((a22 * e[0] - a12 * e[1]) / det)
        y1 = f((a11 * e[1] - a12 * e[0]) / det)
        dq = (-(jx * y0 + jy * y1)).astype(f)
        m = np.abs(dq).max()
        if m > f(step):
            dq = (dq * (f(step) / m)).astype(f)
        q = np.clip((q + dq).astype(f), lo, hi)
    e, _, _ = err(q)
    return q, float(np.hypot(e[0], e[1])), hist


# ----------------------------------------------------------------------------------------------- scenes
# the end-to-end scene (BLS, default hyper-parameters, the reference arm and obstacles, start 0): targets the
# fp64 BLS restatement reaches from the IK seed and from three perturbed seeds, at N = 33 and N = 50
E2E_TARGETS = np.array([[1.348, 2.538], [1.983, 2.145]], np.float32)
E2E_N = (33, 50)
# every target the IK tests use for the reference arm from start 0
IK_TARGETS3 = np.array([[1.348, 2.538], [1.983, 2.145], [-0.206, 2.680], [2.5, -0.5]], np.float32)


def ik_problems7(n=16, seed=0):
    """7-DoF IK problems: targets = FK of configurations U(0, 0.5)⁷, starts U(−0.5, 0.5)⁷ (links LINKS7)."""
    from moving_cases import LINKS7
    rng = np.random.default_rng(4000 + seed)
    qg = rng.uniform(0.0, 0.5, (n, 7))
    start = rng.uniform(-0.5, 0.5, (n, 7)).astype(np.float32)
    return start, fk64(LINKS7, qg).astype(np.float32)


def safety_range(p):
    """[lo, hi] the IK seed stays in: joint_safety_limit·min/max joint position, in fp32 as the library forms it."""
    return (np.float32(float(p.joint_safety_limit) * float(p.min_joint_position)),
            np.float32(float(p.joint_safety_limit) * float(p.max_joint_position)))


def out_of_reach(links):
    """(start, target) of an IK problem whose target lies one unit beyond the reach, ‖p‖ = Σ links + 1, on the
    axis of the stretched start 0: sin 0 = 0 exactly, so J_eeᵀ·e is exactly 0, the seed stays and the residual
    is the missing length 1.  (A start that is only nearly aligned does not stay: see test_task_host.py.)"""
    r = float(np.sum(np.asarray(links, np.float64))) + 1.0
    return np.zeros(len(links), np.float32), np.array([r, 0.0], np.float32)
