"""Clearance of the arm's links against disc obstacles (irm_clearance): the scenes, the fp64 restatement that the
GPU suite measures the kernel against, a brute-force check of that restatement, and the error bound derived from
the arithmetic include/irm.h states.  Shared by tests/test_clearance_host.py (CPU) and tests/test_gpu_clearance.py.

The reference has no counterpart of this feature, so the yardstick is the restatement below; it is itself checked
against brute force (every link sampled at 2001 points) before anything is compared with it."""
import numpy as np

from physics_cases import ULP_BOUND

LINKS3 = (1.5, 1.0, 0.5)
# obstacles inside the workspace: the closest approach is on an inner link, not at the tip
NEAR = np.array([(0.8, 0.5), (1.9, 0.9), (-0.4, 0.9), (2.4, -0.6)], np.float32)
SEED = 1
B = 16


def reference_scene():
    """The reference's own 11 obstacles, on the rim of the workspace."""
    from irm_motion_planning_amd.environment import OBSTACLES
    return OBSTACLES[:11].astype(np.float32)


def links(D):
    """The link lengths of the D-joint arm of the tests (reach 3; test_gpu_dense.shape_argv's)."""
    return LINKS3 if D == 3 else (3.0 / D,) * D


def problems(D=3, batch=B, seed=SEED):
    """Starts and goals drawn as the benchmark's C3 batch draws them: U(−0.5, 0.5)^D, U(0.2, 1.6)^D."""
    rs = np.random.default_rng(seed)
    start = rs.uniform(-0.5, 0.5, (batch, D)).astype(np.float32)
    goal = rs.uniform(0.2, 1.6, (batch, D)).astype(np.float32)
    return start, goal


def straight_lines(N=64, D=3):
    """The straight-line plans between problems(): B×N×D joint positions (init_alpha's shape)."""
    start, goal = problems(D)
    t = np.linspace(0.0, 1.0, N)
    return start[:, None, :].astype(np.float64) + (goal - start)[:, None, :].astype(np.float64) * t[None, :, None]


# ------------------------------------------------------------------------------------------ fp64 restatement
def fk64(q, link):
    """Joint positions (… × D × 2) in fp64: prefix sums of the angles, then of L·(cos, sin)."""
    c = np.cumsum(np.asarray(q, np.float64), axis=-1)
    ll = np.asarray(link, np.float64)
    return np.stack((np.cumsum(ll * np.cos(c), -1), np.cumsum(ll * np.sin(c), -1)), axis=-1)


def moved(obs, vel, t):
    """The obstacle table of every time t (M): M×O×2, fmaf(t, w, p) in fp64 (static: the table itself)."""
    obs = np.asarray(obs, np.float64)
    t = np.asarray(t, np.float64)
    if vel is None:
        return np.broadcast_to(obs, t.shape + obs.shape)
    return obs[None] + t[:, None, None] * np.asarray(vel, np.float64)[None]


def clearance64(q, link, obs_t, radius=None, link_radius=0.0):
    """The definition in fp64.  q: M×D positions; obs_t: M×O×2 (moved); radius: O or None.
    g (M×D×O): the signed clearance of every (sample, link, obstacle); s (M×D×O): the clamped projection."""
    q = np.asarray(q, np.float64)
    M, D = q.shape
    obs_t = np.asarray(obs_t, np.float64)
    O = obs_t.shape[1]
    c = np.cumsum(q, axis=-1)
    ll = np.asarray(link, np.float64)
    e = np.stack((ll * np.cos(c), ll * np.sin(c)), axis=-1)  # M×D×2
    p = np.cumsum(e, axis=1)
    a = np.concatenate((np.zeros((M, 1, 2)), p[:, :-1]), axis=1)  # p_{l−1}
    u = obs_t[:, None, :, :] - a[:, :, None, :]  # M×D×O×2
    s = np.clip((u * e[:, :, None, :]).sum(-1) / (ll * ll)[None, :, None], 0.0, 1.0)
    r = u - s[..., None] * e[:, :, None, :]
    d = np.sqrt((r * r).sum(-1))
    rad = np.zeros(O) if radius is None else np.asarray(radius, np.float64)
    return (d - rad[None, None, :]) - float(link_radius), s


def lex_argmin(g):
    """(value, i, l, o) of the minimum of g (M×D×O), the lexicographically lowest index on ties; O = 0:
    (inf, −1, −1, −1)."""
    if g.size == 0:
        return np.inf, -1, -1, -1
    k = int(np.argmin(g))  # the first in C order = the lexicographically lowest (i, l, o)
    i, l, o = np.unravel_index(k, g.shape)
    return float(g[i, l, o]), int(i), int(l), int(o)


def summary64(g):
    """What the report and the optional outputs hold, from g (M×D×O) in fp64."""
    M, D, O = g.shape
    if O == 0:
        return {"clearance": np.full(M, np.inf), "link_clearance": np.full(D, np.inf), "min_clearance": np.inf,
                "argmin": (-1, -1, -1)}
    v, i, l, o = lex_argmin(g)
    return {"clearance": g.min(axis=(1, 2)), "link_clearance": g.min(axis=(0, 2)), "min_clearance": v,
            "argmin": (i, l, o)}


def brute_force(q, link, obs_t, samples=2001):
    """The distance of every (sample, link, obstacle) by sampling each link at `samples` points: M×D×O."""
    p = fk64(q, link)
    M, D = p.shape[:2]
    a = np.concatenate((np.zeros((M, 1, 2)), p[:, :-1]), axis=1)
    w = np.linspace(0.0, 1.0, samples)
    pts = a[:, :, None, :] + w[None, None, :, None] * (p - a)[:, :, None, :]  # M×D×S×2
    obs_t = np.asarray(obs_t, np.float64)
    out = np.empty((M, D, obs_t.shape[1]))
    for o in range(obs_t.shape[1]):
        diff = pts - obs_t[:, None, None, o, :]
        out[:, :, o] = np.sqrt((diff * diff).sum(-1)).min(-1)
    return out


def joints_only_min(q, link, obs_t):
    """The minimum distance from the joint positions alone (what --whole-robot-cost looks at): M."""
    p = fk64(q, link)
    diff = p[:, :, None, :] - np.asarray(obs_t, np.float64)[:, None, :, :]
    return np.sqrt((diff * diff).sum(-1)).min(axis=(1, 2))


# ------------------------------------------------------------------------------------------ the error bound
U32 = 2.0 ** -24  # half an ulp, relative: the rounding of one fp32 operation


def tolerance(link, max_angle, max_obstacle, radius_max=0.0, link_radius=0.0, moving=False):
    """A bound on |kernel − clearance64| for every (sample, link, obstacle) — hence for their minima, since
    |min a − min b| ≤ max |a − b| — from the arithmetic include/irm.h states, on the same fp32 positions q.

    max_angle: max |c_l| over the data (rad); max_obstacle: max |o| over the obstacle positions the samples see.

    Geometry (the distance to a segment is 1-Lipschitz in its end points, so the segment's error is that of its
    worse end point).  With u = 2⁻²⁴, R_l = L_0 + … + L_l:
      angle      c_l takes l fp32 additions, each within u·|c| ≤ u·A of its exact result; the kernel keeps those
                 roundings exactly (two-sum) in a tail that itself takes l additions of values ≤ l·u·A, and applies
                 it to sin / cos to first order: what is left of the angle is ≤ l²·u²·A (the tail's roundings) +
                 (l·u·A)²/2 (the dropped second order), which turns link l's direction vector by L_l times that
      sincos     each of sin, cos within ULP_BOUND ulps, an ulp at most 2⁻²³, and the correction fmaf(tail, cs, sn)
                 rounds once more (u): the direction L_l·(cs, sn) is off by at most √2·L_l·(ULP_BOUND·2⁻²³ + u)
      positions  x_l = fmaf(L_l, cs, x_{l−1}) rounds once, within u·|x_l| ≤ u·R_l: √2·u·R_l per joint
      direction  e = (L_l·cs, L_l·sn), one product each: √2·u·L_l
    so with a_k = k²·u²·A + (k·u·A)²/2 and t = √2·(ULP_BOUND·2⁻²³ + u), p_{l−1} is off by
    E_{l−1} = Σ_{k<l} (L_k·(a_k + t) + √2·u·R_k) and the far end point p_{l−1} + e by E_{l−1} + L_l·(a_l + t + √2·u);
    the largest over the links counts.
    A moving obstacle adds its own rounding, fmaf(t, w, p) within u·|coordinate|: √2·u·|o|.

    Arithmetic of the distance from there, with U = |o − p_{l−1}| ≤ |o| + R the length of u and d ≤ U:
      u = o − p        √2·u·U
      s                the dot product's two roundings, 1/(L·L) (two roundings) and the product: |δs| ≤
                       (2√2·u·U·L)/L² + 3u·s, and a point δs·L off the nearest one is at most that much farther:
                       ≤ 2√2·u·U + 3u·L
      r = u − s·e      one fused rounding per coordinate: √2·u·d
      d                r·r (two roundings, u relative on d after the root) and the root (u): 2u·d
      g                two subtractions: u·(|d − radius| + |g|) ≤ 2u·(d + radius + link_radius)
    in total ≤ u·((3√2 + √2 + 2 + 2)·U + 3·L_max + 2·(radius + link_radius))."""
    L = np.asarray(link, np.float64)
    R = np.cumsum(L)
    r2 = np.sqrt(2.0)
    sc = r2 * (ULP_BOUND * 2.0 ** -23 + U32)
    E, worst = 0.0, 0.0
    for l in range(len(L)):
        angle = l * l * U32 * U32 * max_angle + 0.5 * (l * U32 * max_angle) ** 2
        worst = max(worst, E + L[l] * (angle + sc + r2 * U32))
        E += L[l] * (angle + sc) + r2 * U32 * R[l]
    geometry = worst + (r2 * U32 * max_obstacle if moving else 0.0)
    U = max_obstacle + R[-1]
    arithmetic = U32 * ((4.0 * r2 + 4.0) * U + 3.0 * L.max() + 2.0 * (radius_max + link_radius))
    return geometry + arithmetic


def max_angle(q):
    return float(np.abs(np.cumsum(np.asarray(q, np.float64), axis=-1)).max())


# ------------------------------------------------------------------------------------------ what the scenes show
def _check_scenes():
    """The two properties the scenes were chosen for, on the straight-line plans at N = 64 (checked at import: a
    changed seed that breaks them is the wrong seed)."""
    T = straight_lines()
    t = np.linspace(0.0, 1.0, T.shape[1])
    for b in range(B):
        g, s = clearance64(T[b], LINKS3, moved(NEAR, None, t))
        _, i, l, o = lex_argmin(g)
        assert l < len(LINKS3) - 1 and 0.0 < s[i, l, o] < 1.0, ("NEAR", b, i, l, o, s[i, l, o])
        ref_t = moved(reference_scene(), None, t)
        g, _ = clearance64(T[b], LINKS3, ref_t)
        # (equal up to fp64 rounding: (o − p_{l−1}) − e against o − (p_{l−1} + e))
        assert abs(g.min() - joints_only_min(T[b], LINKS3, ref_t).min()) <= 1e-12, ("reference scene", b)


_check_scenes()
