"""Clearance of the arm's links against each other (irm_self_clearance): the scenes, the fp64 restatement that the GPU
suite measures the kernel against, a brute-force check of that restatement, and the error bound derived from the
arithmetic include/irm.h states.  Shared by tests/test_self_clearance_host.py (CPU) and
tests/test_gpu_self_clearance.py, in the manner of tests/clearance_cases.py.

The reference has no counterpart of this feature, so the yardstick is the restatement below; it is itself checked
against brute force (both links of a pair sampled at 401 points each) before anything is compared with it."""
import numpy as np

from clearance_cases import LINKS3, U32, fk64, max_angle  # noqa: F401  (max_angle: re-exported for the tests)
from physics_cases import ULP_BOUND

LINKS7 = (3.0 / 7.0,) * 7  # the arm of the C5 / C7 shapes
SEED = 5  # (of 1 … 5 the seed whose fold3 and lim3 batches keep every problem clear of a flag change: _check_scenes)
B = 16
BRUTE_SAMPLES = 401

# name -> (links, q_end): the joint-space line q(t) = t·q_end from 0
SCENES = {
    "fold3": (LINKS3, (0.0, 2.9, 1.6)),  # a planned sweep that crosses link 2 over link 0
    "curl7": (LINKS7, (1.1,) * 7),  # the 7-link arm curling up through itself
    "curl7lim": (LINKS7, (0.95,) * 7),  # the same inside the default joint limits [−1, 2]
    "lim3": (LINKS3, (0.3, 2.0, 2.0)),  # inside the limits: no crossing, link 2 comes within 0.531 of link 0
}
# what the exact lines show in fp64 — (scene, M): (crossing samples, the first, the pairs that cross)
EXPECTED = {
    ("fold3", 64): (5, 59, {(0, 2)}),
    ("fold3", 65): (5, 60, {(0, 2)}),
    ("curl7", 64): (12, 52, {(0, 5), (0, 6), (1, 6)}),
    ("curl7", 65): (12, 53, {(0, 5), (0, 6), (1, 6)}),
    ("curl7lim", 64): (4, 60, {(0, 6)}),
    ("lim3", 64): (0, -1, set()),
    ("lim3", 65): (0, -1, set()),
}
LIM3_MIN_DISTANCE = 0.531  # of lim3's end configuration: link_radius 0.3 collides, 0.2 does not


def pairs(D):
    """The link pairs (a, b), a + 2 ≤ b, in the order of pair_out: (0,2), (0,3), …, (D−3, D−1)."""
    return [(a, b) for a in range(D) for b in range(a + 2, D)]


def line(scene, M, q_end=None):
    """The scene's joint-space line on linspace(0, 1, M): M×D positions in fp64 (q_end: another end point)."""
    link, end = SCENES[scene]
    end = np.asarray(end if q_end is None else q_end, np.float64)
    return np.linspace(0.0, 1.0, M)[:, None] * end[None, :]


def batch_ends(scene, batch=B, seed=SEED):
    """The end points of a batch of the scene's lines: problem 0 the scene's own, the others within ±5 % of it per
    joint (seeded)."""
    end = np.asarray(SCENES[scene][1], np.float64)
    rs = np.random.default_rng(seed)
    ends = end[None, :] * (1.0 + rs.uniform(-0.05, 0.05, (batch, len(end))))
    ends[0] = end
    return ends


# ------------------------------------------------------------------------------------------ fp64 restatement
def _dist_orient(x, A, e, w):
    """dist(x; A, e, w) and orient(x; A, e) of include/irm.h in fp64, over leading axes."""
    u = x - A
    s = np.clip((u * e).sum(-1) * w, 0.0, 1.0)
    r = u - s[..., None] * e
    return np.sqrt((r * r).sum(-1)), u[..., 0] * e[..., 1] - u[..., 1] * e[..., 0]


def self_clearance64(q, link, link_radius=0.0):
    """The definition in fp64.  q: M×D positions.  Returns (g, crossing, margin), each M×P in the pair order: the
    signed clearance, the crossing flag and the crossing margin min |o_k| over the four orientations (how far the
    flag is from changing where the pair crosses)."""
    q = np.asarray(q, np.float64)
    M, D = q.shape
    ll = np.asarray(link, np.float64)
    c = np.cumsum(q, axis=-1)
    e = np.stack((ll * np.cos(c), ll * np.sin(c)), axis=-1)  # M×D×2
    p = np.cumsum(e, axis=1)
    start = np.concatenate((np.zeros((M, 1, 2)), p[:, :-1]), axis=1)  # p_{l−1}
    w = 1.0 / (ll * ll)
    P = pairs(D)
    g, crossing, margin = (np.empty((M, len(P))) for _ in range(3))
    for k, (a, b) in enumerate(P):
        d1, o1 = _dist_orient(start[:, b], start[:, a], e[:, a], w[a])
        d2, o2 = _dist_orient(p[:, b], start[:, a], e[:, a], w[a])
        d3, o3 = _dist_orient(start[:, a], start[:, b], e[:, b], w[b])
        d4, o4 = _dist_orient(p[:, a], start[:, b], e[:, b], w[b])
        opposite = lambda x, y: ((x > 0) & (y < 0)) | ((x < 0) & (y > 0))  # noqa: E731  (a zero is not a sign)
        x = opposite(o1, o2) & opposite(o3, o4)
        d = np.where(x, 0.0, np.minimum(np.minimum(d1, d2), np.minimum(d3, d4)))
        g[:, k] = d - 2.0 * float(link_radius)
        crossing[:, k] = x
        margin[:, k] = np.minimum(np.minimum(np.abs(o1), np.abs(o2)), np.minimum(np.abs(o3), np.abs(o4)))
    return g, crossing.astype(bool), margin


def summary64(g, crossing, D):
    """What the report and the optional outputs hold, from g and crossing (M×P) in fp64."""
    M, P = g.shape
    if P == 0:
        return {"clearance": np.full(M, np.inf), "pair_clearance": np.zeros(0), "min_clearance": np.inf,
                "argmin": (-1, -1, -1), "n_colliding": 0, "first_colliding": -1, "n_crossing": 0, "collision_free": True}
    k = int(np.argmin(g))  # the first in C order = the lexicographically lowest (i, a, b)
    i, j = np.unravel_index(k, g.shape)
    a, b = pairs(D)[j]
    coll = (crossing | (g < 0.0)).any(axis=1)
    hits = np.flatnonzero(coll)
    return {"clearance": g.min(axis=1), "pair_clearance": g.min(axis=0), "min_clearance": float(g[i, j]),
            "argmin": (int(i), a, b), "n_colliding": int(coll.sum()),
            "first_colliding": int(hits[0]) if hits.size else -1, "n_crossing": int(crossing.any(axis=1).sum()),
            "collision_free": not coll.any()}


def brute_force(q, link, samples=BRUTE_SAMPLES):
    """The distance of every (sample, pair) by sampling both links at `samples` points each: M×P."""
    p = fk64(q, link)
    M, D = p.shape[:2]
    start = np.concatenate((np.zeros((M, 1, 2)), p[:, :-1]), axis=1)
    w = np.linspace(0.0, 1.0, samples)
    pts = start[:, :, None, :] + w[None, None, :, None] * (p - start)[:, :, None, :]  # M×D×S×2
    P = pairs(D)
    out = np.empty((M, len(P)))
    for k, (a, b) in enumerate(P):
        diff = pts[:, a, :, None, :] - pts[:, b, None, :, :]  # M×S×S×2
        out[:, k] = np.sqrt((diff * diff).sum(-1)).min(axis=(1, 2))
    return out


def brute_spacing(link, samples=BRUTE_SAMPLES):
    """How far the nearest pair of brute-force samples can lie from the nearest pair of points, per pair (P): half a
    spacing on either link."""
    ll = np.asarray(link, np.float64)
    return np.array([(ll[a] + ll[b]) / (2.0 * (samples - 1)) for a, b in pairs(len(ll))])


# ------------------------------------------------------------------------------------------ the error bound
def geometry_error(link, max_angle):
    """E of clearance_cases.tolerance (its docstring derives it): how far a segment of the kernel's arm lies from the
    exact one on the same fp32 positions q — the worse of its two end points, the largest over the links."""
    L = np.asarray(link, np.float64)
    R = np.cumsum(L)
    r2 = np.sqrt(2.0)
    sc = r2 * (ULP_BOUND * 2.0 ** -23 + U32)
    E, worst = 0.0, 0.0
    for l in range(len(L)):
        angle = l * l * U32 * U32 * max_angle + 0.5 * (l * U32 * max_angle) ** 2
        worst = max(worst, E + L[l] * (angle + sc + r2 * U32))
        E += L[l] * (angle + sc) + r2 * U32 * R[l]
    return worst


def tolerance(link, max_angle, link_radius=0.0):
    """A bound on |kernel − self_clearance64| for every (sample, pair) — hence for their minima, since
    |min a − min b| ≤ max |a − b| — from the arithmetic include/irm.h states, on the same fp32 positions q.
    max_angle: max |c_l| over the data (rad).  With u = 2⁻²⁴ and R the arm's reach, three terms:

    Geometry.  Each of the two links is a segment of the kernel's arm, off the exact one by at most E =
    geometry_error(link, max_angle) (clearance_cases.tolerance's geometry term: angle sum, sincos, the fmaf
    accumulation of the joints, the direction's product).  The distance between two sets is 1-Lipschitz in each of
    them, so both links count: 2·E.

    Arithmetic of dist, clearance_cases.tolerance's arithmetic term with the measured point now a joint of the arm:
    |u| = |x − A| ≤ U = 2·R, and one subtraction d − 2·link_radius (2·link_radius is exact) in place of two:
        u·((3√2 + √2 + 2 + 2)·U + 3·L_max + 2·(2·link_radius)).
    The minimum of the four distances is exact.

    Orientation.  The two terms above bound the error of the distance of the kernel's own segments, which is 0 where
    they cross; what is left is the kernel's fp32 sign test disagreeing with the exact sign test on those same
    segments.  d is continuous across the crossing boundary (it falls to 0 as an end point reaches the other link)
    but the flag is not.  Where the two tests disagree, an end point's orientation o lies within the rounding error
    δo of its computed value from changing sign, so that end point is within |δo| / L of the line of the other link
    (L that link's length, at least L_min) and both values are within that of 0.  δo comes from the three roundings
    of orient = fmaf(u_x, e_y, −(u_y·e_x)): u = x − A (√2·u·U over the two coordinates, times |e| = L), the product
    (u·U·L) and the fused sum (u·U·L), so L cancels:
        |δo| / L ≤ (√2 + 2)·u·U.
    (Links that are collinear to 1e-7 and apart are the one case where the flags can disagree away from d = 0; the
    scenes meet it only at t = 0 with the arm along the x axis, where the y coordinates are tiny and carry relative,
    not absolute, errors.)"""
    L = np.asarray(link, np.float64)
    R = float(L.sum())
    r2 = np.sqrt(2.0)
    E = geometry_error(link, max_angle)
    U = 2.0 * R
    arithmetic = U32 * ((4.0 * r2 + 4.0) * U + 3.0 * L.max() + 4.0 * link_radius)
    orientation = (r2 + 2.0) * U32 * U
    return 2.0 * E + arithmetic + orientation


def cap_holds(g, crossing, margin, tol):
    """The cap of the count / flag / argmin assertions: they exclude no sample, so every crossing pair's margin and
    every other pair's |g| must be 16 tolerances away from changing the answer (a crossing pair's g is −2·link_radius
    exactly, on both sides)."""
    return bool(np.all(margin[crossing] > 16.0 * tol)) and bool(np.all(np.abs(g[~crossing]) > 16.0 * tol))


# ------------------------------------------------------------------------------------------ what the scenes show
def _check_scenes():
    """The properties the scenes were chosen for, on the exact lines in fp64 (checked at import: a changed scene that
    breaks them is the wrong scene)."""
    for (name, M), (count, first, which) in EXPECTED.items():
        link = SCENES[name][0]
        g, x, margin = self_clearance64(line(name, M), link)
        s = summary64(g, x, len(link))
        crossed = {pairs(len(link))[k] for k in np.flatnonzero(x.any(axis=0))}
        assert (s["n_crossing"], s["first_colliding"], crossed) == (count, first, which), (name, M, s, crossed)
        assert s["n_colliding"] == s["n_crossing"]  # link_radius 0: a collision is exactly a crossing
        tol = tolerance(link, max_angle(line(name, M)))
        assert cap_holds(g, x, margin, tol), (name, M, float(margin[x].min()) if x.any() else None,
                                                     float(np.abs(g[~x]).min()))
    for name in ("fold3", "lim3"):  # the batches whose counts and flags the GPU suite asserts problem by problem
        link = SCENES[name][0]
        for M in (64, 65):
            for end in batch_ends(name):
                q = line(name, M, end)
                g, x, margin = self_clearance64(q, link)
                assert cap_holds(g, x, margin, 4.0 * tolerance(link, max_angle(q))), (name, M, end)
    link, end = SCENES["lim3"]
    g, x, _ = self_clearance64(np.asarray(end)[None, :], link)
    assert not x.any() and abs(g.min() - LIM3_MIN_DISTANCE) < 5e-4, float(g.min())
    for radius, hit in ((0.2, False), (0.3, True)):
        g, x, _ = self_clearance64(np.asarray(end)[None, :], link, link_radius=radius)
        assert bool((g < 0).any()) == hit, (radius, float(g.min()))


_check_scenes()
