"""The numpy twin of multi-start planning (include/irm.h, "Multi-start planning"): the hash and the amplitudes, the
c / φ tables, the waypoint formula, the ranking by (class, loss, s) as a lexsort and as brute force, the replicate
gather, and the nine scenes of the motivation study.

Everything here is the header's arithmetic operation for operation in fp32 (numpy float32 arrays round after every
operation; the fused multiply-adds are formed exactly, see fmaf32), so the device must agree with it to the bit.
tests/test_multistart_host.py checks the twin itself (against hand-computed hashes and a brute-force sort)."""
import numpy as np

f32 = np.float32
MAX_SEEDS = 64
HASH_SALT = 0x243F6A88


# ------------------------------------------------------------------ the hash and the amplitudes
def fmix32(h):
    """MurmurHash3's finaliser on uint32 (arrays or scalars), wrapping arithmetic."""
    h = np.asarray(h, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def _add32(a, b):
    return ((np.asarray(a, np.uint64) + np.asarray(b, np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def seed_hash(seed, problem, s, d):
    """h = fmix32(fmix32(fmix32(fmix32(seed ^ salt) + problem) + s) + d), broadcasting over problem / s / d."""
    h0 = fmix32(np.uint32((int(seed) ^ HASH_SALT) & 0xFFFFFFFF))
    return fmix32(_add32(fmix32(_add32(fmix32(_add32(h0, problem)), s)), d))


def fmaf32(a, b, c):
    """fmaf(a, b, c) of float32 values, correctly rounded: the product of two float32 is exact in float64; the sum
    with c is formed in float64 with its rounding error (two-sum), moved to the odd neighbour when inexact
    (round-to-odd keeps the sticky bit), and then rounded to float32 once — 53 ≥ 2·24 + 2 bits make that the
    correctly rounded result."""
    a, b, c = (np.asarray(x, f32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # exactly (p + c) − s
    s, err = np.broadcast_arrays(s, err)
    s = s.copy()
    inexact = (err != 0) & np.isfinite(s)
    even = (s.view(np.int64) & 1) == 0
    fix = inexact & even
    toward = np.where(err > 0, np.inf, -np.inf)
    s[fix] = np.nextafter(s[fix], toward[fix])
    return s.astype(f32)


def amplitudes(seed, B, S, D, A, problem_offset=0):
    """a (B, S, D) float32: a = fmaf(2A, U, −A), U = (h >> 8)·2⁻²⁴."""
    b = (np.arange(B, dtype=np.uint64) + np.uint64(problem_offset))[:, None, None]
    s = np.arange(S, dtype=np.uint64)[None, :, None]
    d = np.arange(D, dtype=np.uint64)[None, None, :]
    h = seed_hash(seed, b, s, d)
    u = (h >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)  # 24 bits: exact
    A = f32(A)
    return fmaf32(f32(2) * A, u, -A)


# ------------------------------------------------------------------ the tables and the waypoints
def support_times(N):
    """t = linspace(0, 1, N) as the operator build forms it in fp32."""
    t = np.arange(N, dtype=f32) / f32(N - 1)
    t[N - 1] = f32(1)
    return t


def smooth_step(t):
    """c = 6t⁵ − 15t⁴ + 10t³ in the operator build's fp32 order."""
    t = np.asarray(t, f32)
    t3 = t * t * t
    t4 = t3 * t
    t5 = t4 * t
    return f32(6) * t5 - f32(15) * t4 + f32(10) * t3


def bump(t):
    """φ = 16·(p·p), p = t·(1 − t), fp32."""
    t = np.asarray(t, f32)
    p = t * (f32(1) - t)
    return f32(16) * (p * p)


def clamp_bounds(joint_safety_limit, min_joint_position, max_joint_position):
    """(lo, hi): the fp32 roundings of the fp64 products of the fp32 parameters (irm_ik_seed's bounds)."""
    jsl = np.float64(f32(joint_safety_limit))
    return f32(jsl * np.float64(f32(min_joint_position))), f32(jsl * np.float64(f32(max_joint_position)))


def waypoints(start, goal, S, seed, A, lo, hi, t, problem_offset=0):
    """(B, S, N, D) float32: candidate 0 the plain line base = fmaf(c_n, g − s, s); candidate s ≥ 1
    clamp(fmaf(φ_n, a, base), lo, hi)."""
    start, goal = np.asarray(start, f32), np.asarray(goal, f32)
    B, D = start.shape
    c, ph = smooth_step(t), bump(t)
    base = fmaf32(c[None, :, None], (goal - start)[:, None, :], start[:, None, :])  # B×N×D
    a = amplitudes(seed, B, S, D, A, problem_offset)  # B×S×D
    q = fmaf32(ph[None, None, :, None], a[:, :, None, :], base[:, None, :, :])
    q = np.minimum(np.maximum(q, f32(lo)), f32(hi))
    q[:, 0] = base
    return q


def replicate(table, S):
    """out[(b·S + s)·w + j] = in[b·w + j]: every per-problem row S times, problem-major."""
    table = np.asarray(table)
    return np.repeat(table, S, axis=0)


# ------------------------------------------------------------------ the ranking
def keys(ok, loss, n_colliding=None):
    """(class, loss) of the ranking key per candidate: class = 2·(not ok) + (n_colliding > 0); a NaN loss is class 4
    with loss +inf."""
    ok, loss = np.asarray(ok), np.asarray(loss, f32).copy()
    cls = 2 * (ok == 0).astype(np.int64)
    if n_colliding is not None:
        cls = cls + (np.asarray(n_colliding) > 0)
    nan = np.isnan(loss)
    cls[nan] = 4
    loss[nan] = np.inf
    return cls, loss


def rank_lexsort(ok, loss, n_colliding=None):
    """(winner (B,), rank (B, S)) for (B, S) tables, by a stable lexsort on (class, loss) — ties to the lower s."""
    cls, loss = keys(ok, loss, n_colliding)
    B, S = cls.shape
    rank = np.zeros((B, S), np.int32)
    winner = np.zeros(B, np.int32)
    for b in range(B):
        order = np.lexsort((np.arange(S), loss[b], cls[b]))
        rank[b, order] = np.arange(S)
        winner[b] = order[0]
    return winner, rank


def rank_brute(ok, loss, n_colliding=None):
    """The same by counting, for every candidate, the candidates whose key is smaller."""
    cls, loss = keys(ok, loss, n_colliding)
    B, S = cls.shape
    rank = np.zeros((B, S), np.int32)
    for b in range(B):
        for i in range(S):
            n = 0
            for j in range(S):
                kj, ki = (int(cls[b, j]), float(loss[b, j]), j), (int(cls[b, i]), float(loss[b, i]), i)
                n += kj < ki
            rank[b, i] = n
    return np.argmin(rank, axis=1).astype(np.int32), rank


def random_tables(rng, B, S, kind):
    """Synthetic (ok, loss, n_colliding) tables of shape (B, S).  kind: "random", "ties" (few distinct losses),
    "nan" (NaN and ±inf losses mixed in), "allfail" (no candidate ok), "classes" (every class present)."""
    ok = rng.integers(0, 2, (B, S)).astype(np.int32)
    ncol = (rng.integers(0, 3, (B, S)) * rng.integers(0, 2, (B, S))).astype(np.int32)
    loss = rng.uniform(0.1, 50.0, (B, S)).astype(f32)
    if kind == "ties":
        loss = rng.choice(np.array([0.5, 1.0, -0.0, 0.0], f32), (B, S))
    elif kind == "nan":
        pick = rng.integers(0, 6, (B, S))
        loss[pick == 0] = np.nan
        loss[pick == 1] = np.inf
        loss[pick == 2] = -np.inf
    elif kind == "allfail":
        ok[:] = 0
    elif kind == "classes":
        for b in range(B):
            for i in range(min(S, 4)):
                ok[b, (i * 7 + b) % S] = 1 - i // 2
                ncol[b, (i * 7 + b) % S] = i % 2
    return ok, loss, ncol


# ------------------------------------------------------------------ the study's scenes
# One disc obstacle of radius STUDY_RADIUS at nine positions inside the sweep of the reference arm (links 1.5, 1, 0.5)
# moving from START to GOAL; N = 33 support times, clearance on 257 samples, S = 12 seeds of amplitude 1.2.
STUDY_N, STUDY_M, STUDY_S, STUDY_A, STUDY_SEED, STUDY_RADIUS = 33, 257, 12, 1.2, 0, 0.15
STUDY_START = np.zeros(3, f32)
STUDY_GOAL = np.array([1.2, 0.8, 0.3], f32)
STUDY_SCENES = np.array([[1.2, 0.5], [0.9, 0.9], [0.5, 1.2],
                         [2.0, 0.8], [1.6, 1.4], [1.0, 1.9],
                         [2.6, 0.9], [2.2, 1.6], [1.4, 2.3]], f32)


def study_counts(winner_ok, winner_ncol):
    """(collision-free winners, winners that are ok and collision-free) over the scenes."""
    free = np.asarray(winner_ncol) == 0
    return int(free.sum()), int((free & (np.asarray(winner_ok) != 0)).sum())
