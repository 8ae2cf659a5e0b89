"""Inputs, references and the fixture writer of the per-waypoint physics tests (tests/test_physics_host.py on
the CPU, tests/test_gpu_physics.py on the device): sincos_poly / sincos_fast, the FK / Jacobian recurrences and
the obstacle potential of irm_physics.hpp, away from the small angles and the obstacle counts the other
suites feed.

1. `SINCOS_C` restates sincos_poly in C operation for operation (the kernel's constants, fmaf where the kernel
   writes fmaf, the integer xor for the signs; built with -ffp-contract=off like the device code).  Its `measure`
   mode reports the worst error against double sin / cos in ulps of the correctly rounded fp32 result; its
   `fixture` mode turns angles into the restatement's sin / cos bit patterns.
2. `python tests/physics_cases.py --write-fixture` writes tests/golden/physics_sincos.npz from it: the angles of
   `fixture_angles` with those bit patterns.  The device reproduces them to the bit through irm_fk at D = 1, so
   the GPU machine needs no compiler; the CPU suite regenerates the file and compares.
3. The fp64 references of the device tests: FK / Jacobian on the fp32 cumulative angles the device forms, the
   obstacle potential, and Ref64's cost / gradient restated to take those angles.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "physics_sincos.npz")

POLY_MAX = 1.0e4          # sincos_fast: |x| above this goes to sincosf
ULP_BOUND = 2.0           # the asserted bound on sincos_poly's error, ulps of the correctly rounded fp32 result
IDENTITY_BOUND = 4.0 * 2.0 ** -24  # |sin² + cos² − 1| per input
FALLBACK_ULP_BOUND = 4.0  # sincosf (|x| > 1e4): the OpenCL full-profile bound the device math library is built to
MUTANTS = {"sin_sign": "-DMUT_SIN_SIGN", "drop_c2": "-DMUT_DROP_C2"}

SINCOS_C = r"""
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static inline float fb(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t bf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* irm_physics.hpp, sincos_poly: the same operations in the same order */
static void sincos_poly(float x, float* sn, float* cs) {
    const float t = fmaf(x, 0.636619772f, 12582912.0f);
    const float kf = t - 12582912.0f;
    float r = fmaf(kf, -1.57079637050628662109375f, x);
#ifndef MUT_DROP_C2
    r = fmaf(kf, 4.371138828673793e-08f, r);
#endif
    r = fmaf(kf, 1.7151245100058819e-15f, r);
    const float z = r * r;
    const float sp = fmaf(r * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), r);
    const float cp = fmaf(z * z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f),
                          fmaf(-0.5f, z, 1.0f));
    const uint32_t qi = bf(t); /* k mod 4 in the low bits (two's complement: the unsigned sum is the same bits) */
    const float s0 = (qi & 1u) ? cp : sp;
    const float c0 = (qi & 1u) ? sp : cp;
#ifdef MUT_SIN_SIGN
    *sn = fb(bf(s0) ^ (((qi + 1u) << 30) & 0x80000000u));
#else
    *sn = fb(bf(s0) ^ ((qi << 30) & 0x80000000u));
#endif
    *cs = fb(bf(c0) ^ (((qi + 1u) << 30) & 0x80000000u));
}

static double ws = 0, wc = 0, wi = 0;     /* worst sin / cos error (ulp), worst |sin² + cos² − 1| */
static float xs = 0, xc = 0, xi = 0;      /* ... and where */
static long long n = 0, ibad = 0;
static double id_bound;

static inline double ulps(float got, double exact) {
    const float rf = fabsf((float)exact);                  /* the correctly rounded result's ulp */
    const double u = (double)nextafterf(rf, INFINITY) - (double)rf;
    return fabs((double)got - exact) / u;
}
static inline void probe(float x) {
    if (!(fabsf(x) <= 1.0e4f)) return;
    float s, c;
    sincos_poly(x, &s, &c);
    double sd, cd;
    sincos((double)x, &sd, &cd);
    const double es = ulps(s, sd), ec = ulps(c, cd);
    const double id = fabs((double)s * (double)s + (double)c * (double)c - 1.0);
    if (!(es <= ws)) { ws = es; xs = x; }                  /* (a NaN counts as the worst) */
    if (!(ec <= wc)) { wc = ec; xc = x; }
    if (!(id <= wi)) { wi = id; xi = x; }
    ibad += !(id <= id_bound);
    ++n;
}
/* the fp32 numbers in their order as integers */
static inline int64_t ord(float f) { const uint32_t u = bf(f); return (u >> 31) ? -(int64_t)(u & 0x7fffffffu) : (int64_t)u; }
static inline float unord(int64_t o) { return o < 0 ? fb(0x80000000u | (uint32_t)(-o)) : fb((uint32_t)o); }
static void around(double centre) {
    const int64_t o = ord((float)centre);
    for (int64_t d = -64; d <= 64; ++d) probe(unord(o + d));
}
static uint64_t st;
static inline uint64_t xr(void) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; }
static inline double u01(void) { return (double)(xr() >> 11) * 0x1p-53; }

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "fixture")) {        /* fp32 angles on stdin -> (sin bits, cos bits) on stdout */
        float x;
        while (fread(&x, 4, 1, stdin) == 1) {
            float s, c;
            sincos_poly(x, &s, &c);
            const uint32_t o[2] = {bf(s), bf(c)};
            fwrite(o, 4, 2, stdout);
        }
        return 0;
    }
    /* measure <part> <parts> <log2 of the random-pattern count>: this part's share of the probes */
    const int part = atoi(argv[2]), parts = atoi(argv[3]), lg = atoi(argv[4]);
    id_bound = 4.0 * 0x1p-24;
    const double hp = 1.57079632679489661923, qp = 0.78539816339744830962;
    const int kmax = (int)(1.0e4 / hp) + 1;
    for (int k = -kmax; k <= kmax; ++k) {
        if (((k + kmax) % parts) != part) continue;
        around(k * hp);                                    /* multiples of π/2 */
        around((2 * k + 1) * qp);                          /* odd multiples of π/4 */
    }
    st = 88172645463325252ull + 0x9E3779B97F4A7C15ull * (uint64_t)(part + 1);
    const long long cnt = (1ll << lg) / parts;
    for (long long i = 0; i < cnt; ++i) probe(fb((uint32_t)(xr() >> 32)));       /* bit patterns: denormals, ±0, tiny */
    for (long long i = 0; i < cnt / 2; ++i) probe((float)(u01() * 2.0e4 - 1.0e4));
    for (long long i = 0; i < cnt / 2; ++i) probe((float)(u01() * 16.0 - 8.0));
    printf("%lld %.6f %.9g %.6f %.9g %.6e %.9g %lld\n", n, ws, (double)xs, wc, (double)xc, wi, (double)xi, ibad);
    return 0;
}
"""


# ------------------------------------------------------------------------------------------ 1. the restatement
def compile_sincos(workdir, mutant=None):
    """The restatement's executable (None without a host C compiler).  mutant: a key of MUTANTS."""
    src = os.path.join(str(workdir), "sincos.c")
    with open(src, "w") as f:
        f.write(SINCOS_C)
    exe = os.path.join(str(workdir), "sincos" + ("_" + mutant if mutant else ""))
    cmd = ["gcc", "-O2", "-ffp-contract=off"] + ([MUTANTS[mutant]] if mutant else []) + ["-o", exe, src, "-lm"]
    try:
        subprocess.check_call(cmd)
    except (OSError, subprocess.CalledProcessError):
        return None
    return exe


def measure(exe, log2_patterns=26, parts=4):
    """The worst errors over the probe set: every fp32 within ±64 ulps of every multiple of π/2 and odd multiple
    of π/4 up to 1e4, 2^log2_patterns random bit patterns (those with |x| ≤ 1e4 are probed), half as many uniform
    draws in [−1e4, 1e4] and in [−8, 8].  The work is split over `parts` processes."""
    procs = [subprocess.Popen([exe, "measure", str(i), str(parts), str(log2_patterns)], stdout=subprocess.PIPE)
             for i in range(parts)]
    out = dict(n=0, sin_ulp=0.0, sin_at=0.0, cos_ulp=0.0, cos_at=0.0, identity=0.0, identity_at=0.0, identity_bad=0)
    for p in procs:
        text, _ = p.communicate(timeout=600)
        assert p.returncode == 0, p.returncode
        n, ws, xs, wc, xc, wi, xi, ibad = text.split()
        out["n"] += int(n)
        out["identity_bad"] += int(ibad)
        for key, at, val, x in (("sin_ulp", "sin_at", ws, xs), ("cos_ulp", "cos_at", wc, xc),
                                ("identity", "identity_at", wi, xi)):
            if not float(val) <= out[key]:
                out[key], out[at] = float(val), float(x)
    return out


def assert_sincos_bounds(m):
    """The assertions on a `measure` result."""
    assert m["sin_ulp"] < ULP_BOUND, m
    assert m["cos_ulp"] < ULP_BOUND, m
    assert m["identity_bad"] == 0 and m["identity"] <= IDENTITY_BOUND, m


def restate_sincos(exe, x):
    """(sin bits, cos bits) of the restatement for the fp32 angles x."""
    x = np.ascontiguousarray(x, np.float32)
    raw = subprocess.run([exe, "fixture"], input=x.tobytes(), stdout=subprocess.PIPE, check=True, timeout=60).stdout
    bits = np.frombuffer(raw, np.uint32).reshape(-1, 2)
    assert bits.shape[0] == x.shape[0]
    return bits[:, 0].copy(), bits[:, 1].copy()


# ------------------------------------------------------------------------------------------ 2. the fixture
def _neighbours(centres, width=2):
    """The fp32 numbers within ±width ulps of the fp32 nearest each centre."""
    c = np.asarray(centres, np.float64).astype(np.float32)
    out = [c]
    for direction in (np.float32(np.inf), np.float32(-np.inf)):
        x = c
        for _ in range(width):
            x = np.nextafter(x, direction)
            out.append(x)
    return np.concatenate(out)


def fixture_angles():
    """At most 8192 angles with |x| ≤ 1e4: ±{0, the smallest denormal, 2⁻¹²⁶}, the ±2-ulp neighbourhoods of k·π/2
    and (2k+1)·π/4 for |k| ≤ 40, 2000 log-spaced magnitudes from 1e-6 to 1e4 in both signs, 1e4 and its
    predecessor.  Sorted by bit pattern, duplicates removed."""
    k = np.arange(-40, 41)
    mag = np.geomspace(1e-6, 1e4, 2000).astype(np.float32)
    top = np.float32(POLY_MAX)
    parts = [
        np.array([0.0, 2.0 ** -149, 2.0 ** -126], np.float32),
        _neighbours(k * (np.pi / 2)),
        _neighbours((2 * k + 1) * (np.pi / 4)),
        mag,
        np.array([top, np.nextafter(top, np.float32(0))], np.float32),
    ]
    x = np.concatenate(parts).astype(np.float32)
    x = np.concatenate([x, -x])
    x = x[np.abs(x) <= top]
    bits = np.unique(x.view(np.uint32))  # (+0 and −0 are different patterns: both stay)
    assert bits.shape[0] <= 8192
    return bits.view(np.float32)


def make_fixture(exe):
    x = fixture_angles()
    s, c = restate_sincos(exe, x)
    return {"x": x, "sin_bits": s, "cos_bits": c}


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def fallback_angles():
    """The second angle set, |x| ∈ (1e4, 1e7]: sincos_fast's sincosf fallback.  nextafter(1e4, inf) first."""
    top = np.float32(POLY_MAX)
    first = np.nextafter(top, np.float32(np.inf))
    rng = np.random.default_rng(41)
    mag = np.concatenate([[first], _neighbours(np.array([3184, 31831, 318310]) * np.pi),  # next to zeros of sin
                          np.geomspace(1.0001e4, 1e7, 600), rng.uniform(1e4, 1e7, 300), [1e7]]).astype(np.float32)
    mag = mag[(mag > top) & (mag <= np.float32(1e7))]
    x = np.concatenate([mag, -mag])
    return np.unique(x.view(np.uint32)).view(np.float32)


def pack_angles(x, N=50):
    """Angles as B×N×1 trajectories, the tail padded with zeros; returns (traj, count)."""
    n = x.shape[0]
    B = (n + N - 1) // N
    t = np.zeros(B * N, np.float32)
    t[:n] = x
    return t.reshape(B, N, 1), n


def ulp_error(got, exact):
    """|got − exact| in ulps of the correctly rounded fp32 result (exact: fp64)."""
    rf = np.abs(np.asarray(exact, np.float64).astype(np.float32))
    u = np.nextafter(rf, np.float32(np.inf)).astype(np.float64) - rf.astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - exact) / u


# ------------------------------------------------------------------------------------------ 3. fp64 references
def quadrants(cum):
    """The Cody-Waite quadrant index k = round(x·2/π) of fp32 angles (as the shifter forms it, up to ties)."""
    return np.rint(np.asarray(cum, np.float64) * (2.0 / np.pi)).astype(np.int64)


def cum32(q):
    """The device's cumulative joint angles: fp32, left to right (… × D)."""
    return np.cumsum(np.asarray(q, np.float32), axis=-1, dtype=np.float32)


def fk64(cum, link):
    """FK and end-effector Jacobian in fp64 on given cumulative angles (… × D): x, y (…), jx, jy (… × D), and
    the joint positions px, py (… × D)."""
    c = np.asarray(cum, np.float64)
    ll = np.asarray(link, np.float64)
    lx, ly = ll * np.cos(c), ll * np.sin(c)
    px, py = np.cumsum(lx, -1), np.cumsum(ly, -1)
    sx, cy = -ly, lx
    jx = sx + sx.sum(-1, keepdims=True) - np.cumsum(sx, -1)
    jy = cy + cy.sum(-1, keepdims=True) - np.cumsum(cy, -1)
    return px[..., -1], py[..., -1], jx, jy, px, py


def potential64(x, y, obs):
    """environment.py:46-58 in fp64: cv, ∂cv/∂x, ∂cv/∂y for points x, y (any shape) against obs — O×2 shared, or
    shape(x) + (O, 2) per point (a moving table).  An empty table gives zeros."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    obs = np.asarray(obs, np.float64)
    if obs.size == 0:
        return np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape)
    with np.errstate(over="ignore"):
        dx, dy = x[..., None] - obs[..., 0], y[..., None] - obs[..., 1]
        den = 0.5 + 0.5 * (dx * dx + dy * dy)
        return (0.8 / den).sum(-1), (-0.8 * dx / den ** 2).sum(-1), (-0.8 * dy / den ** 2).sum(-1)


def waypoint_cost64(cum, link, obs, whole):
    """The per-waypoint obstacle cost on given cumulative angles (… × D): the end effector's potential, or its
    sum over the joint positions (whole robot).  obs per point: shape(cum)[:-1] + (O, 2)."""
    x, y, _, _, px, py = fk64(cum, link)
    if not whole:
        return potential64(x, y, obs)[0]
    return sum(potential64(px[..., j], py[..., j], obs)[0] for j in range(px.shape[-1]))


class CumRef64:
    """Ref64.cost_tv / grad_ab / cost_g (oracle/ref64.py) with lambda_sg = lambda_jl = 0 — the obstacle term is the
    whole cost — restated to take the fp32 cumulative angles of given positions T (the device's own
    evaluate(α, 0)) in place of an fp64 cumulative sum: at |angle| ~ 1e4 one fp32 rounding of the sum moves
    sin / cos by 1e-3, which is the input's rounding and not the kernel's.  The map back to α is Ref64.cost_g's,
    (Kᵀa + dKᵀb)·Jᵀ in fp64 with b = 0."""

    def __init__(self, link, K, dK, J, whole=False):
        self.link = np.asarray(link, np.float64)
        self.K, self.dK, self.J = (np.asarray(m, np.float64) for m in (K, dK, J))
        self.whole = bool(whole)

    def waypoint_cost(self, T, obs):
        return waypoint_cost64(cum32(T), self.link, obs, self.whole)

    def cost(self, T, obs, lmax):
        cv = self.waypoint_cost(T, obs)
        return lmax * cv.max() + (1 - lmax) * cv.mean()

    def argmax_margin(self, T, obs):
        """(leader − runner-up) / leader of the per-waypoint cost."""
        cv = np.sort(self.waypoint_cost(T, obs))
        return (cv[-1] - cv[-2]) / cv[-1]

    def grad(self, T, obs, lmax):
        N = T.shape[0]
        x, y, jx, jy, px, py = fk64(cum32(T), self.link)
        if not self.whole:
            cv, gx, gy = potential64(x, y, obs)
            da = gx[:, None] * jx + gy[:, None] * jy
        else:
            c = cum32(T).astype(np.float64)
            sx, cy = -(self.link * np.sin(c)), self.link * np.cos(c)
            cv, da = np.zeros(N), np.zeros(T.shape)
            for j in range(T.shape[1]):
                cj, gxj, gyj = potential64(px[:, j], py[:, j], obs)
                cv += cj
                for k in range(j + 1):
                    da[:, k] += sx[:, k:j + 1].sum(1) * gxj + cy[:, k:j + 1].sum(1) * gyj
        w = np.full(N, (1 - lmax) / N)
        w[int(np.argmax(cv))] += lmax
        a = w[:, None] * da
        return (self.K.T @ a) @ self.J.T


# ------------------------------------------------------------------------------------------ scenes
SCALES = (1.0, 40.0)  # … and the shape's S_big (big_scale)
OBSTACLE_COUNTS = (0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 63, 64)


def scaled_alpha(N, D, scales, per_scale, seed):
    """α = scale · 0.2·randn, `per_scale` trajectories per scale, scale-major: (len(scales)·per_scale) × N × D."""
    rng = np.random.default_rng(seed)
    base = (0.2 * rng.standard_normal((len(scales), per_scale, N, D))).astype(np.float32)
    a = base * np.asarray(scales, np.float32)[:, None, None, None]
    return a.reshape(-1, N, D).astype(np.float32)


def wave_kinds(cum, wave=64):
    """For cumulative angles of B × M samples (B × M × D): per 64-sample wave (the last one ragged), 0 if every
    |cum| ≤ 1e4, 2 if every sample has one above, 1 if both kinds of sample occur.  B × ⌈M/64⌉."""
    big = (np.abs(cum) > np.float32(POLY_MAX)).any(-1)
    B, M = big.shape
    out = np.zeros((B, (M + wave - 1) // wave), np.int64)
    for w in range(out.shape[1]):
        blk = big[:, w * wave:(w + 1) * wave]
        out[:, w] = np.where(blk.all(1), 2, np.where(blk.any(1), 1, 0))
    return out


def sweep_obstacles(O, on, seed=0):
    """The obstacle table of the count sweep, O × 2 fp32: uniform in [−3.5, 3.5]²; for O ≥ 2 the first obstacle
    exactly on the fp32 point `on` (e = 1, dx = 0) and the last at distance 1e6; for O ≥ 3 one at (−2e19, 3e19),
    whose squared distance overflows fp32 like a sentinel's and must add 0; for O ≥ 5 one at distance 1e10, where
    u² = 1e-40 underflows."""
    rng = np.random.default_rng(500 + 31 * O + seed)
    obs = rng.uniform(-3.5, 3.5, (O, 2)).astype(np.float32)
    if O >= 2:
        obs[0] = np.asarray(on, np.float32)
        obs[O - 1] = np.float32(0.6e6), np.float32(-0.8e6)
    if O >= 3:
        obs[O // 2] = np.float32(-2e19), np.float32(3e19)
    if O >= 5:
        obs[O - 2] = np.float32(0.8e10), np.float32(0.6e10)
    return obs


def sweep_velocities(O, seed=0):
    """Velocities for sweep_obstacles, multiples of 2⁻⁸ in [−2, 2] as moving_cases.dyadic_scene draws them; the
    coincident, the far and the overflowing obstacles stand still (so the first stays on its point)."""
    rng = np.random.default_rng(900 + 17 * O + seed)
    w = (rng.integers(-2 * 256, 2 * 256 + 1, (O, 2)) / 256.0).astype(np.float32)
    if O >= 2:
        w[0] = 0
        w[O - 1] = 0
    if O >= 3:
        w[O // 2] = 0
    if O >= 5:
        w[O - 2] = 0
    return w


def write_fixture(path=FIXTURE):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = compile_sincos(d)
        if exe is None:
            raise SystemExit("no host C compiler")
        fx = make_fixture(exe)
    np.savez(path, **fx)
    print(f"wrote {path}: {fx['x'].shape[0]} angles")


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-fixture"]:
        write_fixture()
    else:
        raise SystemExit("usage: python tests/physics_cases.py --write-fixture")
