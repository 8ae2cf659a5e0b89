"""The per-waypoint physics of irm_physics.hpp on an MI355X, off the beaten path: sincos_poly / sincos_fast
over every quadrant and beyond the 1e4 fallback threshold, the FK / Jacobian recurrences, and the obstacle
potential's three forms at the obstacle counts where its blocks begin and end and on degenerate geometry.
Inputs, references and the fixture: tests/physics_cases.py; tests/test_physics_host.py measures the C
restatement of sincos_poly whose bit patterns tests/golden/physics_sincos.npz holds.

Every reference is fp64 on the fp32 cumulative joint angles the device itself forms (its own positions, summed
left to right in fp32): at |angle| ~ 1e4 … 1e5 one rounding of the angle moves sin / cos by 1e-3 … 1e-2, and
that is the input's rounding, not the kernel's.  Every test prints the kernel it reached, the measured error
and, where there is one, the small-angle guard's error beside it.

Measured on the MI355X: see the tests' docstrings.
"""
import functools

import numpy as np
import pytest

import moving_cases as mc
import physics_cases as pc
import variant_shape_cases as vc
from conftest import obstacles, params
from test_gpu_dense import _check_report, eval_grid

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24   # one ulp of an fp32 in [0.5, 1)
M_DENSE = 200      # evaluation times of the dense checks: four waves, the last one of 8 samples
BIG = {3: 3.0e4, 7: 2.0e4}  # S_big per joint count: cumulative angles up to 5e4 … 1.3e5, on both sides of 1e4
PER_SCALE = {3: 2, 7: 3}    # trajectories per scale: B = 6 (k_forward: 5 per workgroup), B = 9 (2 per workgroup)
# (N, D) -> the seed of α: one for which the dense check's waves are of all three kinds (N, D = 50, 3 and
# 128, 7) and the small-angle problems' arg-max waypoint leads by more than 1e-3 (the tests assert both)
ALPHA_SEED = {(50, 3): 2, (128, 3): 5, (128, 7): 3, (256, 3): 9, (33, 3): 1}
# obstacle count -> the seed of the forward sweep's α: the first ≥ 5 with every problem's arg-max margin above 1e-3
SWEEP_SEED = {0: 5, 1: 5, 2: 5, 3: 5, 4: 5, 5: 6, 8: 6, 9: 18, 12: 7, 13: 11, 16: 6, 17: 6, 63: 7, 64: 8}


@functools.lru_cache(maxsize=None)
def ctx(*argv, **overrides):
    from irm_motion_planning_amd.context import Context
    return Context(params(*argv, **overrides))


def links_of(c):
    return [float(c.params.link_length[i]) for i in range(c.D)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scales_of(D):
    return pc.SCALES + (BIG[D],)


def alpha_of(N, D):
    """α at the three scales, scale-major (the first PER_SCALE[D] rows are the small-angle guard)."""
    return pc.scaled_alpha(N, D, scales_of(D), PER_SCALE[D], ALPHA_SEED[(N, D)])


def per_scale(err, D):
    """The worst of per-problem errors per scale."""
    return np.asarray(err, np.float64).reshape(len(scales_of(D)), -1).max(1)


# ------------------------------------------------------------------ 3. trigonometry through irm_fk at D = 1
def d1_ctx():
    return ctx("--n-joints", "1", "--link-length", "1.0", "--n-timesteps", "50")


def fk_d1(x):
    """(cos, sin, −sin, cos) as k_fk<1> returns them for the angles x (pos, then the Jacobian), and fk_joints."""
    c = d1_ctx()
    traj, n = pc.pack_angles(x, 50)
    pos, jac = c.fk(traj, with_jacobian=True)
    joints = c.fk_joints(traj)
    assert pos.shape == (traj.shape[0], 2, 50) and jac.shape == (traj.shape[0], 2, 50, 1)
    np.testing.assert_array_equal(bits(joints[:, 0]), bits(pos))  # irm_fk_joints: the same bits
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)[:n]
    return flat(pos[:, 0]), flat(pos[:, 1]), flat(jac[:, 0, :, 0]), flat(jac[:, 1, :, 0])


def test_d1_fk_reproduces_the_restatement_to_the_bit():
    """With one joint of length 1, k_fk returns pos = (cos q, sin q) and jac = (−sin q, cos q) with no other
    rounding (0 + 1·c is exact, (x + S) − C = x for S = C = x, no contraction): for the fixture's angles,
    |x| ≤ 1e4, they equal the C restatement's values — compared by value, since 0 + (−0) = +0.  The gap between
    the device and the restatement: none (0 of 4820 angles differ, in any of the four outputs)."""
    fx = pc.load_fixture()
    x = fx["x"]
    assert np.abs(x).max() == np.float32(pc.POLY_MAX)
    want_s, want_c = fx["sin_bits"].view(np.float32), fx["cos_bits"].view(np.float32)
    cs, sn, jx, jy = fk_d1(x)
    diff = [int(np.sum(a != b)) for a, b in ((sn, want_s), (cs, want_c), (jx, -want_s), (jy, want_c))]
    print(f"k_fk<1>, k_fk_joints<1>: {x.shape[0]} angles, values that differ from the restatement (sin, cos, jac x, "
          f"jac y): {diff}")
    assert np.array_equal(sn, want_s) and np.array_equal(cs, want_c)
    assert np.array_equal(jx, -want_s) and np.array_equal(jy, want_c)


def test_d1_fk_fallback_is_within_four_ulp():
    """|x| ∈ (1e4, 1e7], nextafter(1e4, inf) and its negative included: sincos_fast's sincosf fallback, per lane,
    against fp64 sin / cos of the fp32 angle.  Bound: 4 ulp, the OpenCL full-profile bound the device math library
    is built to.  Measured: sin 0.94 ulp (at x = 2109591.8), cos 1.22 ulp (at x = 2594369.8)."""
    x = pc.fallback_angles()
    first = np.nextafter(np.float32(pc.POLY_MAX), np.float32(np.inf))
    assert np.all(np.abs(x) > np.float32(pc.POLY_MAX)) and first in x and -first in x
    cs, sn, jx, jy = fk_d1(x)
    x64 = x.astype(np.float64)
    es, ec = pc.ulp_error(sn, np.sin(x64)), pc.ulp_error(cs, np.cos(x64))
    print(f"k_fk<1> sincosf fallback, {x.shape[0]} angles in (1e4, 1e7]: sin {es.max():.3f} ulp at {x[np.argmax(es)]!r}, "
          f"cos {ec.max():.3f} ulp at {x[np.argmax(ec)]!r} (bound {pc.FALLBACK_ULP_BOUND})")
    assert es.max() <= pc.FALLBACK_ULP_BOUND and ec.max() <= pc.FALLBACK_ULP_BOUND
    assert np.array_equal(jx, -sn) and np.array_equal(jy, cs)


# ------------------------------------------------------------------ 4. FK and Jacobian over all quadrants
def quadrant_trajectories(D, N=50):
    """7 trajectories uniform in the joint range [−1, 2] per joint and 4 of them scaled ×20: B·N = 550 waypoints,
    three workgroups of k_fk with a ragged last one."""
    rng = np.random.default_rng(60 + D)
    q = rng.uniform(-1.0, 2.0, (11, N, D)).astype(np.float32)
    q[7:] *= np.float32(20.0)
    return q


@pytest.mark.parametrize("D", [3, 8])
def test_fk_and_jacobian_over_all_quadrants(D):
    """k_fk / k_fk_joints at N = 50 against fp64 sin / cos of the fp32 cumulative angles and fp64 sums.  Position
    bound Σ|L_d|·3·2⁻²⁴ (2 ulp of trigonometry, tests/test_physics_host.py, one more per term for the fp32 product
    and the running sum), Jacobian 2·Σ|L|·3·2⁻²⁴ (the (x + S) − C form).
    Measured: D = 3 position 3.1e-7 (bound 5.4e-7), Jacobian 5.0e-7 (1.1e-6); D = 8 position 3.2e-7, Jacobian 4.2e-7."""
    argv = ["--n-timesteps", "50", "--n-joints", str(D)]
    if D != 3:
        argv += ["--link-length"] + [str(3.0 / D)] * D
    c = ctx(*argv)
    link = links_of(c)
    q = quadrant_trajectories(D)
    assert (q.shape[0] * q.shape[1]) % 256 != 0 and q.shape[0] * q.shape[1] > 512
    cum = pc.cum32(q)
    k = pc.quadrants(cum)
    seen = {(int(m), bool(neg)) for m, neg in zip((k % 4).ravel(), (k < 0).ravel())}
    assert seen >= {(m, neg) for m in range(4) for neg in (False, True)}, seen  # every k mod 4, both signs of k
    assert np.abs(k).max() >= 8 and np.abs(cum).max() <= pc.POLY_MAX
    pos, jac = c.fk(q, with_jacobian=True)
    x, y, jx, jy, _, _ = pc.fk64(cum, link)
    sumL = float(np.sum(np.abs(link)))
    ep = max(np.abs(pos[:, 0] - x).max(), np.abs(pos[:, 1] - y).max())
    ej = max(np.abs(jac[:, 0] - jx).max(), np.abs(jac[:, 1] - jy).max())
    bp, bj = sumL * 3 * ULP, 2 * sumL * 3 * ULP
    print(f"k_fk<{D}> N=50 B=11, k in [{k.min()}, {k.max()}]: |pos - fp64| {ep:.2e} (bound {bp:.2e}), "
          f"|jac - fp64| {ej:.2e} (bound {bj:.2e})")
    assert ep <= bp and ej <= bj
    joints = c.fk_joints(q)
    np.testing.assert_array_equal(bits(joints[:, D - 1]), bits(pos))


# ------------------------------------------------------------------ 5. the wave-uniform branch (irm_dense_check)
@pytest.mark.parametrize("whole", [False, True], ids=["end-effector", "whole-robot"])
@pytest.mark.parametrize("N,D", [(50, 3), (128, 7)])
def test_dense_check_on_both_sides_of_the_fallback(N, D, whole):
    """k_dense_check's per-sample cost on M = 200 times (four waves, the last ragged) for α = scale·0.2·randn,
    scale ∈ {1, 40, S_big}: eval_waypoint takes sincos_fast for a whole wave as soon as one lane's |angle| exceeds
    1e4, sincos_poly otherwise.  The device's own q = eval_any(α) (bit-identical to what the kernel evaluates,
    test_support_times_reproduce_evaluate) shows all three kinds of wave: every lane below, lanes on both sides,
    every lane above.  Reference: fp64 FK on the fp32 cumulative sum of q, fp64 potential; rtol 1e-5 per sample
    (test_cost_samples_match_fp64_fk's bound), the scale-1 rows measured beside it as the guard.
    Measured (scale 1 / 40 / S_big): (50, 3) end effector 2.0e-7 / 2.1e-7 / 1.8e-7, whole robot 1.7e-7 / 1.4e-7 /
    1.7e-7; (128, 7) end effector 1.9e-7 / 1.6e-7 / 1.7e-7, whole robot 1.6e-7 / 1.5e-7 / 1.8e-7; by kind of wave
    (below / mixed / above) at most 2.1e-7 / 1.8e-7 / 1.8e-7."""
    c = ctx(*mc.shape_argv(N, D), whole_robot_cost=int(whole))
    link, obs = links_of(c), obstacles()
    a = alpha_of(N, D)
    c.set_eval_times(eval_grid(M_DENSE))
    q = c.eval_any(a, 0)
    cum = pc.cum32(q)
    kinds = pc.wave_kinds(cum)
    ps = PER_SCALE[D]
    assert kinds.shape == (3 * ps, 4)
    assert (kinds[:ps] == 0).all(), kinds          # the guard rows: every wave below the threshold
    assert {0, 1, 2} <= set(kinds.ravel().tolist()), kinds
    assert 1 in kinds[:, :3] and 2 in kinds[:, :3], kinds  # … mixed and all-above among the full waves too
    rep = _check_report(c, a, obs)                 # max / argmax / avg consistent with the samples
    cost = rep["cost"]
    ref = pc.waypoint_cost64(cum, link, obs, whole)
    err = np.abs(cost - ref) / np.abs(ref)
    by_kind = [max(float(err[b, w * 64:(w + 1) * 64].max()) for b, w in zip(*np.nonzero(kinds == kind)))
               for kind in range(3)]
    es = per_scale(err.max(1), D)
    print(f"k_dense_check<{D}> N={N} M={M_DENSE} whole={whole} max|cum| {np.abs(cum).max():.3g}, waves per kind "
          f"{[int((kinds == i).sum()) for i in range(3)]}: cost rel err at scale 1 (guard) {es[0]:.1e}, 40 {es[1]:.1e}, "
          f"{BIG[D]:g} {es[2]:.1e}; by kind of wave (below / mixed / above) "
          f"{by_kind[0]:.1e} / {by_kind[1]:.1e} / {by_kind[2]:.1e}")
    assert np.isfinite(cost).all()
    assert es[0] <= 1e-5, ("the input is wrong, not the branch", es)
    assert np.all(err <= 1e-5), es


# ------------------------------------------------------------------ 6. k_forward at large angles
def forward_reference(c, a, obs, lmax, whole=False):
    """(cost B, gradient B×N×D, arg-max margin B) of CumRef64 on the device's own evaluate(α, 0)."""
    _, K, dK, J = c.kernel_matrices()
    R = pc.CumRef64(links_of(c), K, dK, J, whole)
    T = c.evaluate(a, 0)
    cost = np.array([R.cost(T[b], obs, lmax) for b in range(a.shape[0])])
    G = np.stack([R.grad(T[b], obs, lmax) for b in range(a.shape[0])])
    margin = np.array([R.argmax_margin(T[b], obs) for b in range(a.shape[0])])
    return cost, G, margin, T


def forward_errors(cost, G, ref, Gref):
    B = ref.shape[0]
    ec = np.abs(cost - ref) / np.abs(ref)
    eg = np.abs(G - Gref).reshape(B, -1).max(1) / np.abs(Gref).reshape(B, -1).max(1)
    return ec, eg


@pytest.mark.parametrize("lmax", [0.0, 0.5])
@pytest.mark.parametrize("N,D", [(50, 3), (128, 3), (128, 7)])
def test_forward_cost_and_gradient_at_large_angles(N, D, lmax):
    """irm_eval_cost / irm_eval_cost_grad (k_forward) with λsg = λjl = 0 — the obstacle term is the whole cost —
    on the three α scales in one batch, B no multiple of the trajectories per workgroup (6 at 5, 9 at 2).
    Reference: pc.CumRef64 — Ref64.cost_tv / grad_ab on the fp32 cumulative angles of the device's own
    evaluate(α, 0) (velocities do not enter with λsg = λjl = 0), mapped back by (Kᵀa)·Jᵀ in fp64.  Bounds
    vc.COST_RTOL, vc.GRAD_RTOL·max|G|; the scale-1 rows are the guard.  λmax = 0.5: on every problem the
    reference's largest waypoint cost leads the runner-up by more than 1e-4 relative.
    Measured: cost ≤ 9.2e-8 at every scale (guard ≤ 8.1e-8), gradient ≤ 6.3e-6·max|G| (guard ≤ 2.9e-6)."""
    c = ctx(*mc.shape_argv(N, D))
    a, obs = alpha_of(N, D), obstacles()
    B = a.shape[0]
    tb = min(16 // D, (1024 if D < 5 else 512) // (64 * ((N + 63) // 64)))
    assert B % tb != 0 and B > tb, (B, tb)
    s = g = np.zeros((B, D), np.float32)
    ref, Gref, margin, T = forward_reference(c, a, obs, lmax)
    assert np.abs(pc.cum32(T[-PER_SCALE[D]:])).max() > pc.POLY_MAX > np.abs(pc.cum32(T[:-PER_SCALE[D]])).max()
    if lmax > 0:
        assert np.all(margin > 1e-4), margin
    G, cost = c.eval_cost_grad(a, obs, s, g, 0.0, 0.0, lmax, with_cost=True)
    np.testing.assert_array_equal(cost, c.eval_cost(a, obs, s, g, 0.0, 0.0, lmax))
    ec, eg = forward_errors(cost, G, ref, Gref)
    ecs, egs = per_scale(ec, D), per_scale(eg, D)
    print(f"k_forward<{D}> N={N} B={B} TB={tb} lmax={lmax} max|cum| {np.abs(pc.cum32(T)).max():.3g} margin ≥ "
          f"{margin.min():.1e}: cost rel err / |G - ref|/max|G| at scale 1 (guard) {ecs[0]:.1e} / {egs[0]:.1e}, 40 "
          f"{ecs[1]:.1e} / {egs[1]:.1e}, {BIG[D]:g} {ecs[2]:.1e} / {egs[2]:.1e}")
    assert np.isfinite(G).all() and np.isfinite(cost).all()
    assert ecs[0] <= vc.COST_RTOL and egs[0] <= vc.GRAD_RTOL, ("the input is wrong, not the angles", ecs, egs)
    assert np.all(ec <= vc.COST_RTOL), ec
    assert np.all(eg <= vc.GRAD_RTOL), eg


# ------------------------------------------------------------------ 7. obstacle counts and degenerate geometry
def small_alpha(B=6, N=50, D=3, seed=5):
    return pc.scaled_alpha(N, D, (1.0,), B, seed)


@pytest.mark.parametrize("O", pc.OBSTACLE_COUNTS)
def test_obstacle_counts_cost_vg(O):
    """k_cost_vg (the plain form) on 300 free points, one of them exactly on an obstacle (r² = 0), with an
    obstacle at 1e6, one at 1e10 and one beyond 1e19 (adds less than 1e-38), against the fp64 potential with
    test_fk_jacobian_potential's bounds: cost rtol 2e-6, gradient rtol 1e-5 + atol 1e-7.  The oracle's fp32
    compute_cost_vg is measured against the same bound beside it.

    The gradient bound is an elementwise one on sums of terms with Σ|term| = 2 … 8 that cancel to |g| = 1e-3 …
    3e-2, and its atol is less than one ulp of 1: with fp32 terms and sums k_cost_vg missed it at O = 8, 13, 16,
    63 and 64 (error / bound 1.11, 1.04, 1.79, 1.60, 1.27 on 1 or 2 of the 600 elements; the oracle's fp32 sum
    misses it at O = 63 and 64 too, 1.16 and 2.45).  The kernel now forms the terms and the sums in fp64 and
    rounds once.  Measured with that: cost ≤ 5.9e-8 relative, gradient error / bound 0.01 at every
    count."""
    c = ctx(*mc.shape_argv(50, 3))
    rng = np.random.default_rng(70)
    f = rng.uniform(-3.5, 3.5, (6, 2, 50)).astype(np.float32)
    on = f[1, :, 17].copy()
    obs = pc.sweep_obstacles(O, on)
    cv, cg = c.compute_cost_vg(f, obs)
    rv, rgx, rgy = pc.potential64(f[:, 0], f[:, 1], obs)
    rg = np.stack((rgx, rgy), 1)
    assert np.isfinite(cv).all() and np.isfinite(cg).all()
    if O == 0:
        assert not cv.any() and not cg.any()
        print("k_cost_vg O=0: exact zeros")
        return
    ev = float(np.max(np.abs(cv - rv) / np.abs(rv)))
    eg = float(np.max(np.abs(cg - rg) / (1e-7 + 1e-5 * np.abs(rg))))
    from oracle.oracle import compute_cost_vg
    og = np.stack([compute_cost_vg(f[b], obs)[1] for b in range(f.shape[0])])
    eo = float(np.max(np.abs(og - rg) / (1e-7 + 1e-5 * np.abs(rg))))
    print(f"k_cost_vg O={O}: cost rel err {ev:.1e} (bound 2e-6), gradient error / (1e-7 + 1e-5·|g|) {eg:.2f} (the "
          f"oracle's fp32 sum: {eo:.2f}); at the "
          f"coincident point cost {cv[1, 17]:.7g} (fp64 {rv[1, 17]:.7g})")
    if O >= 2:
        assert rv[1, 17] >= 1.6
    np.testing.assert_allclose(cv, rv, rtol=2e-6, atol=0)
    np.testing.assert_allclose(cg, rg, rtol=1e-5, atol=1e-7)


def dyadic_times(M=M_DENSE):
    """M unsorted multiples of 2⁻⁶ in [−6/64, 70/64]: with sweep_velocities' multiples of 2⁻⁸ (as
    moving_cases.dyadic_scene draws them) t·w is exact, and the kernel's fmaf(t, w, p) is the correctly rounded
    p + t·w — half an ulp of the position, 1.2e-7, from the fp64 table."""
    return (((np.arange(M) * 37) % 77 - 6) / 64.0).astype(np.float32)


@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
@pytest.mark.parametrize("whole", [False, True], ids=["end-effector", "whole-robot"])
@pytest.mark.parametrize("O", pc.OBSTACLE_COUNTS)
def test_obstacle_counts_dense_check(O, whole, moving):
    """k_dense_check's per-sample cost (eval_waypoint's paired form: the straight-line block at 9–12 obstacles,
    the pair loop with 1e20 sentinels elsewhere) at N = 50, D = 3, M = 200, with one obstacle on the fp32
    end-effector position k_fk gives for one sample (e = 1; dx within an ulp of 0, since eval_waypoint sums the
    links with fmaf), one at 1e6, one at 1e10 and one beyond 1e19.  Moving: velocities on a dyadic grid, the
    special obstacles at rest, the others' motion rounded once by the kernel's fmaf.  rtol 1e-5 per sample.
    Measured over the sweep: ≤ 3.6e-7."""
    c = ctx(*mc.shape_argv(50, 3), whole_robot_cost=int(whole))
    link = links_of(c)
    a = small_alpha(3)
    t = dyadic_times() if moving else eval_grid(M_DENSE)
    c.set_eval_times(t)
    q = c.eval_any(a, 0)
    b0, i0 = 1, 77
    fk_ctx = ctx(*mc.shape_argv(50, 3))
    pad = np.zeros((1, 50, 3), np.float32)
    pad[0, 0] = q[b0, i0]
    on = fk_ctx.fk(pad)[0, :, 0].copy()
    obs = pc.sweep_obstacles(O, on)
    w = pc.sweep_velocities(O) if moving else None
    rep = c.dense_check(a, obs, with_cost=True, obstacle_velocity=w)
    cost = rep["cost"]
    assert np.isfinite(cost).all() and np.isfinite(rep["avg_cost"]).all() and np.isfinite(rep["max_cost"]).all()
    if O == 0:
        assert not cost.any() and not rep["max_cost"].any() and not rep["avg_cost"].any()
        print(f"k_dense_check<3> O=0 whole={whole} moving={moving}: exact zeros")
        return
    table = obs.astype(np.float64)
    if moving:
        table = table[None] + t.astype(np.float64)[:, None, None] * w.astype(np.float64)[None]  # M × O × 2
    ref = pc.waypoint_cost64(pc.cum32(q), link, table, whole)
    err = np.abs(cost - ref) / np.abs(ref)
    print(f"k_dense_check<3> O={O} whole={whole} moving={moving}: cost rel err {err.max():.1e} (bound 1e-5); at the "
          f"coincident sample {cost[b0, i0]:.7g} (fp64 {ref[b0, i0]:.7g})")
    if O >= 2:
        assert ref[b0, i0] >= 1.6 - 1e-6
    for b in range(a.shape[0]):
        assert rep["max_cost"][b] == cost[b].max() and rep["argmax_cost"][b] == int(np.argmax(cost[b]))
    np.testing.assert_allclose(cost, ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize("lmax", [0.0, 0.5])
@pytest.mark.parametrize("O", pc.OBSTACLE_COUNTS)
def test_obstacle_counts_forward(O, lmax):
    """k_forward<3> at N = 50 on small angles (item 6's setup at scale 1) over the obstacle counts, one obstacle
    on the fp32 end-effector position of one waypoint: cost vc.COST_RTOL, gradient vc.GRAD_RTOL·max|G|.
    Measured over the sweep: cost ≤ 1.5e-7, gradient ≤ 2.2e-6·max|G|."""
    c = ctx(*mc.shape_argv(50, 3))
    a = small_alpha(6, seed=SWEEP_SEED[O])
    B = a.shape[0]
    s = g = np.zeros((B, 3), np.float32)
    T = c.evaluate(a, 0)
    on = c.fk(T)[2, :, 31].copy()
    obs = pc.sweep_obstacles(O, on)
    G, cost = c.eval_cost_grad(a, obs, s, g, 0.0, 0.0, lmax, with_cost=True)
    np.testing.assert_array_equal(cost, c.eval_cost(a, obs, s, g, 0.0, 0.0, lmax))
    assert np.isfinite(G).all() and np.isfinite(cost).all()
    if O == 0:
        assert not cost.any() and not G.any()
        print(f"k_forward<3> O=0 lmax={lmax}: exact zeros")
        return
    ref, Gref, margin, _ = forward_reference(c, a, obs, lmax)
    if lmax > 0:
        assert np.all(margin > 1e-4), margin
    ec, eg = forward_errors(cost, G, ref, Gref)
    print(f"k_forward<3> N=50 O={O} lmax={lmax} margin ≥ {margin.min():.1e}: cost rel err {ec.max():.1e}, "
          f"|G - ref| {eg.max():.1e}·max|G|")
    assert np.all(ec <= vc.COST_RTOL), ec
    assert np.all(eg <= vc.GRAD_RTOL), eg


# ------------------------------------------------------------------ 8. the optimiser kernels' own evaluation
GD0 = ("--optimizer-name", "gd", "--max-outer-iteration", "1", "--max-inner-iteration", "0", "--lambda-sg-constraint", "0",
       "--lambda-jl-constraint", "0")
# (N, D, whole) -> the kernel launch_plan must name.  k_lean<FixShape<3,256,32>,…,2,…> holds two waypoints per lane:
# its evaluation is eval_waypoint<POT = false> + potential_pair.
OPT_KERNELS = {
    (50, 3, 0): "k_lean<FixShape<3,50,32>,",
    (128, 7, 0): "k_lean<FixShape<7,128,32>,",
    (256, 3, 0): "k_lean<FixShape<3,256,32>,",
    (33, 3, 0): "k_optimize<DynShape<3>,",
    (50, 3, 1): "k_optimize<DynShape<3>,",
}


@pytest.mark.parametrize("O", [8, 9, 12, 13])
@pytest.mark.parametrize("N,D,whole", sorted(OPT_KERNELS))
def test_optimiser_prologue_loss_at_large_angles(N, D, whole, O):
    """GD single loop with max_inner_iteration = 0 and λsg = λjl = 0: the launch returns α0 and final_loss, the
    prologue's in-kernel loss at α0.  Which evaluation feeds it (irm_kernels_impl.hpp): k_lean's prologue calls its
    `evaluate` lambda — eval_waypoint<D, false, true, LEAN> per lane with the obstacle table in VGPRs when
    nq == 3 (O = 9 … 12) and from LDS otherwise (O = 8, 13), or, with two waypoints per lane (N = 256),
    eval_waypoint<POT = false> twice and potential_pair — then `finalize`, whose loss a GD-single-loop launch
    that ends at once stores as final_loss; k_optimize's prologue calls eval_waypoint<D, WHOLE, true, LEAN> and
    stores the loss the same way.  That loss is λmax·max + (1 − λmax)·mean of the per-waypoint potential with the
    context's λmax = 0.5, and must meet item 6's reference on the returned trajectory (traj_out, the kernel's own
    K·α0·J, bit-identical to evaluate(α0)) within vc.COST_RTOL at the three α scales.
    Measured: ≤ 1.5e-7 at every kernel, count and scale (guard ≤ 1.2e-7)."""
    # (N = 256: four trajectories per workgroup is what gives each lane two waypoints, launch_optimize_shape)
    c = ctx(*GD0, *mc.shape_argv(N, D), whole_robot_cost=int(whole), **({"traj_per_block": 4} if N == 256 else {}))
    a0 = alpha_of(N, D)
    B = a0.shape[0]
    pl = c.launch_plan(B, O)
    lean = OPT_KERNELS[(N, D, whole)].startswith("k_lean")
    assert pl["kernel"].startswith(OPT_KERNELS[(N, D, whole)]) and pl["kernel"].endswith(",GD1>" if lean else ",GD>"), pl
    assert bool(pl["lean"]) == lean and pl["waypoints_per_lane"] == (2 if N == 256 else 1), pl
    s = g = np.zeros((B, D), np.float32)
    obs = pc.sweep_obstacles(O, (1.0, 1.5))
    alpha, traj, st = c.optimize(s, g, obs, alpha0=a0)
    np.testing.assert_array_equal(bits(alpha), bits(a0))
    np.testing.assert_array_equal(bits(traj), bits(c.evaluate(a0, 0)))
    assert not st["inner_iterations"].any() and not st["grad_evals"].any()
    lmax = float(c.params.lambda_max_cost)
    assert lmax == 0.5
    _, K, dK, J = c.kernel_matrices()
    R = pc.CumRef64(links_of(c), K, dK, J, bool(whole))
    ref = np.array([R.cost(traj[b], obs, lmax) for b in range(B)])
    loss = st["final_loss"].astype(np.float64)
    es = per_scale(np.abs(loss - ref) / np.abs(ref), D)
    print(f"{pl['kernel']} N={N} D={D} whole={whole} O={O} B={B} max|cum| {np.abs(pc.cum32(traj)).max():.3g}: final_loss "
          f"rel err at scale 1 (guard) {es[0]:.1e}, 40 {es[1]:.1e}, {BIG[D]:g} {es[2]:.1e}")
    assert np.isfinite(loss).all()
    assert es[0] <= vc.COST_RTOL, ("the input is wrong, not the angles", es)
    assert np.all(es <= vc.COST_RTOL), es
