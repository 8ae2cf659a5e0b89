"""Clearance of the arm's links against disc obstacles (Context.clearance / irm_clearance) on an MI355X.

The reference has no counterpart; the yardstick is the fp64 restatement of tests/clearance_cases.py (checked against
brute force by tests/test_clearance_host.py) on the device's own eval_any positions, with the tolerance that file
derives from the stated fp32 arithmetic — nothing here is tuned to what the kernel returns.  What the definition
fixes to the bit (axis-aligned cases, ties, the argmins and counts against the call's own samples, a zero velocity
table, batch independence, the _dev entry point) is asserted to the bit."""
import ctypes

import numpy as np
import pytest

import clearance_cases as cc
from test_gpu_dense import ctx, eval_grid, shape_argv

pytestmark = pytest.mark.gpu

SHAPES = [(50, 3, 1), (50, 3, 63), (50, 3, 64), (50, 3, 65), (50, 3, 300), (128, 7, 300), (50, 1, 65)]
B = cc.B
_CACHE = {}


def inputs(N, D):
    """B trajectories: init_alpha of the seeded starts / goals plus 0.2·standard-normal α (as the dense tests use)."""
    key = ("alpha", N, D)
    if key not in _CACHE:
        c = ctx(*shape_argv(N, D))
        start, goal = cc.problems(D)
        noise = (np.random.default_rng(5).standard_normal((B, N, D)) * 0.2).astype(np.float32)
        _CACHE[key] = (c.init_alpha(start, goal) + noise).astype(np.float32)
    return _CACHE[key]


def sampled(N, D, M):
    """(context with the grid set, α, t_eval, the device's own positions q) — q is computed once per shape."""
    c = ctx(*shape_argv(N, D))
    a = inputs(N, D)
    t = eval_grid(M)
    c.set_eval_times(t)
    key = ("q", N, D, M)
    if key not in _CACHE:
        _CACHE[key] = c.eval_any(a, 0)
    return c, a, t, _CACHE[key]


def scene(name):
    return cc.NEAR if name == "near" else cc.reference_scene()


def per_problem(obs, seed=17):
    """One table per problem: the scene, shifted a little differently for every problem."""
    rng = np.random.default_rng(seed)
    return (obs[None] + rng.uniform(-0.15, 0.15, (B,) + obs.shape)).astype(np.float32)


def reference(q, link, obs, t, vel=None, radius=None, link_radius=0.0):
    """g of clearance64 for every problem: B×M×D×O.  obs / vel / radius shared or with a leading batch axis."""
    out = []
    for b in range(q.shape[0]):
        ob = obs[b] if obs.ndim == 3 else obs
        ve = None if vel is None else (vel[b] if vel.ndim == 3 else vel)
        ra = None if radius is None else (radius[b] if np.ndim(radius) == 2 else radius)
        out.append(cc.clearance64(q[b], link, cc.moved(ob, ve, t), ra, link_radius)[0])
    return np.stack(out)


def bound(q, link, obs, radius=None, link_radius=0.0, vel=None):
    far = float(np.linalg.norm(np.asarray(obs, np.float64), axis=-1).max()) if obs.size else 0.0
    if vel is not None:  # t_eval lies in [−0.1, 1.1]
        far += 1.1 * float(np.linalg.norm(np.asarray(vel, np.float64), axis=-1).max())
    rmax = 0.0 if radius is None else float(np.max(radius))
    return cc.tolerance(link, cc.max_angle(q), far, rmax, link_radius, moving=vel is not None)


def check_against_fp64(rep, g, tol, label):
    """clear_out, link_out, min_clearance, the argmins and the collision counts of one call against g (B×M×D×O).
    Returns the worst error."""
    worst = 0.0
    for b in range(g.shape[0]):
        want = cc.summary64(g[b])
        clear, link = rep["clearance"][b], rep["link_clearance"][b]
        errs = (np.abs(clear - want["clearance"]).max(), np.abs(link - want["link_clearance"]).max(),
                abs(float(rep["min_clearance"][b]) - want["min_clearance"]))
        worst = max(worst, *errs)
        assert max(errs) <= tol, (label, b, errs, tol)
        # the report against the call's own samples: exact
        i, l, o = int(rep["argmin_time"][b]), int(rep["argmin_link"][b]), int(rep["argmin_obstacle"][b])
        assert rep["min_clearance"][b] == clear.min() == link.min(), (label, b)
        assert i == int(np.argmin(clear)) and l == int(np.argmin(link)), (label, b, i, l)
        # ... and the reported (i, l, o) is a minimiser of the fp64 restatement up to the tolerance
        assert 0 <= o < g.shape[3] and g[b, i, l, o] - want["min_clearance"] <= tol, (label, b, i, l, o)
        hit = clear < 0
        assert rep["n_colliding"][b] == hit.sum() and bool(rep["collision_free"][b]) == (not hit.any()), (label, b)
        assert rep["first_colliding"][b] == (int(np.argmax(hit)) if hit.any() else -1), (label, b)
        differ = hit != (want["clearance"] < 0)
        assert np.all(np.abs(want["clearance"][differ]) <= tol), (label, b, want["clearance"][differ])
    return worst


FULL = dict(with_samples=True, with_links=True, with_joints=True)


# ------------------------------------------------- 1. exact cases
def _axis_arm(M=65):
    """α = 0: every q is exactly 0 and sincos(0) is exact — the arm lies on the x axis, joints at 1.5, 2.5, 3."""
    c = ctx()
    c.set_eval_times(eval_grid(M))
    return c, np.zeros((50, 3), np.float32)


@pytest.mark.parametrize("obstacle,value,link", [((2.0, 0.25), 0.25, 1), ((3.5, 0.0), 0.5, 2), ((-1.0, 0.0), 1.0, 0),
                                                 ((1.5, 0.5), 0.5, 0)])
def test_axis_aligned_cases_are_exact(obstacle, value, link):
    c, a = _axis_arm()
    rep = c.clearance(a, np.array([obstacle], np.float32), **FULL)
    np.testing.assert_array_equal(rep["joints"], np.broadcast_to(np.array([[1.5, 0], [2.5, 0], [3, 0]], np.float32),
                                                                 (65, 3, 2)))
    assert rep["min_clearance"] == np.float32(value)
    np.testing.assert_array_equal(rep["clearance"], np.full(65, value, np.float32))
    # every sample is the same: the lowest time, the lowest link on the tie at the joint (1.5, 0.5)
    assert (rep["argmin_time"], rep["argmin_link"], rep["argmin_obstacle"]) == (0, link, 0)
    assert rep["link_clearance"][link] == np.float32(value) and rep["link_clearance"].min() == np.float32(value)
    assert rep["collision_free"] and rep["n_colliding"] == 0 and rep["first_colliding"] == -1


def test_mirrored_obstacles_report_the_lower_index():
    c, a = _axis_arm()
    for lead in (0, 1, 2, 3, 4):  # the pair in an even/odd slot, across two slots, behind other obstacles
        far = np.full((lead, 2), 9.0, np.float32)
        for first in (0.25, -0.25):
            obs = np.concatenate((far, np.array([(2.0, first), (2.0, -first)], np.float32)))
            rep = c.clearance(a, obs)
            assert rep["min_clearance"] == np.float32(0.25)
            assert (rep["argmin_time"], rep["argmin_link"], rep["argmin_obstacle"]) == (0, 1, lead), (lead, first)


def test_touching_is_not_colliding():
    c, a = _axis_arm()
    obs = np.array([(2.0, 0.25)], np.float32)
    rep = c.clearance(a, obs, obstacle_radius=0.25, with_samples=True)
    assert rep["min_clearance"] == 0.0 and rep["collision_free"] and rep["n_colliding"] == 0
    rep = c.clearance(a, obs, obstacle_radius=0.25, link_radius=2.0 ** -20, with_samples=True)
    assert rep["min_clearance"] == np.float32(-2.0 ** -20) and not rep["collision_free"]
    assert rep["n_colliding"] == 65 and rep["first_colliding"] == 0
    rep = c.clearance(a, obs, obstacle_radius=[0.125], link_radius=0.0625)  # (d − radius) − link_radius
    assert rep["min_clearance"] == np.float32(0.0625)


# ------------------------------------------------- 2. joints
@pytest.mark.parametrize("N,D,M", SHAPES)
def test_joints_match_fp64_fk(N, D, M):
    """joints_out against the fp64 FK of the device's own positions q, the angles summed in fp64 too, within the
    project's FK tolerance 1e-6 (DESIGN.md §0 row a5–a11).
    Measured (MI355X) with the plain fp32 prefix sum c_l = c_{l−1} + q_l: 2.1e-7 … 3.8e-7 at D = 3 and D = 1 but
    1.33e-6 at (128, 7, 300), where the angles reach 13.1 rad (half an ulp of 8 … 16 rad is 4.8e-7 per addition, six
    additions, lever arm up to 2.6).  That is why the kernel keeps the additions' rounding and applies it to sin / cos
    (include/irm.h); what is left of the angle's error is of second order, below 1e-11.  With it: 2.1e-7 … 3.6e-7 at every shape, 3.6e-7 at (128, 7, 300)."""
    c, a, t, q = sampled(N, D, M)
    rep = c.clearance(a, cc.NEAR, with_joints=True)
    assert rep["joints"].shape == (B, M, D, 2)
    err = float(np.abs(rep["joints"] - cc.fk64(q, cc.links(D))).max())
    print(f"N={N} D={D} M={M}: worst joint position error {err:.2e} against the fp64 FK of q (max |angle| "
          f"{cc.max_angle(q):.3g})")
    assert err <= 1e-6


# ------------------------------------------------- 3.-5. distances, argmins, collisions
@pytest.mark.parametrize("name", ["near", "reference"])
@pytest.mark.parametrize("N,D,M", SHAPES)
def test_clearance_matches_fp64_restatement(N, D, M, name):
    c, a, t, q = sampled(N, D, M)
    link = cc.links(D)
    obs = scene(name)
    O = obs.shape[0]
    rng = np.random.default_rng(23)
    tables = per_problem(obs)
    worst, tol_max = 0.0, 0.0
    for label, ob, radius, lr in (("shared", obs, None, 0.0),
                                  ("shared+radii", obs, rng.uniform(0.05, 0.3, O).astype(np.float32), 0.03125),
                                  ("per-problem", tables, None, 0.0),
                                  ("per-problem+radii", tables, rng.uniform(0.05, 0.3, (B, O)).astype(np.float32), 0.05)):
        rep = c.clearance(a, ob, obstacle_radius=radius, link_radius=lr, **FULL)
        assert rep["clearance"].shape == (B, M) and rep["link_clearance"].shape == (B, D)
        tol = bound(q, link, ob, radius, lr)
        if D == 3:
            assert tol <= 1e-5, tol  # (the derivation's own sanity bound)
        g = reference(q, link, ob, t, None, radius, lr)
        worst = max(worst, check_against_fp64(rep, g, tol, (name, label)))
        tol_max = max(tol_max, tol)
    print(f"N={N} D={D} M={M} {name}: worst clearance error {worst:.2e}, derived bound {tol_max:.2e}")


@pytest.mark.parametrize("N,D,M", [(50, 3, 64), (50, 3, 300), (128, 7, 300)])
def test_collisions_on_the_near_scene(N, D, M):
    """Discs of radius 0.2 inside the workspace: the fp64 restatement finds colliding and free samples, so the
    comparison of the verdicts (check_against_fp64) is not vacuous."""
    c, a, t, q = sampled(N, D, M)
    rep = c.clearance(a, cc.NEAR, obstacle_radius=0.2, **FULL)
    radius = np.full(cc.NEAR.shape[0], 0.2, np.float32)
    g = reference(q, cc.links(D), cc.NEAR, t, None, radius)
    count = (g.min(axis=(2, 3)) < 0).sum(axis=1)
    print(f"N={N} D={D} M={M}: fp64 colliding samples per problem {count.min()} … {count.max()} of {M}")
    assert count.max() > 0 and count.min() < M
    check_against_fp64(rep, g, bound(q, cc.links(D), cc.NEAR, radius), "near r=0.2")
    assert rep["n_colliding"].sum() > 0 and not rep["collision_free"].all()


# ------------------------------------------------- 6. moving obstacles
def _assert_same(x, y):
    assert set(x) == set(y)
    for name in x:
        np.testing.assert_array_equal(x[name], y[name], err_msg=name)


@pytest.mark.parametrize("N,D,M", [(50, 3, 65), (128, 7, 300)])
def test_moving_obstacles(N, D, M):
    c, a, t, q = sampled(N, D, M)
    link = cc.links(D)
    rng = np.random.default_rng(29)
    for obs in (cc.NEAR, per_problem(cc.reference_scene())):
        radius = rng.uniform(0.05, 0.3, obs.shape[:-1]).astype(np.float32)
        static = c.clearance(a, obs, obstacle_radius=radius, **FULL)
        _assert_same(c.clearance(a, obs, obstacle_velocity=np.zeros_like(obs), obstacle_radius=radius, **FULL), static)
        vel = rng.uniform(-0.6, 0.6, obs.shape).astype(np.float32)
        rep = c.clearance(a, obs, obstacle_velocity=vel, obstacle_radius=radius, **FULL)
        tol = bound(q, link, obs, radius, 0.0, vel)
        worst = check_against_fp64(rep, reference(q, link, obs, t, vel, radius), tol, "moving")
        print(f"N={N} D={D} M={M} moving, {obs.ndim - 1} table(s): worst error {worst:.2e}, derived bound {tol:.2e}")
        # sample i sees the table at t_eval[i]: the restatement at other times (the grid shifted by one) is not it
        if M > 1:
            other = reference(q, link, obs, np.roll(t, 1), vel, radius).min(axis=(2, 3))
            assert np.abs(rep["clearance"] - other).max() > 100 * tol


# ------------------------------------------------- 7. batch independence, the _dev entry point
def test_batch_independence():
    c, a, t, q = sampled(50, 3, 300)
    k = 11
    for obs in (cc.reference_scene(), per_problem(cc.NEAR)):
        radius = np.random.default_rng(31).uniform(0.05, 0.3, obs.shape[:-1]).astype(np.float32)
        vel = np.random.default_rng(37).uniform(-0.6, 0.6, obs.shape).astype(np.float32)
        for v in (None, vel):
            full = c.clearance(a, obs, obstacle_velocity=v, obstacle_radius=radius, link_radius=0.01, **FULL)
            one = c.clearance(a[k], obs[k] if obs.ndim == 3 else obs, obstacle_velocity=None if v is None else
                              (v[k] if v.ndim == 3 else v), obstacle_radius=radius[k] if radius.ndim == 2 else radius,
                              link_radius=0.01, **FULL)
            assert set(full) == set(one) == {"min_clearance", "argmin_time", "argmin_link", "argmin_obstacle",
                                             "n_colliding", "first_colliding", "collision_free", "clearance",
                                             "link_clearance", "joints"}
            for name in full:
                assert full[name].shape[0] == B
                np.testing.assert_array_equal(full[name][k], one[name], err_msg=name)
    # optional outputs do not change the report
    bare = c.clearance(a, cc.NEAR)
    assert set(bare) == {"min_clearance", "argmin_time", "argmin_link", "argmin_obstacle", "n_colliding",
                         "first_colliding", "collision_free"}
    rich = c.clearance(a, cc.NEAR, **FULL)
    for name in bare:
        np.testing.assert_array_equal(bare[name], rich[name], err_msg=name)
    assert bare["collision_free"].dtype == bool


@pytest.mark.parametrize("moving", [False, True])
def test_dev_entry_point_gives_the_host_bits(moving):
    import torch
    from irm_motion_planning_amd.clearance import IrmClearanceReport
    N, D, M = 50, 3, 300
    c, a, t, q = sampled(N, D, M)
    obs = per_problem(cc.NEAR)
    O = obs.shape[1]
    radius = np.random.default_rng(41).uniform(0.05, 0.3, (B, O)).astype(np.float32)
    vel = np.random.default_rng(43).uniform(-0.6, 0.6, obs.shape).astype(np.float32) if moving else None
    want = c.clearance(a, obs, obstacle_velocity=vel, obstacle_radius=radius, link_radius=0.02, **FULL)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        a_t, o_t, r_t = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (a, obs, radius))
        v_t = torch.from_numpy(vel).to(dev) if moving else None
        rep_t = torch.zeros((B, ctypes.sizeof(IrmClearanceReport) // 4), dtype=torch.int32, device=dev)
        clear = torch.full((B, M), float("nan"), device=dev)
        link = torch.full((B, D), float("nan"), device=dev)
        joints = torch.full((B, M, D, 2), float("nan"), device=dev)
        c.clearance_dev(a_t.data_ptr(), o_t.data_ptr(), O, 2 * O, B, rep_t.data_ptr(),
                        obstacle_velocity_dev=v_t.data_ptr() if moving else 0, obstacle_radius_dev=r_t.data_ptr(),
                        link_radius=0.02, clear_dev=clear.data_ptr(), link_dev=link.data_ptr(),
                        joints_dev=joints.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(clear.cpu().numpy(), want["clearance"])
    np.testing.assert_array_equal(link.cpu().numpy(), want["link_clearance"])
    np.testing.assert_array_equal(joints.cpu().numpy(), want["joints"])
    recs = rep_t.cpu().numpy()
    np.testing.assert_array_equal(recs[:, 0].view(np.float32), want["min_clearance"])
    for col, name in enumerate(("argmin_time", "argmin_link", "argmin_obstacle", "n_colliding", "first_colliding"), 1):
        np.testing.assert_array_equal(recs[:, col], want[name], err_msg=name)
    np.testing.assert_array_equal(recs[:, 6].astype(bool), want["collision_free"])
    assert not recs[:, 7].any()


# ------------------------------------------------- 8. bounds
def test_no_obstacles_and_the_most():
    c, a, t, q = sampled(50, 3, 65)
    for empty in (np.zeros((0, 2), np.float32), np.zeros((B, 0, 2), np.float32)):
        rep = c.clearance(a, empty, obstacle_radius=0.2, link_radius=0.1, **FULL)
        assert np.all(rep["min_clearance"] == np.inf) and np.all(rep["clearance"] == np.inf)
        assert np.all(rep["link_clearance"] == np.inf)
        for name in ("argmin_time", "argmin_link", "argmin_obstacle", "first_colliding"):
            assert np.all(rep[name] == -1), name
        assert not rep["n_colliding"].any() and rep["collision_free"].all()
        assert np.abs(rep["joints"] - cc.fk64(q, cc.LINKS3)).max() <= 1e-6
    rng = np.random.default_rng(47)
    obs = rng.uniform(-3.5, 3.5, (64, 2)).astype(np.float32)
    radius = rng.uniform(0.0, 0.2, 64).astype(np.float32)
    for count in (64, 63, 5):  # full pairs, a padded slot, a padded pair
        rep = c.clearance(a, obs[:count], obstacle_radius=radius[:count], **FULL)
        g = reference(q, cc.LINKS3, obs[:count], t, None, radius[:count])
        check_against_fp64(rep, g, bound(q, cc.LINKS3, obs[:count], radius[:count]), f"O={count}")
        assert np.isfinite(rep["clearance"]).all() and rep["argmin_obstacle"].max() < count


def test_the_largest_grid():
    c, a, t, q = sampled(50, 3, 4096)
    rep = c.clearance(a[:4], cc.NEAR, obstacle_radius=0.2, **FULL)
    radius = np.full(4, 0.2, np.float32)
    g = reference(q[:4], cc.LINKS3, cc.NEAR, t, None, radius)
    check_against_fp64(rep, g, bound(q[:4], cc.LINKS3, cc.NEAR, radius), "M=4096")
    # a repeated time far behind its first occurrence: the lower index is reported
    i = int(rep["argmin_time"][0])
    t2 = np.concatenate((t, [t[i]])).astype(np.float32)[1:]
    c.set_eval_times(t2)
    again = c.clearance(a[0], cc.NEAR, obstacle_radius=0.2, with_samples=True)
    if i > 0:
        assert again["argmin_time"] == i - 1
        assert again["clearance"][-1] == again["clearance"][i - 1] == again["min_clearance"]


def test_error_paths():
    from irm_motion_planning_amd._abi import IrmError, c_float_p
    from irm_motion_planning_amd.clearance import IrmClearanceReport
    from irm_motion_planning_amd.context import Context
    from conftest import params
    c = Context(params())
    a = np.zeros((50, 3), np.float32)
    with pytest.raises(IrmError, match="irm_clearance"):  # no evaluation grid
        c.clearance(a, cc.NEAR)
    c.set_eval_times([0.25, 0.5])
    assert c.clearance(a, cc.NEAR)["argmin_time"] == 0
    assert c.clearance(np.zeros((0, 50, 3), np.float32), cc.NEAR, with_samples=True)["clearance"].shape == (0, 2)
    for kw in (dict(link_radius=-0.1), dict(link_radius=np.nan), dict(link_radius=np.inf), dict(obstacle_radius=-0.1),
               dict(obstacle_radius=[0.1, np.nan, 0.1, 0.1]), dict(obstacle_velocity=np.full((4, 2), np.inf))):
        with pytest.raises(IrmError, match="irm_clearance"):
            c.clearance(a, cc.NEAR, **kw)
    with pytest.raises(IrmError, match="irm_clearance"):
        c.clearance(a, np.zeros((65, 2), np.float32))
    with pytest.raises(ValueError):
        c.clearance(a[None], np.zeros((2, 3, 2), np.float32))  # per-problem tables of another batch
    with pytest.raises(ValueError):
        c.clearance(a, cc.NEAR, obstacle_radius=[0.1, 0.2])
    with pytest.raises(ValueError):
        c.clearance(a, cc.NEAR, obstacle_velocity=np.zeros((3, 2)))
    # what the wrapper cannot express, on the C ABI
    lib, h = c.lib, c._h
    p = lambda x: x.ctypes.data_as(c_float_p)  # noqa: E731
    rep = (IrmClearanceReport * 2)()
    obs2 = np.zeros((2, 5, 2), np.float32)
    rad2 = np.zeros((2, 5), np.float32)
    a2 = np.zeros((2, 50, 3), np.float32)
    for fn, tail in ((lib.irm_clearance, ()), (lib.irm_clearance_dev, (None,))):
        name = b"irm_clearance_dev" if tail else b"irm_clearance"
        assert fn(h, p(a2), p(obs2), 5, 0, None, None, 0.0, -1, rep, None, None, None, *tail) == -22  # negative batch
        assert name + b":" in lib.irm_last_error()
        assert fn(h, p(a2), None, 5, 0, None, None, 0.0, 2, rep, None, None, None, *tail) == -22  # obstacles missing
        assert name + b":" in lib.irm_last_error()
        assert fn(h, p(a2), p(obs2), 5, 11, None, p(rad2), 0.0, 2, rep, None, None, None, *tail) == -22  # odd stride
        assert name + b":" in lib.irm_last_error()
        assert fn(h, p(a2), p(obs2), -1, 0, None, None, 0.0, 2, rep, None, None, None, *tail) == -22
        assert fn(h, p(a2), p(obs2), 5, 0, None, None, -1.0, 2, rep, None, None, None, *tail) == -22
        assert name + b":" in lib.irm_last_error()
    assert lib.irm_clearance(h, p(a2), p(obs2), 5, 11, None, None, 0.0, 1, rep, None, None, None) == 0  # no radii: fine
    c.close()


# ------------------------------------------------- the CLI
GD20 = ["--optimizer-name", "gd", "--max-inner-iteration", "20"]


def test_cli_clearance(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(GD20)
    plain = capsys.readouterr().out
    assert "clearance" not in plain
    before = (tmp_path / "trajectory_result.txt").read_bytes()
    irm_main.main(GD20 + ["--dense-check", "64", "--clearance", "64", "--obstacle-radius", "0.2"])
    out = capsys.readouterr().out.splitlines()
    lines = [ln for ln in out if ln.startswith("clearance (64 samples): min ")]
    assert len(lines) == 1, out
    assert " at t=" in lines[0] and " link " in lines[0] and " obstacle " in lines[0], lines[0]
    assert lines[0].endswith("collision-free") or " colliding samples, the first at t=" in lines[0], lines[0]
    assert out.index(lines[0]) > [i for i, ln in enumerate(out) if ln.startswith("dense check (64 samples)")][0]
    assert (tmp_path / "trajectory_result.txt").read_bytes() == before
    # every other line is the run's without the flags (the timing lines carry a time)
    skip = ("took", "setup object", "clearance", "dense check")
    keep = lambda ls: [ln for ln in ls if not ln.startswith(skip)]  # noqa: E731
    assert keep(out) == keep(plain.splitlines())


def test_cli_clearance_batch(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import batch_io, main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(GD20 + ["--batch-size", "8"])
    assert "clearance" not in capsys.readouterr().out
    files = {f: (tmp_path / f).read_bytes() for f in (batch_io.RESULT, batch_io.RESULT_BATCH, batch_io.SUMMARY_BATCH)}
    assert files[batch_io.SUMMARY_BATCH].splitlines()[0] == ("# " + " ".join(batch_io.SUMMARY_COLUMNS)).encode()
    irm_main.main(GD20 + ["--batch-size", "8", "--clearance", "64", "--obstacle-radius", "0.2"])
    out = capsys.readouterr().out.splitlines()
    assert len([ln for ln in out if ln.startswith("clearance (64 samples): min ")]) == 1, out
    tail = [ln for ln in out if ln.startswith("clearance: ")]
    assert len(tail) == 1 and tail[0].endswith(" problems that fulfil the constraints on the support grid collide"), out
    for f in (batch_io.RESULT, batch_io.RESULT_BATCH):
        assert (tmp_path / f).read_bytes() == files[f], f
    summary = (tmp_path / batch_io.SUMMARY_BATCH).read_text().splitlines()
    assert summary[0] == "# " + " ".join(batch_io.SUMMARY_COLUMNS) + " min_clearance"
    old = files[batch_io.SUMMARY_BATCH].decode().splitlines()
    assert len(summary) == len(old) == 9
    for new_row, old_row in zip(summary[1:], old[1:]):
        assert new_row.startswith(old_row + " ") and len(new_row.split()) == 7
        float(new_row.split()[-1])
