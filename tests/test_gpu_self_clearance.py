"""Clearance of the arm's links against each other (Context.self_clearance / irm_self_clearance) on an MI355X.

The reference has no counterpart; the yardstick is the fp64 restatement of tests/self_clearance_cases.py (checked
against brute force by tests/test_self_clearance_host.py) on the device's own eval_any positions, with the tolerance
that file derives from the stated fp32 arithmetic — nothing here is tuned to what the kernel returns.  What the
definition fixes to the bit (the straight arm, touching, ties, the counts and argmins against the call's own samples
and the restatement's flags, the joints of irm_clearance, batch independence, the _dev entry point) is asserted to the
bit.  Count, flag and argmin assertions exclude no sample: each first asserts self_clearance_cases.cap_holds."""
import ctypes

import numpy as np
import pytest

import multistart_cases as mc
import self_clearance_cases as sc
from test_gpu_dense import ctx, eval_grid, shape_argv

pytestmark = pytest.mark.gpu

B = sc.B
# the end of the joint-space line per D: the scenes at D = 3 and 7, arms that curl through themselves at D = 4 and 8
END = {1: (1.0,), 2: (1.0, 1.0), 3: sc.SCENES["fold3"][1], 4: (2.0,) * 4, 7: sc.SCENES["curl7"][1], 8: (1.0,) * 8}
VALUE_SHAPES = [(50, 3, 1), (50, 3, 63), (50, 3, 64), (50, 3, 65), (50, 3, 300), (50, 4, 65), (128, 7, 300), (50, 8, 65)]
FULL = dict(with_samples=True, with_pairs=True, with_joints=True)
_CACHE = {}


def links(D):
    return sc.LINKS3 if D == 3 else (3.0 / D,) * D


def fitted(N, D, ends, noise=False):
    """α = fit_alpha of the lines t·end on the support times (one per row of ends); noise: plus 0.2·standard-normal α,
    as test_gpu_clearance.inputs adds."""
    c = ctx(*shape_argv(N, D))
    ends = np.atleast_2d(np.asarray(ends, np.float64))
    way = (np.linspace(0.0, 1.0, N)[None, :, None] * ends[:, None, :]).astype(np.float32)
    a = c.fit_alpha(way)
    if noise:
        a = a + (np.random.default_rng(5).standard_normal(a.shape) * 0.2).astype(np.float32)
    return a.astype(np.float32)


def batch(N, D, noise=False, scene=None):
    """B trajectories of the shape: the lines to END[D] (or the scene's end), each end varied by a seeded ±5 %."""
    key = ("alpha", N, D, noise, scene)
    if key not in _CACHE:
        if scene is None:
            end = np.asarray(END[D], np.float64)
            ends = end[None, :] * (1.0 + np.random.default_rng(sc.SEED).uniform(-0.05, 0.05, (B, D)))
        else:
            ends = sc.batch_ends(scene)
        _CACHE[key] = fitted(N, D, ends, noise)
    return _CACHE[key]


def positions(c, a, t):
    """The grid set, and the device's own positions of α on it."""
    c.set_eval_times(t)
    return c.eval_any(a, 0)


def check_values(rep, q, link, label, link_radius=0.0):
    """clear_out, pair_out and min_clearance of one call against the restatement on q (B×M×D), and what the report
    must equal in the call's own outputs.  Returns the worst error and the tolerance."""
    tol = sc.tolerance(link, sc.max_angle(q), link_radius)
    D = len(link)
    worst = 0.0
    for b in range(q.shape[0]):
        g, x, _ = sc.self_clearance64(q[b], link, link_radius)
        want = sc.summary64(g, x, D)
        clear, pair = rep["clearance"][b], rep["pair_clearance"][b]
        errs = (np.abs(clear - want["clearance"]).max(), np.abs(pair - want["pair_clearance"]).max(),
                abs(float(rep["min_clearance"][b]) - want["min_clearance"]))
        worst = max(worst, *errs)
        assert max(errs) <= tol, (label, b, errs, tol)
        # the report against the call's own samples: exact
        i, la, lb = int(rep["argmin_time"][b]), int(rep["argmin_link_a"][b]), int(rep["argmin_link_b"][b])
        assert rep["min_clearance"][b] == clear.min() == pair.min(), (label, b)
        assert i == int(np.argmin(clear)) and (la, lb) in sc.pairs(D), (label, b, i, la, lb)
        assert pair[sc.pairs(D).index((la, lb))] == rep["min_clearance"][b], (label, b, la, lb)
        # ... and the reported (i, a, b) is a minimiser of the restatement up to the tolerance
        assert g[i, sc.pairs(D).index((la, lb))] - want["min_clearance"] <= tol, (label, b, i, la, lb)
    return worst, tol


# ------------------------------------------------- 1. values
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("N,D,M", VALUE_SHAPES)
def test_values_match_fp64_restatement(N, D, M, noise):
    c = ctx(*shape_argv(N, D))
    a = batch(N, D, noise)
    t = eval_grid(M) if noise else np.linspace(0, 1, M, dtype=np.float32)
    q = positions(c, a, t)
    rep = c.self_clearance(a, **FULL)
    worst, tol = check_values(rep, q, links(D), (N, D, M, noise))
    crossing = sum(int(sc.self_clearance64(q[b], links(D))[1].any(axis=1).sum()) for b in range(B))
    print(f"N={N} D={D} M={M} noise={noise}: worst error {worst:.2e}, tolerance {tol:.2e}, {crossing} crossing samples "
          f"of {B * M}, reported {int(rep['n_crossing'].sum())}")
    assert rep["clearance"].shape == (B, M) and rep["pair_clearance"].shape == (B, len(sc.pairs(D)))
    with_radius = c.self_clearance(a, link_radius=0.125, **FULL)
    check_values(with_radius, q, links(D), (N, D, M, noise, "capsules"), link_radius=0.125)


@pytest.mark.parametrize("N,D,M", [(50, 1, 65), (50, 2, 65)])
def test_no_pairs(N, D, M):
    c = ctx(*shape_argv(N, D))
    a = batch(N, D, True)
    c.set_eval_times(eval_grid(M))
    rep = c.self_clearance(a, link_radius=0.3, **FULL)
    assert np.all(rep["min_clearance"] == np.inf) and np.all(rep["clearance"] == np.inf)
    assert rep["pair_clearance"].shape == (B, 0)
    for name in ("argmin_time", "argmin_link_a", "argmin_link_b", "first_colliding"):
        assert np.all(rep[name] == -1), name
    assert not rep["n_colliding"].any() and not rep["n_crossing"].any() and rep["collision_free"].all()
    obstacle = c.clearance(a, np.zeros((0, 2), np.float32), with_joints=True)
    np.testing.assert_array_equal(rep["joints"], obstacle["joints"])


# ------------------------------------------------- 2. exact to the bit
def _straight_arm(M=65):
    """α = 0: every q is exactly 0 and sincos(0) is exact — four unit links on the x axis, joints at 1, 2, 3, 4."""
    c = ctx("--n-timesteps", "50", "--n-joints", "4", "--link-length", "1", "1", "1", "1")
    c.set_eval_times(eval_grid(M))
    return c, np.zeros((50, 4), np.float32)


def test_axis_aligned_case_is_exact_and_ties_report_the_lower_index():
    c, a = _straight_arm()
    rep = c.self_clearance(a, **FULL)
    np.testing.assert_array_equal(rep["joints"], np.broadcast_to(
        np.array([[1, 0], [2, 0], [3, 0], [4, 0]], np.float32), (65, 4, 2)))
    # pairs (0,2), (0,3), (1,3): links one, two and one link apart; every orientation is 0 and a zero is not a sign
    np.testing.assert_array_equal(rep["pair_clearance"], np.array([1, 2, 1], np.float32))
    np.testing.assert_array_equal(rep["clearance"], np.ones(65, np.float32))
    assert rep["min_clearance"] == np.float32(1)
    # (0,2) and (1,3) tie in every sample: the lowest time, then the lower pair
    assert (rep["argmin_time"], rep["argmin_link_a"], rep["argmin_link_b"]) == (0, 0, 2)
    assert rep["collision_free"] and rep["n_colliding"] == 0 and rep["n_crossing"] == 0 and rep["first_colliding"] == -1
    thick = c.self_clearance(a, link_radius=0.25, **FULL)
    np.testing.assert_array_equal(thick["pair_clearance"], np.array([0.5, 1.5, 0.5], np.float32))
    assert (thick["argmin_time"], thick["argmin_link_a"], thick["argmin_link_b"]) == (0, 0, 2)


def test_touching_is_not_colliding():
    c, a = _straight_arm()
    rep = c.self_clearance(a, link_radius=0.5, with_samples=True)  # g = 1 − 2·0.5 = 0 for (0,2) and (1,3)
    assert rep["min_clearance"] == 0.0 and np.all(rep["clearance"] == 0.0)
    assert rep["collision_free"] and rep["n_colliding"] == 0 and rep["first_colliding"] == -1
    rep = c.self_clearance(a, link_radius=np.nextafter(np.float32(0.5), np.float32(1)), with_samples=True)
    assert rep["min_clearance"] < 0.0 and not rep["collision_free"]
    assert rep["n_colliding"] == 65 and rep["first_colliding"] == 0 and rep["n_crossing"] == 0


def test_square_fold_matches_the_hand_values():
    """Four unit links folded at right angles close the square: (0,2) and (1,3) are opposite sides, 1 apart, and link
    3's tip returns to link 0's start.  π/2 is no fp32 number, so these hold to the tolerance, not to the bit."""
    c = ctx("--n-timesteps", "50", "--n-joints", "4", "--link-length", "1", "1", "1", "1")
    way = np.broadcast_to(np.array([0.0, np.pi / 2, np.pi / 2, np.pi / 2], np.float32), (50, 4))
    a = c.fit_alpha(np.ascontiguousarray(way))
    q = positions(c, a[None], np.linspace(0.25, 0.75, 5, dtype=np.float32))
    rep = c.self_clearance(a, **FULL)
    g, x, _ = sc.self_clearance64(q[0], (1.0,) * 4)
    tol = sc.tolerance((1.0,) * 4, sc.max_angle(q))
    assert np.abs(rep["pair_clearance"] - g.min(axis=0)).max() <= tol
    assert np.abs(rep["pair_clearance"] - np.array([1.0, 0.0, 1.0])).max() < 2e-2  # (the fit's own error)


def _assert_report_consistent(rep, q, link, link_radius, label):
    """The report against the call's own clear_out and the restatement's flags — under the cap, so no sample is
    excluded."""
    D = len(link)
    for b in range(q.shape[0]):
        g, x, margin = sc.self_clearance64(q[b], link, link_radius)
        tol = sc.tolerance(link, sc.max_angle(q[b]), link_radius)
        shown = (float(margin[x].min()) if x.any() else None, float(np.abs(g[~x]).min()), 16 * tol)
        assert sc.cap_holds(g, x, margin, tol), (label, b, shown)
        clear = rep["clearance"][b]
        crossed = x.any(axis=1)
        hit = crossed | (clear < 0)
        assert rep["n_crossing"][b] == crossed.sum(), (label, b)
        assert rep["n_colliding"][b] == hit.sum() and bool(rep["collision_free"][b]) == (not hit.any()), (label, b)
        assert rep["first_colliding"][b] == (int(np.argmax(hit)) if hit.any() else -1), (label, b)
        np.testing.assert_array_equal(clear < 0, (g < 0).any(axis=1), err_msg=str((label, b)))
        i = int(np.argmin(clear))
        assert rep["argmin_time"][b] == i and rep["min_clearance"][b] == clear[i], (label, b)
        pair = (int(rep["argmin_link_a"][b]), int(rep["argmin_link_b"][b]))
        if crossed[i]:  # every crossing pair holds −2·link_radius exactly: the lowest of them
            assert pair == sc.pairs(D)[int(np.argmax(x[i]))], (label, b, pair)
        else:
            assert g[i, sc.pairs(D).index(pair)] - g[i].min() <= tol, (label, b, pair)


@pytest.mark.parametrize("scene,M,link_radius", [("fold3", 64, 0.0), ("fold3", 65, 0.0), ("fold3", 64, 0.04),
                                                 ("fold3", 65, 0.05), ("lim3", 64, 0.2), ("lim3", 64, 0.28),
                                                 ("lim3", 65, 0.32)])
def test_report_equals_its_own_samples_and_the_restatement_flags(scene, M, link_radius):
    link = sc.SCENES[scene][0]
    c = ctx(*shape_argv(50, 3))
    a = batch(50, 3, scene=scene)
    q = positions(c, a, np.linspace(0, 1, M, dtype=np.float32))
    rep = c.self_clearance(a, link_radius=link_radius, **FULL)
    _assert_report_consistent(rep, q, link, link_radius, (scene, M, link_radius))
    print(f"{scene} M={M} r={link_radius}: crossing {rep['n_crossing'].tolist()}, colliding {rep['n_colliding'].tolist()}")


@pytest.mark.parametrize("N,D", [(50, 3), (50, 4), (128, 7), (50, 8)])
def test_joints_are_the_obstacle_checks_joints(N, D):
    c = ctx(*shape_argv(N, D))
    a = batch(N, D, True)
    c.set_eval_times(eval_grid(300))
    mine = c.self_clearance(a, with_joints=True)["joints"]
    theirs = c.clearance(a, np.array([[0.5, 0.5]], np.float32), with_joints=True)["joints"]
    assert mine.shape == (B, 300, D, 2)
    np.testing.assert_array_equal(mine, theirs)


# ------------------------------------------------- 3. the scenes
@pytest.mark.parametrize("scene,N,M", [("fold3", 50, 64), ("fold3", 50, 65), ("curl7", 128, 64), ("curl7", 128, 65)])
def test_scenes_report_the_first_colliding_sample_and_pair(scene, N, M):
    link, end = sc.SCENES[scene]
    D = len(link)
    c = ctx(*shape_argv(N, D))
    a = fitted(N, D, end)
    q = positions(c, a, np.linspace(0, 1, M, dtype=np.float32))
    rep = c.self_clearance(a[0], **FULL)
    rep = {k: np.asarray(v)[None] for k, v in rep.items()}
    _assert_report_consistent(rep, q, link, 0.0, (scene, M))
    g, x, _ = sc.self_clearance64(q[0], link)
    want = sc.summary64(g, x, D)
    count, first, which = sc.EXPECTED[(scene, M)]  # the exact line's; the fitted line's are the restatement's
    print(f"{scene} M={M}: restatement {want['n_crossing']} crossing from {want['first_colliding']} (exact line: {count} "
          f"from {first}); reported {int(rep['n_crossing'][0])} from {int(rep['first_colliding'][0])}")
    assert want["n_crossing"] > 0 and not rep["collision_free"][0]
    assert rep["first_colliding"][0] == want["first_colliding"] == rep["argmin_time"][0]
    assert (rep["argmin_time"][0], rep["argmin_link_a"][0], rep["argmin_link_b"][0]) == want["argmin"]
    assert rep["n_crossing"][0] == want["n_crossing"] == rep["n_colliding"][0]
    crossed = {sc.pairs(D)[k] for k in np.flatnonzero(rep["pair_clearance"][0] == 0.0)}
    assert crossed == {sc.pairs(D)[k] for k in np.flatnonzero(x.any(axis=0))}


def test_lim3_flips_its_verdict_with_the_link_radius():
    link, end = sc.SCENES["lim3"]
    c = ctx(*shape_argv(50, 3))
    a = fitted(50, 3, end)[0]
    q = positions(c, a[None], np.linspace(0, 1, 65, dtype=np.float32))
    g, x, _ = sc.self_clearance64(q[0], link)
    assert not x.any() and abs(g.min() - sc.LIM3_MIN_DISTANCE) < 16 * sc.tolerance(link, sc.max_angle(q)) + 5e-3
    thin, thick = c.self_clearance(a, link_radius=0.2), c.self_clearance(a, link_radius=0.3)
    assert thin["collision_free"] and thin["n_colliding"] == 0 and thin["min_clearance"] > 0
    assert not thick["collision_free"] and thick["n_colliding"] > 0 and thick["min_clearance"] < 0
    assert thick["n_crossing"] == 0 and (thick["argmin_link_a"], thick["argmin_link_b"]) == (0, 2)


# ------------------------------------------------- 4. batch independence, the _dev entry point, bounds
def test_batch_independence_and_optional_outputs():
    c = ctx(*shape_argv(128, 7))
    a = batch(128, 7, True)
    c.set_eval_times(eval_grid(300))
    k = 11
    full = c.self_clearance(a, link_radius=0.01, **FULL)
    one = c.self_clearance(a[k], link_radius=0.01, **FULL)
    assert set(full) == set(one) == {"min_clearance", "argmin_time", "argmin_link_a", "argmin_link_b", "n_colliding",
                                     "first_colliding", "collision_free", "n_crossing", "clearance", "pair_clearance",
                                     "joints"}
    for name in full:
        assert full[name].shape[0] == B
        np.testing.assert_array_equal(full[name][k], one[name], err_msg=name)
    bare = c.self_clearance(a, link_radius=0.01)
    assert set(bare) == set(full) - {"clearance", "pair_clearance", "joints"}
    for name in bare:
        np.testing.assert_array_equal(bare[name], full[name], err_msg=name)
    assert bare["collision_free"].dtype == bool


def test_dev_entry_point_gives_the_host_bits():
    import torch
    from irm_motion_planning_amd.clearance import IrmSelfClearanceReport
    N, D, M = 128, 7, 300
    c = ctx(*shape_argv(N, D))
    a = batch(N, D, True)
    c.set_eval_times(eval_grid(M))
    want = c.self_clearance(a, link_radius=0.02, **FULL)
    P = len(sc.pairs(D))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        a_t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        rep_t = torch.zeros((B, ctypes.sizeof(IrmSelfClearanceReport) // 4), dtype=torch.int32, device=dev)
        clear = torch.full((B, M), float("nan"), device=dev)
        pair = torch.full((B, P), float("nan"), device=dev)
        joints = torch.full((B, M, D, 2), float("nan"), device=dev)
        c.self_clearance_dev(a_t.data_ptr(), B, rep_t.data_ptr(), link_radius=0.02, clear_dev=clear.data_ptr(),
                             pair_dev=pair.data_ptr(), joints_dev=joints.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(clear.cpu().numpy(), want["clearance"])
    np.testing.assert_array_equal(pair.cpu().numpy(), want["pair_clearance"])
    np.testing.assert_array_equal(joints.cpu().numpy(), want["joints"])
    recs = rep_t.cpu().numpy()
    np.testing.assert_array_equal(recs[:, 0].view(np.float32), want["min_clearance"])
    for col, name in enumerate(("argmin_time", "argmin_link_a", "argmin_link_b", "n_colliding", "first_colliding"), 1):
        np.testing.assert_array_equal(recs[:, col], want[name], err_msg=name)
    np.testing.assert_array_equal(recs[:, 6].astype(bool), want["collision_free"])
    np.testing.assert_array_equal(recs[:, 7], want["n_crossing"])
    # the report alone, and a batch of none
    with torch.cuda.stream(stream):
        rep2 = torch.zeros_like(rep_t)
        c.self_clearance_dev(a_t.data_ptr(), B, rep2.data_ptr(), link_radius=0.02, stream=stream.cuda_stream)
        c.self_clearance_dev(0, 0, 0, stream=stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(rep2.cpu().numpy(), recs)


def test_the_largest_grid():
    from irm_motion_planning_amd import _abi
    M = _abi.IRM_MAX_EVAL_TIMES
    c = ctx(*shape_argv(50, 3))
    a = batch(50, 3, True)[:2]
    t = eval_grid(M)
    q = positions(c, a, t)
    rep = c.self_clearance(a, **FULL)
    check_values(rep, q, sc.LINKS3, ("largest grid", M))
    # a repeated time far behind its first occurrence: the lower index is reported
    i = int(rep["argmin_time"][0])
    t2 = np.concatenate((t, [t[i]])).astype(np.float32)[1:]
    c.set_eval_times(t2)
    again = c.self_clearance(a[0], with_samples=True)
    if i > 0:
        assert again["argmin_time"] == i - 1
        assert again["clearance"][-1] == again["clearance"][i - 1] == again["min_clearance"]


def test_error_paths():
    from conftest import params
    from irm_motion_planning_amd._abi import IrmError, c_float_p
    from irm_motion_planning_amd.clearance import IrmSelfClearanceReport
    from irm_motion_planning_amd.context import Context
    c = Context(params())
    a = np.zeros((50, 3), np.float32)
    with pytest.raises(IrmError, match="irm_self_clearance: no evaluation times"):
        c.self_clearance(a)
    with pytest.raises(IrmError, match="rank_self_clearance"):
        c.optimize_multistart(np.zeros(3, np.float32), np.ones(3, np.float32), np.zeros((0, 2), np.float32), 2,
                              rank_self_clearance=True)
    c.set_eval_times([0.25, 0.5])
    assert c.self_clearance(a)["argmin_time"] == 0
    empty = c.self_clearance(np.zeros((0, 50, 3), np.float32), **FULL)
    assert empty["clearance"].shape == (0, 2) and empty["pair_clearance"].shape == (0, 1)
    assert empty["min_clearance"].shape == (0,)
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(IrmError, match="irm_self_clearance: link_radius"):
            c.self_clearance(a, link_radius=bad)
    lib, h = c.lib, c._h
    p = lambda x: x.ctypes.data_as(c_float_p)  # noqa: E731
    rep = (IrmSelfClearanceReport * 2)()
    a2 = np.zeros((2, 50, 3), np.float32)
    for fn, tail in ((lib.irm_self_clearance, ()), (lib.irm_self_clearance_dev, (None,))):
        name = b"irm_self_clearance_dev:" if tail else b"irm_self_clearance:"
        for args, word in (((h, p(a2), 0.0, -1, rep), b"batch"), ((h, None, 0.0, 2, rep), b"alpha"),
                           ((h, p(a2), 0.0, 2, None), b"report"), ((h, p(a2), -1.0, 2, rep), b"link_radius")):
            assert fn(*args, None, None, None, *tail) == -22
            assert name in lib.irm_last_error() and word in lib.irm_last_error(), (args, lib.irm_last_error())
        assert fn(h, None, 0.0, 0, None, None, None, None, *tail) == 0  # batch = 0: a no-op
    c.close()


# ------------------------------------------------- 5. multi-start
def test_multistart_ranks_with_the_summed_counts():
    from test_gpu_multistart import B as MB, KW, S, call_ctx, run, scene
    c = call_ctx()
    start, goal, obs, radius, _, _ = scene("static")
    (alpha0, traj0, st0, info0), _, _ = run("static")
    # the flag off: today's call, to the bit
    off = c.optimize_multistart(start, goal, obs, S, rank_clearance=True, obstacle_radius=radius, link_radius=0.02,
                                candidates=True, rank_self_clearance=False, **KW)
    np.testing.assert_array_equal(off[0], alpha0)
    np.testing.assert_array_equal(off[1], traj0)
    assert set(off[3]) == set(info0)
    for name in ("winner", "rank", "alpha", "traj"):
        np.testing.assert_array_equal(off[3][name], info0[name], err_msg=name)
    for name in st0:
        np.testing.assert_array_equal(off[2][name], st0[name], err_msg=name)
    rows = np.arange(MB)
    # (capsules of radius 0.45 collide where link 2 comes within 0.9 of link 0: some candidates do, others do not)
    for with_obstacles, link_radius in ((True, 0.02), (False, 0.45), (True, 0.45)):
        kw = dict(rank_clearance=True, obstacle_radius=radius) if with_obstacles else {}
        alpha, traj, st, info = c.optimize_multistart(start, goal, obs, S, link_radius=link_radius, candidates=True,
                                                      rank_self_clearance=True, **kw, **KW)
        np.testing.assert_array_equal(info["alpha"], info0["alpha"])  # the candidates are the same plans
        cs = info["stats"]
        own = c.self_clearance(info["alpha"].reshape(MB * S, *info["alpha"].shape[2:]), link_radius=link_radius)
        np.testing.assert_array_equal(info["self_reports"]["n_colliding"], own["n_colliding"].reshape(MB, S))
        ncol = own["n_colliding"].reshape(MB, S) + (info["reports"]["n_colliding"] if with_obstacles else 0)
        want_w, want_r = mc.rank_lexsort(cs["constraints_ok"], cs["final_loss"], ncol)
        np.testing.assert_array_equal(info["winner"], want_w)
        np.testing.assert_array_equal(info["rank"], want_r)
        np.testing.assert_array_equal(alpha, info["alpha"][rows, want_w])
        np.testing.assert_array_equal(traj, info["traj"][rows, want_w])
        for name in st:
            np.testing.assert_array_equal(st[name], cs[name][rows, want_w], err_msg=name)
        print(f"obstacles={with_obstacles} r={link_radius}: self-colliding candidates "
              f"{int((own['n_colliding'] > 0).sum())} of {MB * S}, winners {info['winner'].tolist()} "
              f"(without the self check {info0['winner'].tolist()})")
    # without the candidate outputs: the same winner's rows; a single problem is un-batched
    a2, t2, st2, info2 = c.optimize_multistart(start, goal, obs, S, rank_clearance=True, obstacle_radius=radius,
                                               link_radius=0.45, rank_self_clearance=True, **KW)
    assert set(info2) == {"winner", "n_seeds", "rank", "self_reports"}
    np.testing.assert_array_equal(a2, alpha)
    np.testing.assert_array_equal(info2["winner"], info["winner"])
    a1, t1, st1, info1 = c.optimize_multistart(start[0], goal[0], obs[0], S, rank_clearance=True,
                                               obstacle_radius=radius[0], link_radius=0.45, rank_self_clearance=True, **KW)
    assert a1.shape == alpha.shape[1:] and np.ndim(info1["winner"]) == 0 and info1["rank"].shape == (S,)
    np.testing.assert_array_equal(a1, alpha[0])


# ------------------------------------------------- the CLI
GD20 = ["--optimizer-name", "gd", "--max-inner-iteration", "20"]


def test_cli_self_clearance(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(GD20)
    plain = capsys.readouterr().out
    assert "self-clearance" not in plain
    before = (tmp_path / "trajectory_result.txt").read_bytes()
    irm_main.main(GD20 + ["--clearance", "64", "--self-clearance", "65", "--link-radius", "0.05"])
    out = capsys.readouterr().out.splitlines()
    lines = [ln for ln in out if ln.startswith("self-clearance (65 samples): min ")]
    assert len(lines) == 1, out
    assert " at t=" in lines[0] and lines[0].count(" link ") == 2, lines[0]
    assert lines[0].endswith("collision-free") or " colliding samples (" in lines[0], lines[0]
    assert out.index(lines[0]) > [i for i, ln in enumerate(out) if ln.startswith("clearance (64 samples)")][0]
    assert (tmp_path / "trajectory_result.txt").read_bytes() == before
    skip = ("took", "setup object", "clearance", "self-clearance")
    keep = lambda ls: [ln for ln in ls if not ln.startswith(skip)]  # noqa: E731
    assert keep(out) == keep(plain.splitlines())
    # with --multi-start the candidates are ranked with the check as well
    irm_main.main(GD20 + ["--multi-start", "4", "--self-clearance", "65", "--link-radius", "0.05"])
    out = capsys.readouterr().out.splitlines()
    assert len([ln for ln in out if ln.startswith("self-clearance (65 samples): min ")]) == 1, out
    assert any(ln.startswith("multi-start: 4 seeds") and "collisions" in ln for ln in out), out


def test_cli_self_clearance_batch(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import batch_io, main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(GD20 + ["--batch-size", "8"])
    assert "self-clearance" not in capsys.readouterr().out
    files = {f: (tmp_path / f).read_bytes() for f in (batch_io.RESULT, batch_io.RESULT_BATCH, batch_io.SUMMARY_BATCH)}
    irm_main.main(GD20 + ["--batch-size", "8", "--self-clearance", "65", "--link-radius", "0.05"])
    out = capsys.readouterr().out.splitlines()
    assert len([ln for ln in out if ln.startswith("self-clearance (65 samples): min ")]) == 1, out
    tail = [ln for ln in out if ln.startswith("self-clearance: ")]
    assert len(tail) == 1 and tail[0].endswith(" problems that fulfil the constraints on the support grid self-collide"), out
    for f in (batch_io.RESULT, batch_io.RESULT_BATCH):
        assert (tmp_path / f).read_bytes() == files[f], f
    summary = (tmp_path / batch_io.SUMMARY_BATCH).read_text().splitlines()
    assert summary[0] == "# " + " ".join(batch_io.SUMMARY_COLUMNS) + " min_self_clearance"
    old = files[batch_io.SUMMARY_BATCH].decode().splitlines()
    assert len(summary) == len(old) == 9
    for new_row, old_row in zip(summary[1:], old[1:]):
        assert new_row.startswith(old_row + " ") and len(new_row.split()) == 7
        float(new_row.split()[-1])
