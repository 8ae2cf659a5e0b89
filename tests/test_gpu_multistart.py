"""Multi-start planning on an MI355X (Context.seed_ensemble / rank_candidates / optimize_multistart).

Every assertion is an identity: the seeds against the numpy twin of tests/multistart_cases.py and against fit_alpha /
init_alpha to the bit, the ranking against the twin's integers, and the call against the plain calls it is composed
of (optimize of the replicated problems from the seeds, clearance of those results, the twin's ranking of the
device's own stats).  Nothing depends on how a line search happens to end."""
import ctypes

import numpy as np
import pytest

import multistart_cases as mc
from conftest import obstacles
from test_gpu_dense import ctx, shape_argv

pytestmark = pytest.mark.gpu

f32 = np.float32
B3 = 3


def problems(D, B=B3, seed=21):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.9, 1.9, (B, D)).astype(f32), rng.uniform(-0.9, 1.9, (B, D)).astype(f32)


def bounds(c):
    p = c.params
    return mc.clamp_bounds(p.joint_safety_limit, p.min_joint_position, p.max_joint_position)


# ------------------------------------------------------------------ 1. seeds
@pytest.mark.parametrize("S", [1, 5, 64])
@pytest.mark.parametrize("N,D", [(33, 3), (64, 7), (130, 2)])
def test_seeds_are_the_twins_waypoints_and_their_fit(N, D, S):
    c = ctx(*shape_argv(N, D))
    start, goal = problems(D)
    t = c.kernel_matrices()[0]
    np.testing.assert_array_equal(t, mc.support_times(N))
    alpha, way = c.seed_ensemble(start, goal, S, seed=9, amplitude=1.0, with_waypoints=True)
    assert alpha.shape == way.shape == (B3, S, N, D)
    lo, hi = bounds(c)
    np.testing.assert_array_equal(way, mc.waypoints(start, goal, S, 9, 1.0, lo, hi, t))
    np.testing.assert_array_equal(alpha[:, 0], c.init_alpha(start, goal))
    if S > 1:
        fit = c.fit_alpha(way[:, 1:].reshape(-1, N, D)).reshape(B3, S - 1, N, D)
        np.testing.assert_array_equal(alpha[:, 1:], fit)
    np.testing.assert_array_equal(c.seed_ensemble(start, goal, S, seed=9, amplitude=1.0), alpha)  # without waypoints


def test_ensembles_nest_and_a_shard_reproduces_its_rows():
    c = ctx(*shape_argv(33, 3))
    start, goal = problems(3)
    a8, w8 = c.seed_ensemble(start, goal, 8, seed=4, amplitude=1.0, with_waypoints=True)
    a4, w4 = c.seed_ensemble(start, goal, 4, seed=4, amplitude=1.0, with_waypoints=True)
    np.testing.assert_array_equal(a8[:, :4], a4)
    np.testing.assert_array_equal(w8[:, :4], w4)
    a, w = c.seed_ensemble(start[1:], goal[1:], 8, seed=4, amplitude=1.0, problem_offset=1, with_waypoints=True)
    np.testing.assert_array_equal(a, a8[1:])
    np.testing.assert_array_equal(w, w8[1:])
    assert not np.array_equal(c.seed_ensemble(start[1:], goal[1:], 8, seed=4, amplitude=1.0), a8[1:])
    one = c.seed_ensemble(start[2], goal[2], 8, seed=4, amplitude=1.0, problem_offset=2)  # a single problem: (S, N, D)
    np.testing.assert_array_equal(one, a8[2])


def test_large_amplitude_is_clamped_and_zero_amplitude_is_the_clamped_line():
    c = ctx(*shape_argv(33, 3))
    start, goal = problems(3)
    t = c.kernel_matrices()[0]
    lo, hi = bounds(c)
    _, way = c.seed_ensemble(start, goal, 6, seed=0, amplitude=4.0, with_waypoints=True)
    np.testing.assert_array_equal(way, mc.waypoints(start, goal, 6, 0, 4.0, lo, hi, t))
    assert way[:, 1:].min() == lo and way[:, 1:].max() == hi
    _, way0 = c.seed_ensemble(start, goal, 3, seed=0, amplitude=0.0, with_waypoints=True)
    np.testing.assert_array_equal(way0, mc.waypoints(start, goal, 3, 0, 0.0, lo, hi, t))
    np.testing.assert_array_equal(way0[:, 1], np.clip(way0[:, 0], lo, hi))


# ------------------------------------------------------------------ 2. ranking
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 33, 64])
def test_ranking_equals_the_twin(S, B):
    c = ctx(*shape_argv(33, 3))
    for k, kind in enumerate(("random", "ties", "nan", "allfail", "classes")):
        ok, loss, ncol = mc.random_tables(np.random.default_rng(100 * S + 10 * B + k), B, S, kind)
        for reports in (None, {"n_colliding": ncol}, ncol.reshape(-1)):
            winner, rank = c.rank_candidates({"constraints_ok": ok.reshape(-1), "final_loss": loss.reshape(-1)}, reports,
                                             n_seeds=S)
            want_w, want_r = mc.rank_lexsort(ok, loss, None if reports is None else ncol)
            np.testing.assert_array_equal(rank, want_r, err_msg=f"{kind} {reports is not None}")
            np.testing.assert_array_equal(winner, want_w, err_msg=f"{kind} {reports is not None}")
    winner, rank = c.rank_candidates({"constraints_ok": ok, "final_loss": loss})  # (B, S) tables: n_seeds from the shape
    np.testing.assert_array_equal(rank, mc.rank_lexsort(ok, loss)[1])


# ------------------------------------------------------------------ 3. the call
N, D, B, S, M = 33, 3, 4, 6, 65
KW = dict(seed=3, amplitude=1.0)
_RUNS = {}


def call_ctx():
    c = ctx(*shape_argv(N, D))
    c.set_eval_times(np.linspace(0, 1, M, dtype=f32))
    return c


def scene(variant):
    """B problems with one obstacle table each (the reference scene's first five, shifted per problem), radii per
    problem; "moving": a velocity table; "goal_xy": end-effector targets instead of goal configurations."""
    rng = np.random.default_rng(8)
    start, goal = problems(D, B, seed=5)
    obs = (obstacles(5)[None] + rng.uniform(-0.2, 0.2, (B, 5, 2))).astype(f32)
    radius = rng.uniform(0.05, 0.15, (B, 5)).astype(f32)
    vel = rng.uniform(-0.3, 0.3, obs.shape).astype(f32) if variant == "moving" else None
    gxy = np.array([[1.0, 1.5], [0.5, 2.0], [-0.5, 1.8], [1.8, 0.9]], f32) if variant == "goal_xy" else None
    return start, goal, obs, radius, vel, gxy


def run(variant):
    """The multi-start call with every candidate output, and the plain calls it must equal — once per variant."""
    if variant in _RUNS:
        return _RUNS[variant]
    c = call_ctx()
    start, goal, obs, radius, vel, gxy = scene(variant)
    multi = c.optimize_multistart(start, None if gxy is not None else goal, obs, S, rank_clearance=True,
                                  obstacle_radius=radius, link_radius=0.02, obstacle_velocity=vel, goal_xy=gxy,
                                  candidates=True, **KW)
    if gxy is not None:
        goal = c.ik_seed(start, gxy)[0]
    seeds = c.seed_ensemble(start, goal, S, **KW).reshape(B * S, N, D)
    rep = lambda x: None if x is None else mc.replicate(x, S)  # noqa: E731
    plain = c.optimize(rep(start), rep(goal), rep(obs), alpha0=seeds, obstacle_velocity=rep(vel), goal_xy=rep(gxy))
    clear = c.clearance(plain[0], rep(obs), obstacle_velocity=rep(vel), obstacle_radius=rep(radius), link_radius=0.02)
    _RUNS[variant] = (multi, plain, clear)
    return _RUNS[variant]


VARIANTS = ["static", "moving", "goal_xy"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_candidate_is_the_plain_optimize_from_its_seed(variant):
    (alpha, traj, st, info), (p_alpha, p_traj, p_st), clear = run(variant)
    np.testing.assert_array_equal(info["alpha"].reshape(B * S, N, D), p_alpha)
    np.testing.assert_array_equal(info["traj"].reshape(B * S, N, D), p_traj)
    for name, vals in p_st.items():
        np.testing.assert_array_equal(info["stats"][name].reshape(-1), vals, err_msg=name)
    assert int(np.sum(p_st["inner_iterations"])) > 0
    for name, vals in clear.items():
        np.testing.assert_array_equal(info["reports"][name].reshape(-1), vals, err_msg=name)


@pytest.mark.parametrize("variant", VARIANTS)
def test_winner_is_the_twins_ranking_and_the_outputs_are_its_rows(variant):
    (alpha, traj, st, info), _, _ = run(variant)
    cs, cr = info["stats"], info["reports"]
    want_w, want_r = mc.rank_lexsort(cs["constraints_ok"], cs["final_loss"], cr["n_colliding"])
    np.testing.assert_array_equal(info["winner"], want_w)
    np.testing.assert_array_equal(info["rank"], want_r)
    rows = np.arange(B)
    np.testing.assert_array_equal(alpha, info["alpha"][rows, want_w])
    np.testing.assert_array_equal(traj, info["traj"][rows, want_w])
    for name, vals in st.items():
        np.testing.assert_array_equal(vals, cs[name][rows, want_w], err_msg=name)
    # the winner never ranks behind candidate 0, the plain call's result
    cls, loss = mc.keys(cs["constraints_ok"], cs["final_loss"], cr["n_colliding"])
    for b in range(B):
        w = int(want_w[b])
        assert (cls[b, w], loss[b, w], w) <= (cls[b, 0], loss[b, 0], 0), (b, w)


def test_without_candidate_outputs_and_without_clearance():
    c = call_ctx()
    start, goal, obs, radius, _, _ = scene("static")
    (alpha, traj, st, info), _, _ = run("static")
    a2, t2, st2, info2 = c.optimize_multistart(start, goal, obs, S, rank_clearance=True, obstacle_radius=radius,
                                               link_radius=0.02, **KW)
    assert set(info2) == {"winner", "n_seeds"}
    np.testing.assert_array_equal(info2["winner"], info["winner"])
    np.testing.assert_array_equal(a2, alpha)
    np.testing.assert_array_equal(t2, traj)
    a3, t3, st3, info3 = c.optimize_multistart(start, goal, obs, S, candidates=True, **KW)  # ranked without reports
    assert "reports" not in info3
    np.testing.assert_array_equal(info3["alpha"], info["alpha"])
    cs = info3["stats"]
    np.testing.assert_array_equal(info3["winner"], mc.rank_lexsort(cs["constraints_ok"], cs["final_loss"])[0])
    np.testing.assert_array_equal(a3, info3["alpha"][np.arange(B), info3["winner"]])


def test_shared_obstacle_table_and_single_problem():
    c = call_ctx()
    start, goal, _, _, _, _ = scene("static")
    obs = obstacles(5)
    alpha, traj, st, info = c.optimize_multistart(start, goal, obs, S, rank_clearance=True, obstacle_radius=0.1,
                                                  candidates=True, **KW)
    seeds = c.seed_ensemble(start, goal, S, **KW).reshape(B * S, N, D)
    p_alpha, p_traj, p_st = c.optimize(mc.replicate(start, S), mc.replicate(goal, S), obs, alpha0=seeds)
    np.testing.assert_array_equal(info["alpha"].reshape(B * S, N, D), p_alpha)
    clear = c.clearance(p_alpha, obs, obstacle_radius=0.1)
    np.testing.assert_array_equal(info["reports"]["n_colliding"].reshape(-1), clear["n_colliding"])
    a1, t1, st1, info1 = c.optimize_multistart(start[0], goal[0], obs, S, rank_clearance=True, obstacle_radius=0.1,
                                               candidates=True, **KW)
    assert a1.shape == (N, D) and info1["alpha"].shape == (S, N, D)
    np.testing.assert_array_equal(a1, alpha[0])
    assert int(info1["winner"]) == int(info["winner"][0])


@pytest.mark.parametrize("variant", ["static", "goal_xy"])
def test_one_seed_is_the_plain_call(variant):
    c = call_ctx()
    start, goal, obs, _, _, gxy = scene(variant)
    alpha, traj, st, info = c.optimize_multistart(start, None if gxy is not None else goal, obs, 1, goal_xy=gxy, **KW)
    if gxy is not None:
        goal = c.ik_seed(start, gxy)[0]
    p_alpha, p_traj, p_st = c.optimize(start, goal, obs, alpha0=c.init_alpha(start, goal), goal_xy=gxy)
    np.testing.assert_array_equal(alpha, p_alpha)
    np.testing.assert_array_equal(traj, p_traj)
    for name, vals in p_st.items():
        np.testing.assert_array_equal(st[name], vals, err_msg=name)
    np.testing.assert_array_equal(info["winner"], np.zeros(B, np.int32))


def test_dev_entry_point_with_a_caller_workspace_gives_the_host_bits():
    import torch
    from irm_motion_planning_amd.clearance import IrmClearanceReport
    from irm_motion_planning_amd.context import batch_dev
    c = call_ctx()
    start, goal, obs, radius, vel, _ = scene("moving")
    (alpha, traj, st, info), _, _ = run("moving")
    O = obs.shape[1]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    nbytes = c.multistart_workspace(B, S, O, 2 * O)
    assert nbytes > 0
    with torch.cuda.stream(stream):
        s_t, g_t, o_t, r_t, v_t = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (start, goal, obs, radius, vel))
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        a_out = torch.full((B, N, D), float("nan"), device=dev)
        t_out = torch.full((B, N, D), float("nan"), device=dev)
        st_out = torch.zeros((B, 8), dtype=torch.int32, device=dev)
        winner = torch.full((B,), -1, dtype=torch.int32, device=dev)
        rank = torch.full((B, S), -1, dtype=torch.int32, device=dev)
        c_alpha = torch.full((B, S, N, D), float("nan"), device=dev)
        c_rep = torch.zeros((B * S, ctypes.sizeof(IrmClearanceReport) // 4), dtype=torch.int32, device=dev)
        bd = batch_dev(start=s_t.data_ptr(), goal=g_t.data_ptr(), obstacles=o_t.data_ptr(), n_obstacles=O,
                       obstacle_stride=2 * O, batch=B, alpha_out=a_out.data_ptr(), traj_out=t_out.data_ptr(),
                       stats_out=st_out.data_ptr(), obstacle_velocity=v_t.data_ptr())
        c.optimize_multistart_dev(bd, S, winner.data_ptr(), ws.data_ptr(), nbytes, rank_clearance=True,
                                  obstacle_radius_dev=r_t.data_ptr(), link_radius=0.02, cand_alpha_dev=c_alpha.data_ptr(),
                                  cand_reports_dev=c_rep.data_ptr(), rank_dev=rank.data_ptr(),
                                  stream=stream.cuda_stream, **KW)
    stream.synchronize()
    np.testing.assert_array_equal(winner.cpu().numpy(), info["winner"])
    np.testing.assert_array_equal(rank.cpu().numpy(), info["rank"])
    np.testing.assert_array_equal(a_out.cpu().numpy(), alpha)
    np.testing.assert_array_equal(t_out.cpu().numpy(), traj)
    np.testing.assert_array_equal(c_alpha.cpu().numpy(), info["alpha"])
    np.testing.assert_array_equal(st_out.cpu().numpy()[:, 5], st["constraints_ok"])
    np.testing.assert_array_equal(st_out.cpu().numpy()[:, 7].view(f32), st["final_loss"])
    np.testing.assert_array_equal(c_rep.cpu().numpy()[:, 4], info["reports"]["n_colliding"].reshape(-1))
    with pytest.raises(Exception, match="workspace"):  # a workspace that is too small is refused before anything runs
        c.optimize_multistart_dev(bd, S, winner.data_ptr(), ws.data_ptr(), nbytes - 256, stream=stream.cuda_stream, **KW)


def test_refused_arguments_name_themselves():
    from irm_motion_planning_amd._abi import IrmError
    from irm_motion_planning_amd.via import ViaPoints
    c = call_ctx()
    start, goal, obs, radius, _, _ = scene("static")
    bare = ctx(*shape_argv(N, D), "--seed", "2")  # a context of its own, without an evaluation grid
    cases = [
        (bare, dict(n_seeds=S, rank_clearance=True), "rank_clearance"),
        (c, dict(n_seeds=S, obstacle_radius=radius), "obstacle_radius"),
        (c, dict(n_seeds=S, link_radius=0.05), "link_radius"),
        (c, dict(n_seeds=0), "n_seeds"),
        (c, dict(n_seeds=65), "n_seeds"),
        (c, dict(n_seeds=S, amplitude=-1.0), "amplitude"),
        (c, dict(n_seeds=S, amplitude=float("nan")), "amplitude"),
        (c, dict(n_seeds=S, problem_offset=-1), "problem_offset"),
        (c, dict(n_seeds=S, series=True), "series"),
        (c, dict(n_seeds=S, via=ViaPoints([5], [0], np.zeros((1, D), f32))), "via"),
    ]
    for cx, kw, word in cases:
        with pytest.raises(IrmError, match=word):
            cx.optimize_multistart(start, goal, obs, **kw)
    with pytest.raises(IrmError, match="n_seeds"):
        c.seed_ensemble(start, goal, 65)
    with pytest.raises(IrmError, match="amplitude"):
        c.seed_ensemble(start, goal, 4, amplitude=float("inf"))
    with pytest.raises(IrmError, match="goal"):
        c.optimize_multistart(start, None, obs, S)


# ------------------------------------------------------------------ 4. the CLI
GD20 = ["--optimizer-name", "gd", "--max-inner-iteration", "20", "--n-timesteps", "33"]


def test_cli_multi_start(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(GD20)
    plain = capsys.readouterr().out
    assert "multi-start" not in plain
    before = (tmp_path / "trajectory_result.txt").read_bytes()
    irm_main.main(GD20 + ["--multi-start", "1"])  # one seed: the plain run, to the byte
    out = capsys.readouterr().out.splitlines()
    assert (tmp_path / "trajectory_result.txt").read_bytes() == before
    assert [ln for ln in out if ln.startswith("multi-start:")] == \
        ["multi-start: 1 seeds, winner candidate 0 (ranked by constraints, loss)"], out
    skip = ("took", "setup object", "multi-start", "  candidate")
    keep = lambda ls: [ln for ln in ls if not ln.startswith(skip)]  # noqa: E731
    assert keep(out) == keep(plain.splitlines())
    irm_main.main(GD20 + ["--multi-start", "4", "--multi-start-amplitude", "0.8", "--multi-start-seed", "5",
                          "--clearance", "65", "--obstacle-radius", "0.1"])
    out = capsys.readouterr().out.splitlines()
    head = [ln for ln in out if ln.startswith("multi-start:")]
    assert len(head) == 1 and head[0].endswith("(ranked by constraints, collisions, loss)"), out
    rows = [ln for ln in out if ln.startswith("  candidate ")]
    assert len(rows) == 4 and all(", colliding samples " in ln for ln in rows), out
    assert sorted(int(ln.split(": rank ")[1].split(" ")[0]) for ln in rows) == [0, 1, 2, 3]
    winner = int(head[0].split("winner candidate ")[1].split(" ")[0])
    assert f"  candidate {winner} : rank 0 " in rows[winner]


def test_cli_multi_start_batch(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import batch_io, main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(GD20 + ["--batch-size", "6"])
    assert "multi-start" not in capsys.readouterr().out
    files = {f: (tmp_path / f).read_bytes() for f in (batch_io.RESULT, batch_io.RESULT_BATCH, batch_io.SUMMARY_BATCH)}
    irm_main.main(GD20 + ["--batch-size", "6", "--multi-start", "1"])
    capsys.readouterr()
    for f, old in files.items():
        assert (tmp_path / f).read_bytes() == old, f
    irm_main.main(GD20 + ["--batch-size", "6", "--multi-start", "3"])
    out = capsys.readouterr().out.splitlines()
    assert len([ln for ln in out if ln.startswith("  candidate ")]) == 3, out
    tail = [ln for ln in out if ln.startswith("multi-start: the winner is candidate 0 (the plain seed) in ")]
    assert len(tail) == 1 and tail[0].endswith(" of 6 problems"), out


# ------------------------------------------------------------------ 5. the nine-scene study (measured, not asserted)
def test_study_ensemble_is_never_behind_the_single_seed():
    """Nine scenes, one disc each; S = 12 seeds of amplitude 1.2 against the single seed (candidate 0 of the same call,
    which is the plain call to the bit).  The counts are printed (DESIGN.md §5 records them); the assertion is the one
    that holds by construction: a winner's key is never behind candidate 0's, so the winners that are both ok and
    collision-free are never fewer than the single seeds that are."""
    c = ctx(*shape_argv(mc.STUDY_N, 3), "--seed", "3")  # a context of its own: the study sets its own evaluation grid
    c.set_eval_times(np.linspace(0, 1, mc.STUDY_M, dtype=f32))
    nb = mc.STUDY_SCENES.shape[0]
    start = np.broadcast_to(mc.STUDY_START, (nb, 3))
    goal = np.broadcast_to(mc.STUDY_GOAL, (nb, 3))
    obs = mc.STUDY_SCENES[:, None, :]
    _, _, st, info = c.optimize_multistart(start, goal, obs, mc.STUDY_S, seed=mc.STUDY_SEED, amplitude=mc.STUDY_A,
                                           rank_clearance=True, obstacle_radius=mc.STUDY_RADIUS, candidates=True)
    cs, cr = info["stats"], info["reports"]
    single = mc.study_counts(cs["constraints_ok"][:, 0], cr["n_colliding"][:, 0])
    rows = np.arange(nb)
    multi = mc.study_counts(cs["constraints_ok"][rows, info["winner"]], cr["n_colliding"][rows, info["winner"]])
    free = (cr["n_colliding"] == 0).sum(axis=1)
    print(f"study: single seed collision-free {single[0]}/9, ok and free {single[1]}/9; S=12 winners collision-free "
          f"{multi[0]}/9, ok and free {multi[1]}/9; collision-free candidates per scene {free.tolist()}; "
          f"winners {info['winner'].tolist()}")
    assert multi[1] >= single[1]
