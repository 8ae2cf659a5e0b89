"""Fitting and re-timing (Context.fit_alpha / set_transfer / transfer_alpha, Replanner.advance, main.py
--coarse-n-timesteps) on an MI355X.

The arithmetic is stated, so it is checked against the numpy fp64 restatement of tests/fit_cases.py —
built from the library's own operators — to the rigorous bound of an fp64 sum in any order plus the one rounding to
fp32.  What the operators mean (the re-timed source trajectory; the waypoints that were fitted) is checked to twice
the reproduction error that restatement has on the same inputs, recorded by the CPU suite (fit_cases.TRANSFER_ERR /
FIT_ERR, tests/test_fit_host.py).  start_out, the batch, the _dev entry points and the replanner are bit for bit."""
import numpy as np
import pytest

import fit_cases as fc
from conftest import obstacles, params, ref_args

pytestmark = pytest.mark.gpu

_CTX = {}


def ctx(N, D):
    """One context per (N, D) for the module (N = 512 spends seconds in set-up)."""
    from irm_motion_planning_amd.context import Context
    if (N, D) not in _CTX:
        _CTX[(N, D)] = Context(params(*fc.shape_argv(N, D)))
    return _CTX[(N, D)]


def transfer(case, alpha_src=None, with_start=False):
    n_src, N, D, B, t0 = case
    c = ctx(N, D)
    c.set_transfer(n_src, t0=t0, t1=fc.T1)
    return c.transfer_alpha(fc.bump_alpha(n_src, D, B) if alpha_src is None else alpha_src, with_start=with_start)


def start_reference(case, alpha_src):
    """The source context's eval_any at the single time t0."""
    n_src, _, D, _, t0 = case
    src = ctx(n_src, D)
    src.set_eval_times([t0])
    return src.eval_any(alpha_src, 0)[:, 0, :]


def test_the_restatement_s_matrices_are_the_library_s():
    for N, D in ((50, 3), (128, 7)):
        for ours, theirs in zip(ctx(N, D).kernel_matrices(), fc.grid(N, D)):
            np.testing.assert_array_equal(ours, theirs)


# ------------------------------------------------- 1. arithmetic
@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_transfer_matches_restatement(case):
    r = fc.transfer_restatement(case)
    got = transfer(case)
    assert got.shape == (case[3], case[1], case[2]) and got.dtype == np.float32
    for b in range(case[3]):
        excess = np.abs(got[b].astype(np.float64) - r["ref"][b]) - r["bound"][b]
        assert (excess <= 0).all(), (b, float(excess.max()))


@pytest.mark.parametrize("N,D,B", fc.fit_grids())
@pytest.mark.parametrize("kind", ["bumps", "line"])
def test_fit_matches_restatement(N, D, B, kind):
    r = fc.fit_restatement(N, D, B, kind)
    c = ctx(N, D)
    alpha = fc.bump_alpha(N, D, B) if kind == "bumps" else fc.line_alpha(N, D, B)
    np.testing.assert_array_equal(c.evaluate(alpha, 0), r["Q"])  # the waypoints are the device's own
    got = c.fit_alpha(r["Q"])
    for b in range(B):
        excess = np.abs(got[b].astype(np.float64) - r["ref"][b]) - r["bound"][b]
        assert (excess <= 0).all(), (b, float(excess.max()))
    np.testing.assert_array_equal(c.fit_alpha(r["Q"][0]), got[0])  # a single trajectory drops the batch dimension


# ------------------------------------------------- 2. meaning
@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_transfer_is_the_source_trajectory_at_the_mapped_times(case):
    n_src, N, D, B, t0 = case
    a_src = fc.bump_alpha(n_src, D, B)
    got = transfer(case)
    src, dst = ctx(n_src, D), ctx(N, D)
    src.set_eval_times(fc.mapped_times(N, t0))
    pos_tol, vel_tol = (2 * x for x in fc.TRANSFER_ERR[fc.case_id(case)])
    pos = np.abs(dst.evaluate(got, 0).astype(np.float64) - src.eval_any(a_src, 0)).max()
    scale = float(np.float32(fc.T1) - np.float32(t0))
    vel = np.abs(dst.evaluate(got, 1).astype(np.float64) - scale * src.eval_any(a_src, 1).astype(np.float64)).max()
    print(f"{fc.case_id(case)}: positions {pos:.3e} (allowed {pos_tol:.3e}), velocities {vel:.3e} (allowed {vel_tol:.3e})")
    assert pos <= pos_tol and vel <= vel_tol


# ------------------------------------------------- 3. fit reproduces its waypoints
@pytest.mark.parametrize("N,D,B", fc.fit_grids())
def test_fit_reproduces_the_waypoints(N, D, B):
    c = ctx(N, D)
    for kind, tol in zip(("bumps", "line"), fc.FIT_ERR[(N, D)]):
        alpha = fc.bump_alpha(N, D, B) if kind == "bumps" else fc.line_alpha(N, D, B)
        Q = c.evaluate(alpha, 0)
        err = np.abs(c.evaluate(c.fit_alpha(Q), 0).astype(np.float64) - Q).max()
        print(f"N={N} D={D} {kind}: {err:.3e} (allowed {2 * tol:.3e})")
        assert err <= 2 * tol


def test_trajectory_fit_next_to_init_trajectory():
    from irm_motion_planning_amd.trajectory import Trajectory
    tr = Trajectory(ref_args(), context=ctx(50, 3))
    s, g = np.array([0.1, -0.2, 0.3], np.float32), np.array([1.2, 0.8, 0.3], np.float32)
    Q = tr.evaluate(tr.initTrajectory(s, g), tr.km, tr.jac)
    a = tr.fit(Q)
    np.testing.assert_array_equal(a, tr.context.fit_alpha(Q))
    assert np.abs(tr.evaluate(a, tr.km, tr.jac) - Q).max() <= 2 * fc.FIT_ERR[(50, 3)][1]
    assert np.abs(a).max() < 0.5 * np.abs(tr.initTrajectory(s, g)).max()  # the ridge keeps α small


# ------------------------------------------------- 4. start_out
@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_start_out_is_eval_any_at_t0(case):
    n_src, N, D, B, t0 = case
    a_src = fc.bump_alpha(n_src, D, B)
    alpha, start = transfer(case, with_start=True)
    assert start.shape == (B, D)
    np.testing.assert_array_equal(start, start_reference(case, a_src))
    np.testing.assert_array_equal(alpha, transfer(case))  # the same α with and without start_out
    a1, s1 = transfer(case, a_src[0], with_start=True)
    assert a1.shape == (N, D) and s1.shape == (D,)
    np.testing.assert_array_equal(s1, start[0])


# ------------------------------------------------- 5. batch independence
@pytest.mark.parametrize("case", [fc.CASES[0], fc.CASES[2], fc.CASES[4]], ids=fc.case_id)
def test_batch_independence(case):
    n_src, N, D, B, t0 = case
    assert B == 5
    a_src = fc.bump_alpha(n_src, D, B)
    full, start = transfer(case, with_start=True)
    c = ctx(N, D)
    Q = c.evaluate(fc.bump_alpha(N, D, B), 0)
    fit = c.fit_alpha(Q)
    for b in range(B):
        one, s1 = transfer(case, a_src[b:b + 1], with_start=True)
        np.testing.assert_array_equal(one[0], full[b])
        np.testing.assert_array_equal(s1[0], start[b])
        np.testing.assert_array_equal(c.fit_alpha(Q[b]), fit[b])
    # … nor on where in the batch it stands
    perm = np.array([3, 0, 4, 2, 1])
    np.testing.assert_array_equal(transfer(case, a_src[perm]), full[perm])


# ------------------------------------------------- 6. device-pointer entry points
@pytest.mark.parametrize("case", [fc.CASES[1], fc.CASES[2]], ids=fc.case_id)
def test_dev_entry_points_on_a_torch_stream(case):
    import torch
    n_src, N, D, B, t0 = case
    c = ctx(N, D)
    a_src = fc.bump_alpha(n_src, D, B)
    want, want_start = transfer(case, with_start=True)
    Q = c.evaluate(fc.bump_alpha(N, D, B), 0)
    want_fit = c.fit_alpha(Q)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        src = torch.from_numpy(a_src).to(dev)
        q = torch.from_numpy(Q).to(dev)
        out = torch.full((B, N, D), float("nan"), device=dev)
        out2 = torch.full((B, N, D), float("nan"), device=dev)
        fit = torch.full((B, N, D), float("nan"), device=dev)
        start = torch.full((B, D), float("nan"), device=dev)
        c.transfer_alpha_dev(src.data_ptr(), B, out.data_ptr(), start.data_ptr(), stream.cuda_stream)
        c.transfer_alpha_dev(src.data_ptr(), B, out2.data_ptr(), 0, stream.cuda_stream)
        c.fit_alpha_dev(q.data_ptr(), B, fit.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(out2.cpu().numpy(), want)
    np.testing.assert_array_equal(start.cpu().numpy(), want_start)
    np.testing.assert_array_equal(fit.cpu().numpy(), want_fit)


# ------------------------------------------------- 7. receding horizon
GD8 = ("--optimizer-name", "gd", "--max-outer-iteration", "1", "--max-inner-iteration", "8",
       "--loop-loss-reduction=-1e30", "--n-timesteps", "64")


def test_replanner_advance():
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args
    from irm_motion_planning_amd.replanning import Replanner
    args = ref_args(*GD8)
    B, tau = 5, 0.25
    rng = np.random.default_rng(31)
    s = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    g = rng.uniform(0.2, 1.6, (B, 3)).astype(np.float32)
    obs = obstacles()
    rp = Replanner(args, batch=B, n_obstacles=len(obs))
    rp.plan(obs, s, g)
    prev = rp.alpha_host()
    calls = []
    orig = rp.context.set_transfer
    rp.context.set_transfer = lambda *a, **k: (calls.append((a, k)), orig(*a, **k))[1]
    rp.advance(tau)
    rp.torch.cuda.synchronize()
    c = Context(params_from_args(args))
    c.set_transfer(64, t0=tau, t1=1.0)
    a_t, start = c.transfer_alpha(prev, with_start=True)
    c.set_eval_times([tau])
    np.testing.assert_array_equal(start, c.eval_any(prev, 0)[:, 0, :])
    np.testing.assert_array_equal(rp.start.cpu().numpy(), start)
    np.testing.assert_array_equal(rp.alpha_host(), a_t)
    obs2 = (obs + np.array([0.05, -0.03], np.float32)).astype(np.float32)
    st = rp.plan(obs2, warm_start=True)  # start: where the robot is; goal kept
    a_w, t_w, st_w = c.optimize(start, g, obs2, alpha0=a_t)
    np.testing.assert_array_equal(rp.alpha_host(), a_w)
    np.testing.assert_array_equal(rp.trajectory_host(), t_w)
    np.testing.assert_array_equal(st["grad_evals"], st_w["grad_evals"])
    # the operator is kept while tau stays the same
    rp.advance(tau)
    assert len(calls) == 1
    rp.advance(0.5)
    assert len(calls) == 2
    rp.torch.cuda.synchronize()


def test_replanner_advance_needs_a_plan():
    from irm_motion_planning_amd._abi import IrmError
    from irm_motion_planning_amd.replanning import Replanner
    rp = Replanner(ref_args(*GD8), batch=2, n_obstacles=3)
    with pytest.raises(IrmError):
        rp.advance(0.25)


# ------------------------------------------------- 8. coarse to fine
CLI = ["--optimizer-name", "gd", "--max-outer-iteration", "1", "--max-inner-iteration", "10", "--n-timesteps", "64"]


def test_cli_coarse_to_fine(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.environment import GOAL_CONFIG, OBSTACLES, START_CONFIG
    monkeypatch.chdir(tmp_path)
    alpha = irm_main.main(CLI + ["--coarse-n-timesteps", "32"])
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if ln.startswith("coarse stage, N = 32 :")]) == 1, out
    assert len([ln for ln in out.splitlines() if ln.startswith("fine stage, N = 64 :")]) == 1, out
    # the API path
    obs = OBSTACLES.astype(np.float32)
    fine, coarse = Context(params(*CLI)), Context(params(*(CLI[:-1] + ["32"])))
    a_c, _, _ = coarse.optimize(START_CONFIG, GOAL_CONFIG, obs)
    fine.set_transfer(32)
    a0 = fine.transfer_alpha(a_c)
    a_f, t_f, _ = fine.optimize(START_CONFIG, GOAL_CONFIG, obs, alpha0=a0)
    np.testing.assert_array_equal(alpha, a_f)
    assert np.abs(a_f - fine.optimize(START_CONFIG, GOAL_CONFIG, obs)[0]).max() > 0  # not the straight line's run
    np.testing.assert_array_equal(np.loadtxt(tmp_path / "trajectory_result.txt").astype(np.float32),
                                  fine.evaluate(a_f, 0))  # the output files are the fine stage's
    # the fine stage's α0 itself
    opt = irm_main.GradientDescentOptimizer(irm_main.parse_args(CLI + ["--coarse-n-timesteps", "32"]))
    opt.coarse_to_fine(irm_main.coarse_context(opt.args), START_CONFIG, GOAL_CONFIG)
    np.testing.assert_array_equal(opt.last_stages["fine"]["alpha0"][0], a0)
    np.testing.assert_array_equal(opt.last_stages["coarse"]["alpha"][0], a_c)


def test_cli_without_the_flag_is_unchanged(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    outs = []
    for name, extra in (("absent", []), ("zero", ["--coarse-n-timesteps", "0"])):
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        irm_main.main(CLI + extra)
        text = capsys.readouterr().out
        assert "stage, N =" not in text
        outs.append((d / "trajectory_result.txt").read_bytes())
    assert outs[0] == outs[1]


def test_cli_coarse_to_fine_batch(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(CLI + ["--coarse-n-timesteps", "32", "--batch-size", "6"])
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if ln.startswith("coarse stage, N = 32 :")]) == 1, out
    assert "of 6 , final loss mean" in out
    assert np.loadtxt(tmp_path / "trajectory_result.txt").shape == (64, 3)


# ------------------------------------------------- 9. errors
def test_errors():
    from irm_motion_planning_amd._abi import IrmError
    from irm_motion_planning_amd.context import Context
    c = Context(params(*fc.shape_argv(50, 3)))  # a context of its own: no transfer set yet
    a = fc.bump_alpha(50, 3, 5)
    with pytest.raises(IrmError, match="irm_set_transfer"):
        c.transfer_alpha(a)
    for bad in (1, 513, -2):
        with pytest.raises(IrmError, match="n_src"):
            c.set_transfer(bad)
    for t0, t1 in ((0.5, 0.5), (0.8, 0.1), (float("nan"), 1.0), (0.0, float("inf"))):
        with pytest.raises(IrmError):
            c.set_transfer(50, t0=t0, t1=t1)
    with pytest.raises(IrmError, match="irm_set_transfer"):  # a refused transfer sets nothing
        c.transfer_alpha(a)
    c.set_transfer(50)
    good = c.transfer_alpha(a)
    with pytest.raises(IrmError):  # alpha_src of another grid than the transfer's n_src
        c.transfer_alpha(fc.bump_alpha(32, 3, 5))
    for ridge in (1e-8, 0.0, -1.0, float("nan")):
        with pytest.raises(IrmError, match="rho"):
            c.set_fit_ridge(ridge)
    np.testing.assert_array_equal(c.transfer_alpha(a), good)  # a refused ridge keeps W and the transfer
    c.set_fit_ridge(1e-4)  # a new ridge rebuilds W and drops the transfer
    with pytest.raises(IrmError, match="irm_set_transfer"):
        c.transfer_alpha(a)
    c.set_transfer(50)
    assert np.abs(c.transfer_alpha(a) - good).max() > 0
    # batch 0 is a no-op
    assert c.transfer_alpha(np.zeros((0, 50, 3), np.float32)).shape == (0, 50, 3)
    assert c.fit_alpha(np.zeros((0, 50, 3), np.float32)).shape == (0, 50, 3)
