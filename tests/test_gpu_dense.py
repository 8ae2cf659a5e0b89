"""Evaluation and checks at arbitrary times (Context.set_eval_times / eval_any / dense_check) on an MI355X.

The arithmetic of the evaluation is stated, so it is checked to the bit: on the support times against the
existing irm_evaluate path, elsewhere against a numpy restatement (fp64 sum of the exact fp32 products in the
order m = 0..N−1, one rounding, then ·J the same way) of the query matrices irm_query_matrices builds.  The
report is recomputed from the call's own samples; the per-sample obstacle cost is compared with the oracle's
compute_cost_vg on an fp64 FK of the device's own positions (rtol 1e-5, SURVEY.md §8c's cost tolerance; the
CPU suite — tests/test_dense_host.py — confirms the fp32 oracle itself stays inside that band here)."""
import numpy as np
import pytest

from conftest import GOAL, START, obstacles, params

pytestmark = pytest.mark.gpu

_CTX = {}


def ctx(*argv, **overrides):
    from irm_motion_planning_amd.context import Context
    key = (tuple(str(a) for a in argv), tuple(sorted(overrides.items())))
    if key not in _CTX:
        _CTX[key] = Context(params(*argv, **overrides))
    return _CTX[key]


def shape_argv(N, D):
    argv = ["--n-timesteps", str(N), "--n-joints", str(D)]
    if D != 3:
        argv += ["--link-length"] + [str(3.0 / D)] * D
    return argv


def query_matrices(N, t_eval, var=0.1):
    from irm_motion_planning_amd._abi import c_float_p, check, load_library
    t = np.ascontiguousarray(t_eval, np.float32)
    kq = np.zeros((t.shape[0], N), np.float32)
    dkq = np.zeros_like(kq)
    check(load_library().irm_query_matrices(N, var, t.ctypes.data_as(c_float_p), t.shape[0],
                                            kq.ctypes.data_as(c_float_p), dkq.ctypes.data_as(c_float_p)))
    return kq, dkq


def restate(Mq, alpha, J):
    """fp32(fp32(Mq·α)·J): fp64 accumulation of the exact fp32×fp32 products in the order m = 0, 1, …, one
    rounding to fp32, then ·J the same way (an fp64 product of two fp32 values is exact, so `acc += a * b` is
    the device's FMA chain bit for bit)."""
    f64 = np.float64
    acc = np.zeros((Mq.shape[0], alpha.shape[1]), f64)
    for m in range(alpha.shape[0]):
        acc += Mq[:, m, None].astype(f64) * alpha[m].astype(f64)
    T = acc.astype(np.float32)
    acc = np.zeros_like(acc)
    for d in range(J.shape[0]):
        acc += T[:, d, None].astype(f64) * J[d].astype(f64)
    return acc.astype(np.float32)


def eval_grid(M, seed=3):
    """M unsorted times in [−0.1, 1.1]."""
    return np.random.default_rng(seed).uniform(-0.1, 1.1, M).astype(np.float32)


def cost_inputs():
    """The inputs of test_gpu_parity.test_batched_cost_grad_matches_oracle."""
    rng = np.random.default_rng(7)
    a = (rng.standard_normal((37, 50, 3)) * 0.2).astype(np.float32)
    return a, obstacles()


def fk64(q, link, joint=None):
    """robot.py:29-36 (joint None) / 39-72 (fk_joint_j) in fp64: 2×M."""
    j = len(link) if joint is None else joint
    c = np.cumsum(np.asarray(q, np.float64)[:, :j], axis=1)
    ll = np.asarray(link, np.float64)[:j]
    return np.stack((ll @ np.cos(c).T, ll @ np.sin(c).T))


def cost64(q, link, obs, whole=False):
    """Per-sample obstacle cost: the oracle's compute_cost_vg on the fp64 FK of q (whole robot: summed over the
    joint positions)."""
    from oracle.oracle import compute_cost_vg
    if not whole:
        return compute_cost_vg(fk64(q, link), obs)[0].astype(np.float64)
    return sum(compute_cost_vg(fk64(q, link, j), obs)[0].astype(np.float64) for j in range(1, len(link) + 1))


# ------------------------------------------------- 1. support times: the existing path, bit for bit
@pytest.mark.parametrize("N,D", [(50, 3), (128, 3), (128, 7), (512, 3)])
def test_support_times_reproduce_evaluate(N, D):
    c = ctx(*shape_argv(N, D))
    rng = np.random.default_rng(11)
    B = 5
    s = rng.uniform(-0.5, 0.5, (B, D)).astype(np.float32)
    g = rng.uniform(0.2, 1.6, (B, D)).astype(np.float32)
    a0 = c.init_alpha(s, g)
    assert np.abs(a0).max() > 10.0  # the singular solve's large α
    small = (rng.standard_normal((B, N, D)) * 0.2).astype(np.float32)
    c.set_eval_times(c.kernel_matrices()[0])
    np.testing.assert_array_equal(c.eval_times(), c.kernel_matrices()[0])
    for a in (a0, small):
        for w in (0, 1):
            got = c.eval_any(a, w)
            assert got.shape == (B, N, D)
            np.testing.assert_array_equal(got, c.evaluate(a, w))


# ------------------------------------------------- 2. arbitrary times against the stated arithmetic
@pytest.mark.parametrize("N,D,M", [(50, 3, 1), (50, 3, 63), (50, 3, 64), (50, 3, 65), (50, 3, 300), (50, 3, 4096),
                                   (128, 7, 65), (128, 7, 300)])
def test_arbitrary_times_match_restatement(N, D, M):
    c = ctx(*shape_argv(N, D))
    J = c.kernel_matrices()[3]
    t = eval_grid(M)
    kq, dkq = query_matrices(N, t)
    rng = np.random.default_rng(5)
    B = 3
    a = (rng.standard_normal((B, N, D)) * 0.2).astype(np.float32)
    a[1] = c.init_alpha(rng.uniform(-0.5, 0.5, D).astype(np.float32), rng.uniform(0.2, 1.6, D).astype(np.float32))
    c.set_eval_times(t)
    np.testing.assert_array_equal(c.eval_times(), t)
    q, v = c.eval_any(a, 0), c.eval_any(a, 1)
    assert q.shape == v.shape == (B, M, D)
    for b in range(B):
        np.testing.assert_array_equal(q[b], restate(kq, a[b], J))
        np.testing.assert_array_equal(v[b], restate(dkq, a[b], J))
    # a single trajectory drops the batch dimension
    np.testing.assert_array_equal(c.eval_any(a[2], 1), v[2])


# ------------------------------------------------- 3. batch independence
def test_batch_independence():
    c = ctx()
    a, obs = cost_inputs()
    B, k = a.shape[0], 17
    assert B == 37
    c.set_eval_times(eval_grid(300))
    for w in (0, 1):
        np.testing.assert_array_equal(c.eval_any(a, w)[k], c.eval_any(a[k], w))
    full, one = c.dense_check(a, obs, with_cost=True), c.dense_check(a[k], obs, with_cost=True)
    assert set(full) == set(one) == {"max_cost", "avg_cost", "argmax_cost", "max_position", "min_position",
                                     "max_abs_velocity", "argmax_abs_velocity", "position_ok", "velocity_ok", "cost"}
    for name in full:
        assert full[name].shape[0] == B
        np.testing.assert_array_equal(full[name][k], one[name], err_msg=name)
    # one obstacle table per problem, every table the shared one: what the shared table gives
    per = c.dense_check(a, np.broadcast_to(obs, (B,) + obs.shape), with_cost=True)
    for name in full:
        np.testing.assert_array_equal(per[name], full[name], err_msg=name)
    # ... and tables that differ are the problems' own
    tables = np.ascontiguousarray(np.broadcast_to(obs, (B,) + obs.shape)).copy()
    tables[k] += np.float32(0.25)
    moved = c.dense_check(a, tables, with_cost=True)
    np.testing.assert_array_equal(moved["cost"][k], c.dense_check(a[k], tables[k], with_cost=True)["cost"])
    np.testing.assert_array_equal(np.delete(moved["cost"], k, 0), np.delete(full["cost"], k, 0))
    assert not np.array_equal(moved["cost"][k], full["cost"][k])


# ------------------------------------------------- 4. report self-consistency
def _check_report(c, a, obs, pmax=2.0, pmin=-1.0, vmax=7.0):
    rep = c.dense_check(a, obs, with_cost=True)
    q, v = c.eval_any(a, 0), c.eval_any(a, 1)
    if a.ndim == 2:
        rep, q, v = {k: np.asarray(x)[None] for k, x in rep.items()}, q[None], v[None]
    f32 = np.float32
    for b in range(q.shape[0]):
        cost = rep["cost"][b]
        assert rep["max_cost"][b] == cost.max() and rep["argmax_cost"][b] == int(np.argmax(cost))
        assert rep["max_position"][b] == q[b].max() and rep["min_position"][b] == q[b].min()
        va = np.abs(v[b]).max(axis=1)
        assert rep["max_abs_velocity"][b] == va.max() and rep["argmax_abs_velocity"][b] == int(np.argmax(va))
        assert bool(rep["position_ok"][b]) == bool(q[b].max() <= f32(pmax) and q[b].min() >= f32(pmin))
        assert bool(rep["velocity_ok"][b]) == bool(va.max() <= f32(vmax))
        mean = cost.astype(np.float64).mean()
        print(f"[{b}] avg_cost {rep['avg_cost'][b]:.8g} (fp64 mean {mean:.8g})")
        assert abs(float(rep["avg_cost"][b]) - mean) <= 1e-5 * abs(mean)
    return rep


@pytest.mark.parametrize("N,D,M", [(50, 3, 300), (50, 3, 65), (128, 7, 300)])
def test_report_is_consistent_with_its_samples(N, D, M):
    c = ctx(*shape_argv(N, D))
    rng = np.random.default_rng(13)
    a = (rng.standard_normal((6, N, D)) * 0.2).astype(np.float32)
    a[0] = c.init_alpha(rng.uniform(-0.5, 0.5, D).astype(np.float32), rng.uniform(0.2, 1.6, D).astype(np.float32))
    c.set_eval_times(eval_grid(M, seed=M))
    _check_report(c, a, obstacles())
    _check_report(c, a[3], obstacles(3))


def test_report_ties_go_to_the_lower_index():
    """A repeated time gives two identical samples: whichever attains a maximum, the lower index is reported."""
    c = ctx()
    a, obs = cost_inputs()
    t = eval_grid(130)
    c.set_eval_times(t)
    base = c.dense_check(a[:4], obs)
    for b in range(4):
        # repeat this problem's maximising times far behind (another wave, another chunk) and in front
        i, j = int(base["argmax_cost"][b]), int(base["argmax_abs_velocity"][b])
        t2 = np.concatenate(([t[j]], t, np.full(200, t[3], np.float32), [t[i], t[j], t[i]])).astype(np.float32)
        assert t2.shape[0] > 256 and np.sum(t2 == t[i]) >= 3 and np.sum(t2 == t[j]) >= 3
        c.set_eval_times(t2)
        rep = _check_report(c, a[b], obs)
        assert int(rep["argmax_cost"][0]) == int(np.flatnonzero(t2 == t[i])[0]) <= i + 1
        assert int(rep["argmax_abs_velocity"][0]) == 0
        assert rep["cost"][0][i + 1] == rep["cost"][0][-1] == rep["cost"][0][-3] == rep["max_cost"][0]


def test_lowered_limits_turn_their_flag_only():
    """--max-joint-velocity / --max-joint-position below the sampled maximum: that flag turns false, the other
    stays true (robot.py:104-113 on the M samples)."""
    a = ctx().init_alpha(START, GOAL)
    t = np.linspace(0, 1, 333, dtype=np.float32)
    ctx().set_eval_times(t)
    rep = _check_report(ctx(), a, obstacles())
    assert rep["position_ok"][0] and rep["velocity_ok"][0], rep
    vlow = f"{0.9 * float(rep['max_abs_velocity'][0]):.4f}"
    plow = f"{0.9 * float(rep['max_position'][0]):.4f}"
    cv = ctx("--max-joint-velocity", vlow)
    cv.set_eval_times(t)
    r = _check_report(cv, a, obstacles(), vmax=float(vlow))
    assert not r["velocity_ok"][0] and r["position_ok"][0]
    cp = ctx("--max-joint-position", plow)
    cp.set_eval_times(t)
    r = _check_report(cp, a, obstacles(), pmax=float(plow))
    assert not r["position_ok"][0] and r["velocity_ok"][0]
    for name in ("max_cost", "avg_cost", "argmax_cost", "max_position", "min_position", "max_abs_velocity",
                 "argmax_abs_velocity"):  # the limits change the verdicts only
        assert r[name][0] == rep[name][0], name


# ------------------------------------------------- 5. cost samples against fp64
@pytest.mark.parametrize("whole", [False, True])
def test_cost_samples_match_fp64_fk(whole):
    """Per-sample cost vs compute_cost_vg on the fp64 FK of the device's own positions, rtol 1e-5."""
    c = ctx("--whole-robot-cost", "true") if whole else ctx()
    a, obs = cost_inputs()
    c.set_eval_times(eval_grid(300))
    cost = c.dense_check(a, obs, with_cost=True)["cost"]
    q = c.eval_any(a, 0)
    link = [1.5, 1.0, 0.5]
    worst = 0.0
    for b in range(0, 37, 6):
        ref = cost64(q[b], link, obs, whole)
        worst = max(worst, float(np.max(np.abs(cost[b] - ref) / np.abs(ref))))
        np.testing.assert_allclose(cost[b], ref, rtol=1e-5, atol=0)
    print(f"whole={whole}: worst relative cost error {worst:.2e}")


def test_support_grid_report_matches_eval_cost():
    c = ctx()
    a, obs = cost_inputs()
    c.set_eval_times(c.kernel_matrices()[0])
    rep = c.dense_check(a, obs)
    np.testing.assert_allclose(rep["max_cost"], c.eval_cost(a, obs, START, GOAL, 0, 0, 1), rtol=1e-5, atol=0)
    np.testing.assert_allclose(rep["avg_cost"], c.eval_cost(a, obs, START, GOAL, 0, 0, 0), rtol=1e-5, atol=0)
    # no obstacles: zero cost everywhere, the first sample is the maximum
    none = c.dense_check(a[:2], np.zeros((0, 2), np.float32), with_cost=True)
    assert not none["cost"].any() and not none["max_cost"].any() and not none["argmax_cost"].any()


# ------------------------------------------------- 6. error paths and the drop-in
def test_error_paths():
    from irm_motion_planning_amd._abi import IrmError
    from irm_motion_planning_amd.context import Context
    c = Context(params())
    a = np.zeros((50, 3), np.float32)
    assert c.eval_times().shape == (0,)
    with pytest.raises(IrmError, match="irm_eval_any"):
        c.eval_any(a)
    with pytest.raises(IrmError, match="irm_dense_check"):
        c.dense_check(a, obstacles())
    for bad in (np.zeros(0), np.zeros(4097), [0.1, np.nan], [np.inf]):
        with pytest.raises(IrmError, match="irm_set_eval_times"):
            c.set_eval_times(bad)
    assert c.eval_times().shape == (0,)  # a rejected grid sets nothing
    c.set_eval_times([0.5, 0.25])
    c.set_eval_times([0.75])  # replaces the previous grid
    np.testing.assert_array_equal(c.eval_times(), np.array([0.75], np.float32))
    assert c.eval_any(a).shape == (1, 3)
    assert c.eval_any(np.zeros((0, 50, 3), np.float32)).shape == (0, 1, 3)  # batch 0 is a no-op
    with pytest.raises(IrmError):  # what irm_optimize_batch rejects: more than IRM_MAX_OBSTACLES
        c.dense_check(a, np.zeros((65, 2), np.float32))
    with pytest.raises(ValueError):
        c.dense_check(a[None], np.zeros((2, 3, 2), np.float32))  # per-problem tables of another batch
    c.close()


def test_trajectory_eval_any_drop_in():
    from irm_motion_planning_amd.trajectory import Trajectory, d_rbf_kernel, rbf_kernel
    from conftest import ref_args
    tr = Trajectory(ref_args())
    c = tr.context
    alpha = tr.initTrajectory(START, GOAL)
    x = eval_grid(77)
    got = tr.eval_any(alpha, rbf_kernel, tr.t, x, tr.jac)
    np.testing.assert_array_equal(c.eval_times(), x)
    np.testing.assert_array_equal(got, c.eval_any(alpha, 0))
    np.testing.assert_array_equal(tr.eval_any(alpha, d_rbf_kernel, tr.t.copy(), x, tr.jac.copy()), c.eval_any(alpha, 1))
    # eval_x = t is evaluate
    np.testing.assert_array_equal(tr.eval_any(alpha, rbf_kernel, tr.t, tr.t, tr.jac), tr.evaluate(alpha, tr.km, tr.jac))
    np.testing.assert_array_equal(tr.eval_any(alpha, d_rbf_kernel, tr.t, tr.t, tr.jac),
                                  tr.evaluate(alpha, tr.dkm, tr.jac))
    with pytest.raises(ValueError):
        tr.eval_any(alpha, rbf_kernel, np.linspace(0, 2, 50, dtype=np.float32), x, tr.jac)
    with pytest.raises(ValueError):
        tr.eval_any(alpha, rbf_kernel, tr.t, x, np.eye(3, dtype=np.float32))
    with pytest.raises(ValueError):
        tr.eval_any(alpha, np.exp, tr.t, x, tr.jac)


def test_trajectory_eval_any_uploads_only_a_new_grid(monkeypatch):
    from irm_motion_planning_amd.trajectory import Trajectory, rbf_kernel
    from conftest import ref_args
    tr = Trajectory(ref_args())
    alpha = tr.initTrajectory(START, GOAL)
    calls = []
    orig = tr.context.set_eval_times
    monkeypatch.setattr(tr.context, "set_eval_times", lambda t: (calls.append(len(t)), orig(t))[1])
    x = eval_grid(40)
    tr.eval_any(alpha, rbf_kernel, tr.t, x, tr.jac)
    tr.eval_any(alpha, rbf_kernel, tr.t, x.copy(), tr.jac)
    assert calls == [40]
    tr.eval_any(alpha, rbf_kernel, tr.t, x[:39], tr.jac)
    assert calls == [40, 39]


# ------------------------------------------------- 7. CLI
def test_cli_dense_check(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(["--optimizer-name", "gd", "--max-inner-iteration", "20", "--dense-check", "200"])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("dense check (200 samples): max cost ")]
    assert len(lines) == 1, out
    assert " at t=" in lines[0] and "; joint limit " in lines[0] and "; velocity limit " in lines[0], lines[0]
    dense = np.loadtxt(tmp_path / "trajectory_result_dense.txt")
    grid = np.loadtxt(tmp_path / "trajectory_result.txt")
    assert dense.shape == (200, 3) and grid.shape == (50, 3)
    np.testing.assert_array_equal(dense[0], grid[0])
    np.testing.assert_array_equal(dense[-1], grid[-1])


def test_cli_dense_check_batch(tmp_path, monkeypatch, capsys):
    from irm_motion_planning_amd import main as irm_main
    monkeypatch.chdir(tmp_path)
    irm_main.main(["--optimizer-name", "gd", "--max-inner-iteration", "20", "--batch-size", "6", "--dense-check", "120"])
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if ln.startswith("dense check (120 samples): max cost ")]) == 1, out
    tail = [ln for ln in out.splitlines() if ln.startswith("dense check: ")]
    assert len(tail) == 1 and " problems that fulfil the constraints on the support grid " in tail[0], out
    assert np.loadtxt(tmp_path / "trajectory_result_dense.txt").shape == (120, 3)
