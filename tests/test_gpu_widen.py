"""SURVEY.md §8f rows on the GPU: batched CLI + output files (row 2) and dynamic
environments with warm-started re-planning (row 4), against the CPU oracle.

Tolerances: a few GD steps from the same α0 agree with the oracle's fp32 α-space
iteration within 2e-3 in waypoint space (smoke() / test_gd_steps use the same band);
HIP-vs-HIP comparisons of the same launch configuration are bit-exact.
"""
import os

import numpy as np
import pytest

from conftest import GOAL, START, obstacles, oracle_for, ref_args

pytestmark = pytest.mark.gpu

GD20 = ("--optimizer-name", "gd", "--max-outer-iteration", "1", "--max-inner-iteration", "20",
        "--loop-loss-reduction=-1e30")


def _oracle_traj(orc, alpha0, obs, s, g):
    a, st = orc.optimize(alpha0, obs, s, g)
    return orc.evaluate(a), st


def test_main_cli_batch_mode(tmp_path, capsys):
    """--batch-size B: problem 0 keeps the reference files, the batch files hold every problem,
    each problem's trajectory matches the oracle run of the same start/goal."""
    from irm_motion_planning_amd import batch_io
    from irm_motion_planning_amd import main as irm_main
    B = 12
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        irm_main.main(list(GD20) + ["--batch-size", str(B), "--seed", "3", "--extended-vis", "true",
                                    "--n-measurements", "2"])
    finally:
        os.chdir(cwd)
    out = capsys.readouterr().out
    assert "batch of 12 problems" in out and "result cost: ( avg" in out and "runtimes in ms: mean" in out
    res0 = np.loadtxt(tmp_path / batch_io.RESULT)
    allr = batch_io.read_result_batch(tmp_path / batch_io.RESULT_BATCH, 50, 3)
    assert res0.shape == (50, 3) and allr.shape == (B, 50, 3)
    np.testing.assert_array_equal(res0, allr[0])
    ser0 = np.loadtxt(tmp_path / batch_io.SERIES)
    frames = batch_io.read_series_batch(tmp_path / batch_io.SERIES_BATCH)
    assert len(frames) == B and ser0.shape == (21, 150)  # frame 0 + 20 accepted steps
    np.testing.assert_array_equal(ser0.reshape(-1, 50, 3).astype(np.float32), frames[0])
    for b in range(B):
        np.testing.assert_array_equal(frames[b][-1], allr[b].astype(np.float32))
    summ = np.loadtxt(tmp_path / batch_io.SUMMARY_BATCH)
    assert summ.shape == (B, 6) and np.all(summ[:, 5] == 20)
    s, g = batch_io.batch_problems(B, 3, 3)
    orc = oracle_for(*GD20)
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args
    c = Context(params_from_args(ref_args(*GD20)))
    for b in (0, 5, B - 1):
        # the oracle from the α0 the CLI started from (the device's initTrajectory, bit-equal to
        # irm_init_alpha; the oracle's own fp32 LU solve of the singular K gives another α0)
        a0 = c.init_alpha(s[b], g[b])
        t_o, st_o = _oracle_traj(orc, a0, obstacles(), s[b], g[b])
        assert np.abs(allr[b] - t_o).max() < 2e-3, b
        assert abs(summ[b, 0] - orc.cost(orc.optimize(a0, obstacles(), s[b], g[b])[0],
                                          obstacles(), s[b], g[b], 0, 0, 0)) < 1e-3


def _moved(obs, k):
    """The reference obstacles drifting by k·(0.05, −0.03)."""
    return (obs + np.float32(k) * np.array([0.05, -0.03], np.float32)).astype(np.float32)


def test_replanner_cold_and_warm_equal_host_entry_point():
    """Cold plan == irm_optimize_batch; warm plan == irm_optimize_batch(alpha0 = previous α)."""
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args
    from irm_motion_planning_amd.replanning import Replanner
    args = ref_args(*GD20)
    B = 40
    rng = np.random.default_rng(21)
    s = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    g = rng.uniform(0.2, 1.6, (B, 3)).astype(np.float32)
    rp = Replanner(args, batch=B, n_obstacles=11)
    c = Context(params_from_args(args))
    obs0 = obstacles()
    st0 = rp.plan(obs0, s, g)
    a_h, t_h, st_h = c.optimize(s, g, obs0)
    np.testing.assert_array_equal(rp.alpha_host(), a_h)
    np.testing.assert_array_equal(rp.trajectory_host(), t_h)
    np.testing.assert_array_equal(st0["grad_evals"], st_h["grad_evals"])
    prev = a_h
    for k in (1, 2, 3):
        obs_k = _moved(obs0, k)
        rp.plan(obs_k)  # warm start, start/goal kept
        a_w, t_w, _ = c.optimize(s, g, obs_k, alpha0=prev)
        np.testing.assert_array_equal(rp.alpha_host(), a_w)
        np.testing.assert_array_equal(rp.trajectory_host(), t_w)
        prev = a_w
    # warm_start=False is the cold plan of the current environment
    rp.plan(obs0, warm_start=False)
    np.testing.assert_array_equal(rp.trajectory_host(), t_h)


def test_replanner_warm_start_matches_oracle():
    """A warm-started plan is the reference iteration started from the previous α."""
    from irm_motion_planning_amd.replanning import Replanner
    args = ref_args(*GD20)
    B = 6
    rng = np.random.default_rng(5)
    s = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    g = rng.uniform(0.2, 1.6, (B, 3)).astype(np.float32)
    rp = Replanner(args, batch=B, n_obstacles=11)
    orc = oracle_for(*GD20)
    obs0 = obstacles()
    rp.plan(obs0, s, g)
    prev = rp.alpha_host()
    obs1 = _moved(obs0, 4)
    st = rp.plan(obs1)
    traj = rp.trajectory_host()
    for b in range(B):
        t_o, st_o = _oracle_traj(orc, prev[b], obs1, s[b], g[b])
        assert np.abs(traj[b] - t_o).max() < 2e-3, b
        assert int(st["grad_evals"][b]) == st_o["grad_evals"] == 20


def test_replanner_per_problem_obstacles():
    """Each problem its own (moving) obstacle set: equals the shared-environment run of that
    problem alone (batch independence, summation-tile tolerance as test_batch_equals_single)."""
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args
    from irm_motion_planning_amd.replanning import Replanner
    args = ref_args(*GD20)
    B, O = 5, 7
    rng = np.random.default_rng(8)
    s = rng.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    g = rng.uniform(0.2, 1.6, (B, 3)).astype(np.float32)
    obs = rng.uniform(-3, 3, (B, O, 2)).astype(np.float32)
    rp = Replanner(args, batch=B, n_obstacles=O, per_problem_obstacles=True)
    rp.plan(obs, s, g)
    c = Context(params_from_args(args))
    prev = rp.alpha_host()
    obs2 = (obs + 0.1).astype(np.float32)
    rp.plan(obs2)
    traj = rp.trajectory_host()
    for b in range(B):
        _, t1, _ = c.optimize(s[b], g[b], obs2[b], alpha0=prev[b])
        np.testing.assert_allclose(traj[b], t1, rtol=0, atol=1e-4)


# ------------------------------------------------ whole-robot obstacle cost (§8f row 3)

@pytest.fixture(scope="module")
def g_wr():
    from conftest import golden
    return golden("ref_whole_robot_n50")


def _wr_ctx(*argv):
    from irm_motion_planning_amd.context import Context
    from conftest import params
    return Context(params(*argv, whole_robot_cost=1))


def test_fk_joints_match_reference(g_wr):
    """k_fk_joints == Robot.fk_joint_1..3 of the reference (golden) and the oracle."""
    from irm_motion_planning_amd.context import Context
    from conftest import params
    c = Context(params())
    o = oracle_for()
    for name in ("alpha0", "small1", "small2"):
        tr = g_wr[f"traj_{name}"]
        pos = c.fk_joints(tr)
        assert pos.shape == (3, 2, 50)
        np.testing.assert_allclose(pos, g_wr[f"fkj_{name}"], rtol=0, atol=2e-6)
        for j in (1, 2, 3):
            np.testing.assert_allclose(pos[j - 1], o.fk_joint(tr, j), rtol=0, atol=2e-6)
        np.testing.assert_allclose(pos[2], c.fk(tr), rtol=0, atol=1e-6)  # fk_joint_D = fk
    from irm_motion_planning_amd.robot import Robot
    rob = Robot(ref_args(), c)
    np.testing.assert_array_equal(rob.fk_joint_2(g_wr["traj_small1"]), c.fk_joints(g_wr["traj_small1"])[1])


@pytest.mark.parametrize("name", ["small1", "small2", "alpha0"])
def test_whole_robot_cost_and_grad(g_wr, g_eval, name):
    """Host-API cost / gradient with whole_robot_cost = 1: vs the reference composition (golden,
    bands of tests/test_oracle_golden.py) and vs the oracle on the same α (tight)."""
    c = _wr_ctx()
    o = oracle_for(whole_robot_cost=1)
    _, K, _, J = o.kernel_matrices()
    a, obs = g_eval[name], g_wr["obstacles"]
    rtol, gtol = (2e-3, 5e-3) if name == "alpha0" else (1e-5, 2e-4)
    for i, lm in enumerate(g_wr["lmax"]):
        lm = float(lm)
        cost = c.eval_cost(a, obs, START, GOAL, 0, 0, lm)
        ref = float(g_wr[f"loss_{name}"][i])
        assert abs(cost - ref) <= rtol * abs(ref), (lm, cost, ref)
        assert abs(cost - o.cost(a, obs, START, GOAL, 0, 0, lm)) <= 2e-6 * abs(ref)
        G = c.eval_cost_grad(a, obs, START, GOAL, 0, 0, lm)
        Gref = K.T.astype(np.float64) @ g_wr[f"grad_{name}"][i].astype(np.float64) @ J.T.astype(np.float64)
        assert np.abs(G - Gref).max() <= gtol * np.abs(Gref).max(), lm
        Go = o.cost_g(a, obs, START, GOAL, 0, 0, lm)
        assert np.abs(G - Go).max() <= 1e-5 * np.abs(Go).max(), lm
    # full loss with penalties (λsg, λjl) on top of the whole-robot obstacle term
    for lam in ((0.5, 0.1, 0.5), (50, 10, 0)):
        ref = o.cost(a, obs, START, GOAL, *lam)
        assert abs(c.eval_cost(a, obs, START, GOAL, *lam) - ref) <= 1e-5 * abs(ref)


@pytest.mark.parametrize("lmax", ["0.0", "0.5"])
def test_whole_robot_gd_steps_match_oracle(lmax):
    """20 GD steps of the whole-robot loss: HIP optimiser vs oracle α-space iteration.

    λmax = 0: 2e-3 (the smoke / GD-step band).  λmax = 0.5: the max term's first-index argmax
    over the summed per-waypoint cost meets near-ties (problem 1, step 2: waypoints 33 / 32
    differ by 7e-6 in a cost of 6.44, far below the 1e-4 waypoint noise of either fp32
    iteration), so a step may weight a neighbouring waypoint: 5e-2 on waypoints (the band of
    test_bench_mode_vs_exact for λmax > 0) and 1e-3 relative on the final loss."""
    argv = GD20 + ("--lambda-max-cost", lmax)
    c = _wr_ctx(*argv)
    o = oracle_for(*argv, whole_robot_cost=1)
    rng = np.random.default_rng(17)
    s = np.vstack([START, rng.uniform(-0.5, 0.5, (5, 3))]).astype(np.float32)
    g = np.vstack([GOAL, rng.uniform(0.2, 1.6, (5, 3))]).astype(np.float32)
    _, traj, st = c.optimize(s, g, obstacles())
    tol = 2e-3 if float(lmax) == 0 else 5e-2
    for b in range(len(s)):
        t_o, st_o = _oracle_traj(o, o.init_alpha(s[b], g[b]), obstacles(), s[b], g[b])
        assert np.abs(traj[b] - t_o).max() < tol, b
        assert abs(float(st["final_loss"][b]) - st_o["final_loss"]) < 1e-3 * abs(st_o["final_loss"])


def test_whole_robot_bls_end_to_end():
    """Reference control flow (BLS, defaults) on the whole-robot loss: constraints met, the
    whole-robot obstacle cost in the oracle's band and below that of the end-effector plan."""
    c = _wr_ctx()
    o = oracle_for(whole_robot_cost=1)
    obs = obstacles()
    alpha, traj, st = c.optimize(START, GOAL, obs)
    avg = c.eval_cost(alpha, obs, START, GOAL, 0, 0, 0)
    a_o, st_o = o.optimize(o.init_alpha(START, GOAL), obs, START, GOAL)
    avg_o = o.cost(a_o, obs, START, GOAL, 0, 0, 0)
    assert bool(st["constraints_ok"]) and st_o["constraints_ok"]
    assert abs(avg - avg_o) < 0.05, (avg, avg_o)
    from irm_motion_planning_amd.context import Context
    from conftest import params
    c_ee = Context(params())
    a_ee, _, _ = c_ee.optimize(START, GOAL, obs)
    assert avg < c.eval_cost(a_ee, obs, START, GOAL, 0, 0, 0)


def test_main_cli_two_ranks_sharded(tmp_path):
    """torchrun, 2 ranks (sharing the box's one GPU, host-side gloo collectives): the sharded
    batch run writes the same batch files as the single-process run (per-problem results are
    independent of batch neighbours up to summation-tile differences, 1e-4)."""
    import subprocess
    import sys
    from irm_motion_planning_amd import batch_io
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = list(GD20) + ["--batch-size", "9", "--seed", "5"]
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir()
    d2.mkdir()
    env = dict(os.environ, PYTHONPATH=repo, IRM_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    subprocess.run([sys.executable, "-m", "irm_motion_planning_amd.main"] + argv, cwd=d1, env=env, check=True,
                   timeout=300)
    port = 29500 + os.getpid() % 1000
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), "-m",
                    "irm_motion_planning_amd.main"] + argv, cwd=d2, env=env, check=True, timeout=300)
    a = batch_io.read_result_batch(d1 / batch_io.RESULT_BATCH, 50, 3)
    b = batch_io.read_result_batch(d2 / batch_io.RESULT_BATCH, 50, 3)
    assert a.shape == b.shape == (9, 50, 3)
    np.testing.assert_allclose(b, a, rtol=0, atol=1e-4)
    sa, sb = np.loadtxt(d1 / batch_io.SUMMARY_BATCH), np.loadtxt(d2 / batch_io.SUMMARY_BATCH)
    np.testing.assert_array_equal(sa[:, 2:], sb[:, 2:])  # flags and iteration counts


def test_bench_gpus_flag_runs_ranks():
    """`bench.py --gpus 2` outside torchrun launches two ranks itself and reports n_gpus = 2 with the
    whole job's iterations (the ranks share the box's one GPU, gloo collectives on host tensors); the
    CPU baseline (`--full`) is kept on rank 0 at every world size."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
                        "--steps", "2", "--warmup", "1", "--max-inner", "20", "--full"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, env=env, timeout=300, cwd=repo)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["n_gpus"] == 2 and r["config"]["global_batch"] == 2048
    assert r["iterations_per_step"] == 2 * 1024 * 20
    assert r["value"] > 0 and r["cpu_baseline"]["value"] > 0


def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps, measures no CPU baseline and,
    with --dump-outputs, writes what the last timed step left in the caller's buffers: bit for bit the
    arrays the same library computes for the same (seeded) problems in this process."""
    import json
    import subprocess
    import sys
    import bench
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--max-inner", "20", "--dump-outputs", str(tmp_path / "out")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, env=env, timeout=300, cwd=repo)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["steps"] == 2 and r["cpu_baseline"] is None
    assert r["iterations_per_step"] == 1024 * 20
    assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] * 1e-3 - 1024 * 20) < 1e-6 * 1024 * 20
    alpha, traj, stats = (np.load(tmp_path / "out" / (n + ".npy")) for n in ("alpha", "traj", "stats"))
    assert alpha.dtype == traj.dtype == np.float32 and stats.dtype == np.float64
    assert alpha.shape == traj.shape == (1024, 128, 3) and stats.shape == (1024, 8)
    s, g, obs = bench.make_problem("c3", 1, 0)
    a_here, t_here, st = Context(params_from_args(bench.make_args("c3", False, 20))).optimize(s, g, obs)
    np.testing.assert_array_equal(alpha, a_here)
    np.testing.assert_array_equal(traj, t_here)
    np.testing.assert_array_equal(stats[:, 2], np.asarray(st["grad_evals"], np.float64))
    np.testing.assert_array_equal(stats[:, 7].astype(np.float32), np.asarray(st["final_loss"], np.float32))
