"""The GD single loop's issue order (k_lean, LF_GD1) against the untouched dual-loop kernel.

A launch that records a series runs LF_GD2, which on the single loop (--max-outer-iteration 1) does
the same arithmetic as LF_GD1 (test_gpu_parity.py::test_lean_flows_agree_on_the_single_loop).  LF_GD1
of C3's kernel issues its LDS reads in another order than LF_GD2 does — the flag word ahead of stage
1's operands at the round top, staged waits on them, the α update's G words with the decision's
records — so a read that moved ahead of the write it depends on, or an MFMA ahead of its operand's
arrival, shows up here as a mismatch: α, the trajectory and
every statistic must agree bit for bit.  Each case is the smallest shape at which its path can go
wrong (several workgroups, a partial one, finished trajectories beside live ones, both stage-1 forms,
both obstacle loops, the kernels the change must not reach)."""
import numpy as np
import pytest

from conftest import params

pytestmark = pytest.mark.gpu

STATS = ("grad_evals", "cost_evals", "inner_iterations", "outer_iterations", "constraints_ok", "final_loss")
FORCED = "--loop-loss-reduction=-1e30"  # every iteration runs
_CTX, _C3, _RUN = {}, [], {}


def ctx(*argv, **overrides):
    from irm_motion_planning_amd.context import Context
    key = (argv, tuple(sorted(overrides.items())))
    if key not in _CTX:
        _CTX[key] = Context(params("--optimizer-name", "gd", "--max-outer-iteration", "1", *argv, **overrides))
    return _CTX[key]


def c3_problems(B):
    """The first B problems of the C3 bench line, and its obstacles."""
    if not _C3:
        import bench
        _C3.append(bench.make_problem("c3", 1, 0))
    s, g, obs = _C3[0]
    return s[:B], g[:B], obs


def random_problems(B, D=3, seed=41):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (B, D)).astype(np.float32), rng.uniform(0.2, 1.6, (B, D)).astype(np.float32)


def many_obstacles(n):
    """n obstacles: the reference set and shifted copies of it (n = 0: none)."""
    from irm_motion_planning_amd.environment import OBSTACLES
    reps = -(-max(n, 1) // len(OBSTACLES))
    return np.concatenate([OBSTACLES + 0.1 * i for i in range(reps)])[:n].astype(np.float32).reshape(n, 2)


def both_flows(c, s, g, obs, iters=None):
    """The plain launch (LF_GD1) and the series launch (LF_GD2) of the same problems, compared bit for bit."""
    B = len(s)
    p1, p2 = c.launch_plan(B, len(obs)), c.launch_plan(B, len(obs), series=True)
    assert p1["lean"] == 1 and p1["kernel"].endswith(",GD1>"), p1
    assert p2["lean"] == 1 and p2["kernel"].endswith(",GD2>"), p2
    a1, t1, st1 = c.optimize(s, g, obs)
    a2, t2, st2, _ = c.optimize(s, g, obs, series=True)
    assert np.all(np.isfinite(t1))
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(t1, t2)
    for k in STATS:
        np.testing.assert_array_equal(st1[k], st2[k], err_msg=k)
    if iters is not None:
        assert np.all(st1["grad_evals"] == iters), st1["grad_evals"]
    return p1, (a1, t1, st1)


def c3_forced():
    """C3's own inputs, 200 forced iterations, four trajectories per 512-thread workgroup (run once)."""
    if "c3" not in _RUN:
        s, g, obs = c3_problems(32)
        c = ctx("--n-timesteps", "128", "--max-inner-iteration", "200", FORCED, traj_per_block=4)
        _RUN["c3"] = (c, both_flows(c, s, g, obs, 200))
    return _RUN["c3"]


def test_c3_inputs_forced_iterations():
    """32 of the bench line's problems: eight workgroups of the kernel the bench line times; sparse and
    dense stage-1 rounds both occur on these inputs."""
    _, (pl, _) = c3_forced()
    assert pl["kernel"] == "k_lean<FixShape<3,128,32>,512,1,FULL,GD1>" and pl["traj_per_block"] == 4, pl


def test_c3_inputs_default_loss_reduction():
    """The reference's stopping rule: the trajectories of a workgroup finish in different rounds, so a done
    slot's stale e' and G columns sit beside live ones."""
    s, g, obs = c3_problems(32)
    c = ctx("--n-timesteps", "128", "--max-inner-iteration", "200", traj_per_block=4)
    pl, (_, _, st) = both_flows(c, s, g, obs)
    assert pl["kernel"] == "k_lean<FixShape<3,128,32>,512,1,FULL,GD1>", pl
    assert len(np.unique(st["grad_evals"])) > 1, st["grad_evals"]  # they do stop at different rounds


def test_partial_last_workgroup():
    s, g, obs = c3_problems(13)
    c = ctx("--n-timesteps", "128", "--max-inner-iteration", "200", FORCED, traj_per_block=4)
    pl, _ = both_flows(c, s, g, obs, 200)
    assert pl["traj_per_block"] == 4 and pl["grid"] == 4, pl


@pytest.mark.parametrize("B", [12, 256, 258])
def test_two_trajectories_per_workgroup(B):
    """Both launch forms: a batch of at most half the CUs in workgroups is padded to 512 threads
    (choose_shape), a larger one runs the 256-thread kernel.  On the MI355X's 256 CUs B = 256 is the
    largest padded batch (128 workgroups) and B = 258 the smallest unpadded one."""
    s, g = random_problems(B)
    _, _, obs = c3_problems(1)
    c = ctx("--n-timesteps", "128", "--max-inner-iteration", "20", FORCED, traj_per_block=2)
    pl, _ = both_flows(c, s, g, obs, 20)
    padded = 2 * pl["grid"] <= c.info()["num_cus"]
    assert pl["traj_per_block"] == 2 and pl["grid"] == (B + 1) // 2 and pl["threads"] == (512 if padded else 256), pl
    assert padded == (B <= 256), pl  # the cases above do cover both forms


@pytest.mark.parametrize("N", [50, 64])
def test_one_wave_per_trajectory(N):
    """N ≤ 64: one wave per trajectory (G read with the direction there)."""
    s, g = random_problems(12)
    _, _, obs = c3_problems(1)
    c = ctx("--n-timesteps", str(N), "--max-inner-iteration", "20", FORCED)
    both_flows(c, s, g, obs, 20)


@pytest.mark.parametrize("O", [0, 50])
def test_obstacle_counts(O):
    """No obstacle and 50 of them: the obstacle loop over LDS instead of the register table."""
    s, g = random_problems(8)
    c = ctx("--n-timesteps", "128", "--max-inner-iteration", "20", FORCED)
    both_flows(c, s, g, many_obstacles(O), 20)


def test_repeat_launch_is_bit_equal():
    c, (_, ref) = c3_forced()
    s, g, obs = c3_problems(32)
    a, t, st = c.optimize(s, g, obs)
    np.testing.assert_array_equal(a, ref[0])
    np.testing.assert_array_equal(t, ref[1])
    for k in STATS:
        np.testing.assert_array_equal(st[k], ref[2][k], err_msg=k)
