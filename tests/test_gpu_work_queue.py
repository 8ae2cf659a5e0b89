"""The work queue of optimize() (irm_set_work_queue): a fixed number of persistent workgroups whose
finished slots claim the next problem.

A problem's α, trajectory and statistics do not depend on what shares its workgroup (DESIGN.md §4,
test_gpu_parity.py::test_result_independent_of_workgroup_neighbours), so every comparison here is
bit for bit: the same Context, the same inputs, the queue off and on.  Problems are the bench's
(bench.make_problem / bench.make_args(cfg, True, …): the faithful flows, whose problems end after
very different numbers of rounds).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CTX = {}
_TB = {}
BENCH_B = 1024  # the batch at which the bench's trajectories-per-workgroup is taken


def _args(cfg, opt=None, argv=(), faithful=True, max_inner=200):
    """The bench's argument namespace of `cfg` (faithful flow), optionally with another optimiser or,
    for cfg "n50", the CLI's own N = 50 shape; `argv` overrides single flags."""
    import bench
    from irm_motion_planning_amd import main as irm_main
    if cfg == "n50":
        args = irm_main.parse_args(["--optimizer-name", opt or "bls", "--n-timesteps", "50"] + list(argv))
        return args
    args = bench.make_args(cfg, faithful, max_inner)
    if opt:
        args.optimizer_name = opt
    if argv:
        over = irm_main.parse_args(list(argv))
        for flag in argv:
            if flag.startswith("--"):
                name = flag[2:].split("=")[0].replace("-", "_")
                setattr(args, name, getattr(over, name))
    return args


def _ctx(cfg, opt=None, argv=(), faithful=True, tb="bench", **over):
    """One Context per configuration, at the bench's trajectories per workgroup (what a B = 1,024 launch
    of the same configuration runs with traj_per_block = 0)."""
    from irm_motion_planning_amd.context import Context
    from irm_motion_planning_amd.params import params_from_args
    key = (cfg, opt, tuple(argv), faithful, tb, tuple(sorted(over.items())))
    if key not in _CTX:
        args = _args(cfg, opt, argv, faithful)
        if tb == "bench":
            tkey = (cfg, opt, tuple(argv), faithful, tuple(sorted(over.items())))
            if tkey not in _TB:
                probe = Context(params_from_args(args, **over))
                _TB[tkey] = probe.launch_plan(BENCH_B, 11)["traj_per_block"]
                probe.close()
            tb = _TB[tkey]
        _CTX[key] = Context(params_from_args(args, traj_per_block=tb, **over))
    return _CTX[key]


def _problems(cfg, lo, hi):
    import bench
    s, g, obs = bench.make_problem("c3" if cfg == "n50" else cfg, 1, 0)
    return s[lo:hi], g[lo:hi], obs


def _same(res, ref, what=""):
    """α, trajectory and every irm_stats field, bit for bit."""
    np.testing.assert_array_equal(res[0], ref[0], err_msg=f"alpha {what}")
    np.testing.assert_array_equal(res[1], ref[1], err_msg=f"trajectory {what}")
    assert set(res[2]) == set(ref[2])
    for k in ref[2]:
        np.testing.assert_array_equal(res[2][k], ref[2][k], err_msg=f"stats.{k} {what}")


def _off_on(c, groups, s, g, obs, expect_groups=None, **kw):
    """optimize() with the queue off, then with `groups`; returns (off, on) and leaves the queue off."""
    O = obs.shape[-2]
    B = len(s)
    c.set_work_queue(0)
    assert c.work_queue_groups(B, O) == 0
    off = c.optimize(s, g, obs, **kw)
    c.set_work_queue(groups)
    try:
        if expect_groups is not None:
            assert c.work_queue_groups(B, O) == expect_groups
            if B > 0:
                plan = c.launch_plan(B, O)
                if expect_groups:
                    assert plan["grid"] == expect_groups and "QUEUE" in plan["kernel"], plan
                else:
                    assert "QUEUE" not in plan["kernel"], plan
        on = c.optimize(s, g, obs, **kw)
    finally:
        c.set_work_queue(0)
    return off, on


REFILL = [("c3bls", None), ("c3", None), ("c3n64", None), ("c3n64", "bls"), ("n50", "bls"), ("c7", None), ("c7", "bls")]


@pytest.mark.parametrize("cfg,opt", REFILL, ids=[f"{c}-{o or 'cfg'}" for c, o in REFILL])
def test_refill_uneven_lengths(cfg, opt):
    """37 problems on 2 persistent workgroups: 37 is no multiple of the trajectories per workgroup, so the
    static first assignment and the tail (claims ≥ B) both run, and every slot serves several problems.
    The slice of the seeded problems is the first whose inner-iteration counts (queue off) differ by at
    least 2× between the shortest and the longest problem."""
    c = _ctx(cfg, opt)
    c.set_work_queue(0)
    B = 37
    chosen = None
    for lo in range(0, 8 * B, B):
        s, g, obs = _problems(cfg, lo, lo + B)
        it = c.optimize(s, g, obs)[2]["inner_iterations"]
        print(f"{cfg}/{opt}: problems {lo}..{lo + B - 1}: inner_iterations min {it.min()} max {it.max()}")
        if it.max() >= 2 * max(int(it.min()), 1):
            chosen = (s, g, obs)
            break
    assert chosen is not None, "no seeded slice of 37 problems with a 2x spread of inner iterations"
    s, g, obs = chosen
    off, on = _off_on(c, 2, s, g, obs, expect_groups=2)
    _same(on, off, f"{cfg}/{opt}")


def test_simultaneous_claims():
    """Eight copies of one problem finish in the same round of one workgroup and must claim distinct
    indices (G = 1: every claim of the launch comes from this workgroup)."""
    c = _ctx("c3bls")
    s, g, obs = _problems("c3bls", 0, 17)
    s = np.concatenate([np.repeat(s[5:6], 8, 0), s[:5], s[6:13]])
    g = np.concatenate([np.repeat(g[5:6], 8, 0), g[:5], g[6:13]])
    assert len(s) == 20
    off, on = _off_on(c, 1, s, g, obs, expect_groups=1)
    _same(on, off)
    for b in range(1, 8):
        np.testing.assert_array_equal(on[0][b], on[0][0])
        np.testing.assert_array_equal(on[1][b], on[1][0])
        for k in on[2]:
            assert on[2][k][b] == on[2][k][0], k


@pytest.mark.parametrize("cfg", ["c3bls", "c3"])
@pytest.mark.parametrize("O", [11, 5])
def test_per_problem_obstacles(cfg, O):
    """(B, O, 2) tables that differ per problem: O = 11 is held in registers where the flow does that
    (obs_reg), O = 5 is read from LDS; a loaded problem brings its own table."""
    c = _ctx(cfg)
    B = 21
    s, g, obs = _problems(cfg, 100, 100 + B)
    rng = np.random.default_rng(11)
    tables = (obs[None, :O] + rng.uniform(-0.15, 0.15, (B, O, 2))).astype(np.float32)
    off, on = _off_on(c, 2, s, g, tables, expect_groups=2)
    _same(on, off, f"{cfg} O={O}")
    assert len({tuple(t.ravel()) for t in tables}) == B


@pytest.mark.parametrize("cfg", ["c3bls", "c3"])
def test_warm_start(cfg):
    """alpha0 given (init_alpha plus a seeded 1e-3 perturbation) and alpha0 = None."""
    c = _ctx(cfg)
    B = 21
    s, g, obs = _problems(cfg, 200, 200 + B)
    a0 = c.init_alpha(s, g)
    a0 = (a0 + 1e-3 * np.random.default_rng(5).standard_normal(a0.shape)).astype(np.float32)
    off, on = _off_on(c, 2, s, g, obs, expect_groups=2, alpha0=a0)
    _same(on, off, "alpha0 given")
    off0, on0 = _off_on(c, 2, s, g, obs, expect_groups=2)
    _same(on0, off0, "alpha0 None")
    assert not np.array_equal(off[0], off0[0])


@pytest.mark.parametrize("cfg,argv", [("c3bls", ("--max-outer-iteration=0",)), ("c3bls", ("--max-inner-iteration=0",)),
                                      ("c3", ("--max-inner-iteration=0",))])
def test_problems_that_end_in_their_load_round(cfg, argv):
    """BLS with no outer iteration returns α0 (optimizer_BLS.py:184-186, 210-213); an empty inner loop
    goes straight to the constraint check: the load round's own decision."""
    c = _ctx(cfg, argv=argv)
    B = 19
    s, g, obs = _problems(cfg, 300, 300 + B)
    off, on = _off_on(c, 2, s, g, obs, expect_groups=2)
    _same(on, off, f"{cfg} {argv}")
    assert np.all(off[2]["inner_iterations"] == 0)


def test_degenerate_sizes():
    """Requests that cover every workgroup of the static launch run the static launch."""
    c = _ctx("c3bls")
    for B, G in [(1, 1), (3, 4), (0, 2), (37, 10 ** 6)]:
        s, g, obs = _problems("c3bls", 0, B)
        off, on = _off_on(c, G, s, g, obs, expect_groups=0)
        _same(on, off, f"B={B} G={G}")
    from irm_motion_planning_amd._abi import IrmError
    with pytest.raises(IrmError):
        c.set_work_queue(-2)
    c.set_work_queue(0)


def test_launch_sequence_on_one_context():
    """Queued, queued, off, queued: the counter is set per launch and set_work_queue(0) restores the
    static launch; auto at B = 37 (fewer workgroups than the GPU holds) is the static launch."""
    c = _ctx("c3bls")
    s, g, obs = _problems("c3bls", 400, 437)
    c.set_work_queue(0)
    ref = c.optimize(s, g, obs)
    try:
        for groups, expect in [(2, 2), (3, 3), (0, 0), (2, 2), ("auto", 0), ("off", 0)]:
            c.set_work_queue(groups)
            assert c.work_queue_groups(37, 11) == expect, groups
            _same(c.optimize(s, g, obs), ref, f"groups={groups}")
    finally:
        c.set_work_queue(0)


def test_fallbacks():
    """Launches that dispatch to a kernel without the queue keep the static launch."""
    cases = [
        ("bench-mode GD", _ctx("c3", faithful=False, argv=("--max-inner-iteration=20",)), "c3", {}),
        ("N=100", _ctx("c3bls", argv=("--n-timesteps=100",)), "c3bls", {}),
        ("whole robot", _ctx("c3bls", whole_robot_cost=1), "c3bls", {}),
        ("series", _ctx("c3bls", argv=("--max-inner-iteration=10", "--max-outer-iteration=2")), "c3bls", {"series": True}),
    ]
    for name, c, cfg, kw in cases:
        s, g, obs = _problems(cfg, 0, 37)
        c.set_work_queue(0)
        off = c.optimize(s, g, obs, **kw)
        c.set_work_queue(2)
        try:
            assert c.work_queue_groups(37, 11, **kw) == 0, name
            assert "QUEUE" not in c.launch_plan(37, 11, **kw)["kernel"], name
            on = c.optimize(s, g, obs, **kw)
        finally:
            c.set_work_queue(0)
        _same(on, off, name)
        if kw:
            np.testing.assert_array_equal(on[3], off[3], err_msg=name)


def test_cli_batch_files_identical(tmp_path, monkeypatch, capsys):
    """main's batched path with --work-queue 2 and without: byte-identical batch files."""
    from irm_motion_planning_amd import batch_io, main as irm_main
    files = {}
    for name, extra in [("off", []), ("on", ["--work-queue", "2"])]:
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        irm_main.main(["--batch-size", "40"] + extra)
        out = capsys.readouterr().out
        assert "ignored" not in out, out
        files[name] = {f: open(os.path.join(d, f), "rb").read()
                       for f in (batch_io.RESULT, batch_io.RESULT_BATCH, batch_io.SUMMARY_BATCH)}
    for f in files["off"]:
        assert files["off"][f] == files["on"][f], f
    assert len(files["off"][batch_io.RESULT_BATCH]) > 0
