"""The line search and the dual λ loop of moving, goal and via launches on the GPU, against the tracing restatement
of tests/bls_cases.py (checked on the CPU by tests/test_bls_cases_host.py: anchored to the C oracle, every scene
decides by a safe margin, the log tells five wrong kernels from the right one).

k_optimize<DynShape<D>> writes problem 0's line-search log in every variant; here the log of a feature launch is
laid next to the restatement's row by row.  The band is measured in the same test on the existing code path: e_static
is the deviation of the same context's feature-free launch of the same problems from the restatement without
features, wherever that launch also runs the general kernel (launch_plan says so); the floors are the project's.
Every test prints what it measured.
"""
import functools

import numpy as np
import pytest

import bls_cases as bc
import moving_cases as mc
import variant_shape_cases as vsc
from conftest import obstacles, params
from test_bls_cases_host import REST, rest_problem

pytestmark = pytest.mark.gpu

INT_COLS, LR_COL = [0, 1, 2, 6], 3
COLS = (("new_loss", 4, bc.LOSS_RTOL), ("required", 5, bc.LOSS_RTOL), ("loss", 7, bc.LOSS_RTOL), ("|g|", 8, bc.NORM_RTOL),
        ("alpha_norm", 9, bc.NORM_RTOL))
TRACE_CAP = 2048  # 3 outer × 30 inner × 20 trials at the most: 1800


def ctx(*argv, **overrides):
    from irm_motion_planning_amd.context import Context
    return Context(params(*argv, **overrides))


@functools.lru_cache(maxsize=None)
def flow_ctx(N, D, TB, whole, flow):
    c = ctx(*mc.shape_argv(N, D), *bc.FLOWS[flow], traj_per_block=TB, whole_robot_cost=int(whole))
    c.bls_trace_enable(TRACE_CAP)
    return c


def feature_kw(sc, idx):
    """The feature arguments of optimize() for the problems idx of a scene."""
    from irm_motion_planning_amd.via import ViaPoints
    return dict(obstacle_velocity=None if sc["w"] is None else sc["w"][idx], goal_xy=None if sc["xy"] is None else sc["xy"][idx],
                via=ViaPoints(sc["rows"], sc["cart"], sc["targets"][idx]) if sc["rows"] else None)


def launch(c, sc, idx, features):
    """(alpha, traj, stats, problem 0's log) of one optimize() of the problems idx."""
    kw = feature_kw(sc, idx) if features else {}
    alpha, traj, st = c.optimize(sc["s"][idx], sc["g"][idx], sc["p"][idx], alpha0=sc["alpha"][idx], **kw)
    log = c.bls_trace(int(st["bls_trials"][0])) if sc["flow"] != "gd2" else None
    return alpha, traj, st, log


def reached(c, sc):
    """Assert the kernels the two launches of a scene reach; returns (the feature plan, whether the feature-free
    launch runs the general kernel too)."""
    N, D, TB, B = sc["N"], sc["D"], sc["TB"], sc["B"]
    pl = c.launch_plan(B, sc["O"], **feature_kw(sc, np.arange(B)))
    flow = "GD" if sc["flow"] == "gd2" else "BLS"
    assert pl["lean"] == 0 and pl["kernel"].startswith(f"k_optimize<DynShape<{D}>,") and f",{flow}" in pl["kernel"], pl
    assert pl["traj_per_block"] == TB and pl["grid"] == (B + TB - 1) // TB == 2, pl
    if (N, D, TB) in vsc.OPTIMIZE and not sc["whole"]:
        inst, launched, ops, regops = vsc.OPTIMIZE[(N, D, TB)]
        assert pl["kernel"].startswith(f"k_optimize<DynShape<{D}>,{inst},{ops},{regops},{flow}") and pl["threads"] == launched, pl
    free = c.launch_plan(B, sc["O"])
    return pl, free["lean"] == 0, free["kernel"]


def deviations(log, ref):
    """Per column, the largest relative deviation of a device log from the restatement's; the integer columns and lr
    are asserted here."""
    assert log.shape == ref.shape, (log.shape, ref.shape, log[:, INT_COLS][: len(ref)].tolist(), ref[:, INT_COLS].tolist())
    np.testing.assert_array_equal(log[:, INT_COLS], ref[:, INT_COLS])  # outer, inner, trial, accepted
    np.testing.assert_allclose(log[:, LR_COL], ref[:, LR_COL], rtol=1e-7)
    return {name: float(np.max(np.abs(log[:, c].astype(np.float64) - ref[:, c]) / np.abs(ref[:, c].astype(np.float64))))
            for name, c, _ in COLS}


def static_deviations(log, ref):
    """deviations() of the feature-free launch: measured over the rows before its first differing decision (all of
    them: the host test holds the feature-free runs to the same margins), reported rather than asserted."""
    n = min(len(log), len(ref))
    same = np.all(log[:n, INT_COLS] == ref[:n, INT_COLS], axis=1)
    n = n if same.all() else int(np.argmin(same))
    return deviations(log[:n], ref[:n]), n == len(ref) == len(log)


def check_log(tag, log, run, e_static):
    dev = deviations(log, run.log)
    band = {name: max(tol, 2.0 * e_static.get(name, 0.0)) for name, _, tol in COLS}
    print(f"{tag}: {len(log)} records, accepted {int(log[:, 6].sum())}; relative deviation " +
          ", ".join(f"{k} {v:.1e} (static {e_static.get(k, 0.0):.1e})" for k, v in dev.items()))
    for name in dev:
        assert dev[name] <= band[name], (name, dev, band)
    return dev


def check_counters(tag, st, runs):
    for b, run in enumerate(runs):
        for k in bc.COUNTERS + ("constraints_ok",):
            assert int(st[k][b]) == run.stats[k], (tag, b, k, {q: int(st[q][b]) for q in bc.COUNTERS}, run.stats)


def measure(c, sc, general_static):
    """The two launches of a scene and the restatement's runs of all B problems: a dict of what the tests compare."""
    N, D, TB, fs, flow, B = sc["N"], sc["D"], sc["TB"], sc["fs"], sc["flow"], sc["B"]
    idx = np.arange(B)
    R, _ = bc.restatement(N, D, sc["whole"], flow)
    runs = [bc.reference_run(N, D, TB, fs, flow, b) for b in range(B)]
    free = [bc.reference_run(N, D, TB, fs, flow, b, features=False) for b in range(B)]
    a_f, t_f, st_f, log_f = launch(c, sc, idx, True)
    a_0, t_0, st_0, log_0 = launch(c, sc, idx, False)
    out = dict(runs=runs, free=free, alpha=a_f, traj=t_f, st=st_f, log=log_f, st0=st_0, e_log={}, e_traj=0.0, e_loss=0.0,
               moved=float(np.abs(t_f - t_0).max()))
    if general_static:
        if log_0 is not None:
            out["e_log"], whole_log = static_deviations(log_0, free[0].log)
            if not whole_log:
                print(f"  the feature-free launch leaves the restatement's decisions after {len(log_0)} / {len(free[0].log)} records")
        out["e_traj"] = max(float(np.abs(t_0[b] - R.traj_vel(free[b].alpha)[0]).max()) for b in range(B))
        out["e_loss"] = max(abs(float(st_0["final_loss"][b]) - free[b].stats["final_loss"]) / abs(free[b].stats["final_loss"]) for b in range(B))
    out["traj_err"] = max(float(np.abs(t_f[b] - R.traj_vel(runs[b].alpha)[0]).max()) for b in range(B))
    out["loss_err"] = max(abs(float(st_f["final_loss"][b]) - runs[b].stats["final_loss"]) / abs(runs[b].stats["final_loss"]) for b in range(B))
    return out


# ------------------------------------------------------------------ 1. the line-search log, counters and end state
@pytest.mark.parametrize("N,D,TB,fs,flow", bc.flow_cases())
def test_bls_log_counters_and_end_state_match_the_restatement(N, D, TB, fs, flow):
    """Problem 0's log over all records: outer, inner, trial, accepted equal, lr at 1e-7, new_loss / required / loss at
    max(1e-5, 2·e_static), ‖g‖ / alpha_norm at max(1e-4, 2·e_static).  All B problems: the counters and the flag
    equal, final_loss at the loss tolerance, K·α_out·J within max(2·e_static, ORACLE_FLOOR)."""
    sc = bc.scene(N, D, TB, fs, flow)
    c = flow_ctx(N, D, TB, sc["whole"], flow)
    pl, general_static, free_kernel = reached(c, sc)
    m = measure(c, sc, general_static)
    tag = f"N={N} D={D} TB={TB} {fs} {flow} on {pl['kernel']} (feature-free: {free_kernel})"
    check_counters(tag, m["st"], m["runs"])
    check_log(tag, m["log"], m["runs"][0], m["e_log"])
    band_t, band_l = max(2.0 * m["e_traj"], vsc.ORACLE_FLOOR), max(2.0 * m["e_loss"], bc.LOSS_RTOL)
    print(f"  all {sc['B']} problems: |K·α_out·J − restatement| {m['traj_err']:.2e} (static {m['e_traj']:.2e}, band {band_t:.1e}), "
          f"final_loss {m['loss_err']:.1e} (static {m['e_loss']:.1e}, band {band_l:.1e}); the features move the plan by {m['moved']:.2e}")
    assert m["moved"] > 1e-3  # the features reached the launch
    assert m["loss_err"] <= band_l, (m["loss_err"], band_l)
    assert m["traj_err"] <= band_t, (m["traj_err"], band_t)
    if general_static:
        check_counters(tag + " feature-free", m["st0"], m["free"])


# ------------------------------------------------------------------ 2. every slot
@pytest.mark.parametrize("N,D,TB", [(33, 3, 5), (129, 3, 4)])
def test_every_slot_writes_the_log_of_its_own_problem(N, D, TB):
    """Each other problem of the `all` scene swapped to index 0: its log matches its own restatement, and alpha_out is
    bit-equal to that problem's result in its original slot."""
    fs, flow = "all", "forced"
    sc = bc.scene(N, D, TB, fs, flow)
    c = flow_ctx(N, D, TB, False, flow)
    _, general_static, _ = reached(c, sc)
    base, _, _, _ = launch(c, sc, np.arange(sc["B"]), True)
    for b in range(1, sc["B"]):
        idx = np.arange(sc["B"])
        idx[0], idx[b] = b, 0
        alpha, _, st, log = launch(c, sc, idx, True)
        e_static = {}
        if general_static:
            _, _, _, log0 = launch(c, sc, idx, False)
            e_static, _ = static_deviations(log0, bc.reference_run(N, D, TB, fs, flow, b, features=False).log)
        check_log(f"N={N} problem {b} in slot 0", log, bc.reference_run(N, D, TB, fs, flow, b), e_static)
        np.testing.assert_array_equal(alpha[0], base[b])
        np.testing.assert_array_equal(alpha[b], base[0])


# ------------------------------------------------------------------ 3. the GD dual loop
@pytest.mark.parametrize("N,D,TB,fs,flow", bc.gd_cases())
def test_gd_dual_loop_matches_the_restatement(N, D, TB, fs, flow):
    """Three outer iterations of ten steps, λ raised twice: the plan within max(2·e_static, ORACLE_FLOOR) of gd_dual,
    counters and flag equal.  final_loss, which the raised λ weighs (the plan itself moves by less than the floor in
    the later outer iterations, tests/test_bls_cases_host.py), within max(2·e_static, 1e-5) relative, a band that
    has to stay under GD_LOSS_RTOL_CAP to tell the λ mutant."""
    sc = bc.scene(N, D, TB, fs, flow)
    c = flow_ctx(N, D, TB, sc["whole"], flow)
    pl, general_static, free_kernel = reached(c, sc)
    m = measure(c, sc, general_static)
    tag = f"N={N} D={D} TB={TB} {fs} gd2 on {pl['kernel']} (feature-free: {free_kernel})"
    band_t, band_l = max(2.0 * m["e_traj"], vsc.ORACLE_FLOOR), max(2.0 * m["e_loss"], bc.LOSS_RTOL)
    print(f"{tag}: |K·α_out·J − gd_dual| {m['traj_err']:.2e} (static {m['e_traj']:.2e}, band {band_t:.1e}), final_loss "
          f"{m['loss_err']:.1e} (static {m['e_loss']:.1e}, band {band_l:.1e}); the features move the plan by {m['moved']:.2e}")
    check_counters(tag, m["st"], m["runs"])
    assert m["moved"] > 1e-3
    assert m["traj_err"] <= band_t, (m["traj_err"], band_t)
    assert band_l <= bc.GD_LOSS_RTOL_CAP, band_l
    assert m["loss_err"] <= band_l, (m["loss_err"], band_l)


# ------------------------------------------------------------------ 4. the null case
def test_null_features_leave_the_log_bit_identical():
    from irm_motion_planning_amd.via import ViaPoints
    N, D, TB = 33, 3, 5
    sc = bc.scene(N, D, TB, "all", "forced")
    c = flow_ctx(N, D, TB, False, "forced")
    idx = np.arange(sc["B"])
    a0, t0, st0, log0 = launch(c, sc, idx, False)
    assert len(log0) >= 8
    for kw in (dict(obstacle_velocity=np.zeros_like(sc["p"])), dict(via=None, goal_xy=None), dict(via=ViaPoints.empty()),
               dict(obstacle_velocity=np.zeros_like(sc["p"]), via=ViaPoints.empty(), goal_xy=None)):
        a, t, st = c.optimize(sc["s"], sc["g"], sc["p"], alpha0=sc["alpha"], **kw)
        log = c.bls_trace(int(st["bls_trials"][0]))
        assert log.tobytes() == log0.tobytes(), sorted(kw)
        np.testing.assert_array_equal(a, a0)
        for k in st0:
            np.testing.assert_array_equal(st[k], st0[k], err_msg=k)


# ------------------------------------------------------------------ 5. the predicate sees the feature
@pytest.mark.parametrize("cart", [0, 1])
def test_the_predicate_sees_the_via_and_the_cartesian_distance(cart):
    """The rest scene of tests/test_bls_cases_host.py: α = 0 from 0 to 0 fulfils every static constraint, so the outer
    loop runs on the feature's distance alone — three outer iterations and constraints_ok = 0 with the feature, one
    and constraints_ok = 1 without, as the restatement (a blind predicate would stop after one)."""
    from irm_motion_planning_amd.via import ViaPoints
    R, _, z = rest_problem(cart)
    c = ctx(*REST)
    a0 = np.zeros((33, 3), np.float32)
    obs = obstacles()
    (m, k, target), = R.via
    cases = {"none": {}, "via": dict(via=ViaPoints([m], [k], target[None])), "goal_xy": dict(goal_xy=np.array([2.8, 0.0], np.float32))}
    want = {"none": (1, 1), "via": (3, 0), "goal_xy": (3, 0)}
    for name, kw in cases.items():
        _, _, st = c.optimize(z, z, obs, alpha0=a0, **kw)
        Rn = R if name == "via" else R.with_via(())
        run = bc.bls_log(Rn, a0, obs, z, bc.TaskGoal(kw["goal_xy"]) if name == "goal_xy" else z)
        got = (int(st["outer_iterations"]), int(st["constraints_ok"]))
        print(f"rest scene, {name} (cartesian={cart}): outer iterations, constraints_ok = {got}, restatement "
              f"{(run.stats['outer_iterations'], run.stats['constraints_ok'])}")
        assert got == (run.stats["outer_iterations"], run.stats["constraints_ok"]) == want[name]
