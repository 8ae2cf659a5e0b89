"""The tracing restatement of tests/bls_cases.py on the CPU: it is the C oracle's optimiser on the problems the
oracle knows, every scene the GPU tests run decides each of its comparisons by a safe margin, and the log tells
the right algorithm from five wrong ones."""
import numpy as np
import pytest

import bls_cases as bc
import via_cases as vc
from conftest import GOAL, START, obstacles
from variant_shape_cases import MUTANT_FACTOR, ORACLE_FLOOR

# ------------------------------------------------------------------ 1. the anchor: the C oracle
# Largest relative deviation of the restatement's log from Oracle.optimize_trace per flow and column (new_loss,
# required, loss, ‖g‖, alpha_norm), over N = 33 and 50, measured here: fp64 rounded once against the oracle's fp32
# sums from init_alpha's α0 (|α0| ~ 1e3).  The reject flow's first trials step by lr = 1 and 0.5 from that α0 and
# land on iterates of that size, where the oracle's fp32 gradient sums lose 6e-4 on alpha_norm (N = 33; N = 50 stays
# at 8e-7).  The test holds each column to twice these.
ANCHOR_MEASURED = {
    "forced": (3.9e-6, 1.1e-7, 1.1e-7, 4.0e-7, 5.5e-6),
    "reject": (5.1e-5, 7.5e-6, 7.3e-6, 1.51e-4, 5.7e-4),
    "default-llr": (1.3e-6, 1.9e-7, 1.9e-7, 9.3e-7, 4.7e-6),
}
ANCHOR_GD_MEASURED = 1.1e-7  # max |K·α·J| difference of the end trajectories, gd2


def _static_problem(N, flow):
    R, o = vc.restatement("--n-timesteps", N, *bc.FLOWS[flow])
    obs = obstacles()
    return R, o, o.init_alpha(START, GOAL), obs, R.table(obs, np.zeros_like(obs))


@pytest.mark.parametrize("flow", sorted(ANCHOR_MEASURED))
@pytest.mark.parametrize("N", [33, 50])
def test_bls_log_is_the_oracles_on_a_static_joint_goal_problem(N, flow):
    R, o, a0, obs, table = _static_problem(N, flow)
    assert R.via == []
    run = bc.bls_log(R, a0, table, START, GOAL)
    _, st, tr = o.optimize_trace(a0, obs, START, GOAL, cap=4096)
    assert run.log.shape == tr.shape and len(tr) >= 8
    np.testing.assert_array_equal(run.log[:, [0, 1, 2, 6]], tr[:, [0, 1, 2, 6]])
    np.testing.assert_array_equal(run.log[:, 3], tr[:, 3])  # lr: the same fp32 products
    for k in bc.COUNTERS + ("constraints_ok",):
        assert run.stats[k] == st[k], (k, run.stats, st)
    dev = [float(np.max(np.abs(run.log[:, c].astype(np.float64) - tr[:, c]) / np.abs(tr[:, c]))) for c in (4, 5, 7, 8, 9)]
    print(f"N={N} {flow}: {len(tr)} records, relative deviation new_loss {dev[0]:.1e}, required {dev[1]:.1e}, loss {dev[2]:.1e}, "
          f"|g| {dev[3]:.1e}, alpha_norm {dev[4]:.1e}")
    for d, m in zip(dev, ANCHOR_MEASURED[flow]):
        assert d <= 2.0 * m, (dev, ANCHOR_MEASURED[flow])
    assert abs(run.stats["final_loss"] - st["final_loss"]) <= 2.0 * ANCHOR_MEASURED[flow][0] * abs(st["final_loss"])


@pytest.mark.parametrize("N", [33, 50])
def test_gd_dual_is_the_oracles_on_a_static_joint_goal_problem(N):
    R, o, a0, obs, table = _static_problem(N, "gd2")
    run = bc.gd_dual(R, a0, table, START, GOAL)
    a_o, st = o.optimize(a0, obs, START, GOAL)
    for k in bc.COUNTERS + ("constraints_ok",):
        assert run.stats[k] == st[k], (k, run.stats, st)
    assert run.stats["outer_iterations"] == 3 and len(run.trajectories) == 3
    d = float(np.abs(run.trajectories[-1] - o.evaluate(a_o)).max())
    print(f"N={N} gd2: end trajectories {d:.1e} apart, final_loss {run.stats['final_loss']} / {st['final_loss']}")
    assert d <= 2.0 * ANCHOR_GD_MEASURED
    assert abs(run.stats["final_loss"] - st["final_loss"]) <= 1e-6 * abs(st["final_loss"])


def test_zero_velocity_and_an_empty_via_list_are_the_static_run_to_the_bit():
    sc = bc.scene(33, 3, 5, "all", "forced")
    R, table, goal = bc.problem(sc, 0, features=False)
    a = bc.bls_log(R, sc["alpha"][0], table, sc["s"][0], goal)
    b = bc.bls_log(R, sc["alpha"][0], R.table(sc["p"][0], np.zeros_like(sc["p"][0])), sc["s"][0], goal)
    assert a.log.tobytes() == b.log.tobytes() and a.alpha.tobytes() == b.alpha.tobytes() and a.stats == b.stats


# ------------------------------------------------------------------ 2. seeds are conditions, not luck
def test_the_cases_cover_what_they_must():
    cases = set(bc.CASES)
    assert {c[3] for c in cases if c[:3] == (33, 3, 5)} == set(bc.SETS)
    assert all((*sh, "all") in cases for sh in bc.SHAPES)
    for f in ("moving", "task", "via-joint", "via-cart"):
        assert any(c[3] == f and c[0] > 64 for c in cases), f
    assert bc.via_rows(129, "via-cart") == ([64, 127], [1, 1]) and bc.via_rows(129, "all") == ([64, 127], [0, 1])
    assert all((*sh, "all", "gd2") in bc.gd_cases() for sh in bc.SHAPES)
    assert {c[3] for c in bc.gd_cases() if c[:3] == (33, 3, 5)} >= {"moving", "task", "via-joint", "via-cart", "all"}


@pytest.mark.parametrize("N,D,TB,fs,flow", bc.flow_cases() + bc.gd_cases())
def test_every_problem_of_a_scene_decides_by_a_safe_margin(N, D, TB, fs, flow):
    """All B problems, with the features and without (the launch e_static is measured on)."""
    sc = bc.scene(N, D, TB, fs, flow)
    assert sc["B"] == TB + 1 <= 6
    for b in range(sc["B"]):
        run = bc.reference_run(N, D, TB, fs, flow, b)
        rep = bc.seed_report(run, flow)
        assert all(rep.values()), (b, sc["seeds"][b], rep)
        if flow != "gd2":
            R, table, goal = bc.problem(sc, b)
            spread = bc.gradient_spread(run, R, sc["alpha"][b], table, sc["s"][b], goal)
            assert spread <= bc.GRADIENT_SHARE, (b, sc["seeds"][b], spread)
        free = bc.seed_report(bc.reference_run(N, D, TB, fs, flow, b, features=False), flow)
        assert all(free[k] for k in ("decision", "llr", "predicate", "mask") if k in free), (b, sc["seeds"][b], free)
        if flow != "gd2":
            assert len(run.log) <= 3 * 30 * 20
    run = bc.reference_run(N, D, TB, fs, flow, 0)
    print(f"N={N} D={D} {fs} {flow}: problem 0 runs {run.stats}, smallest margins: decision "
          f"{min(run.decision) if run.decision else float('inf'):.1e}, llr {min(run.llr):.1e}, predicate "
          f"{min(run.predicate):.1f}, mask {min(run.mask):.1f} (the last two in required margins)")


# ------------------------------------------------------------------ 3. mutants
@pytest.mark.parametrize("N,D,TB,fs,flow", bc.flow_cases())
def test_the_log_tells_the_mutants_from_the_restatement(N, D, TB, fs, flow):
    """Problem 0, whose log the device writes.  Every mutant that applies to the scene's features flips an accept /
    reject or a counter, or moves a logged column by MUTANT_FACTOR tolerances.  predicate-blind applies only where
    the blind predicate and the right one differ at some outer end (none of these scenes rests at its ends after
    five line searches: the rest scene below is the one that tells it)."""
    sc = bc.scene(N, D, TB, fs, flow)
    R, table, goal = bc.problem(sc, 0)
    run = bc.reference_run(N, D, TB, fs, flow, 0)
    muts = bc.mutants(R, table, sc["p"][0], goal, sc["g"][0])
    assert {"slope-without-feature", "lr-carried"} <= set(muts)
    assert ("trial-frozen-table" in muts) == (sc["w"] is not None)
    assert ("lambda-stuck" in muts) == (fs != "moving")
    told = {}
    for name, kw in sorted(muts.items()):
        kw = dict(kw)
        mut = bc.bls_log(kw.pop("R", R), sc["alpha"][0], table, sc["s"][0], goal, **kw)
        kind, d = bc.separation(run, mut)
        told[name] = kind if d is None else f"{d:.0f} tolerances"
        if name == "predicate-blind" and kind == "moved" and d == 0.0:
            told[name] = "does not apply"
            continue
        assert kind == "flip" or d >= MUTANT_FACTOR, (name, kind, d)
    print(f"N={N} D={D} {fs} {flow}: {told}")


GD_PLAN_TELLS = {(129, "all"), (256, "all"), (33, "via-cart")}
REST = ("--optimizer-name", "bls", "--n-timesteps", "33", "--max-outer-iteration", "3", "--max-inner-iteration", "0")


def rest_problem(cart):
    """The plan α = 0 from the configuration 0 to itself fulfils every static constraint exactly; a via-point 0.2
    away, or an end-effector goal 0.2 from f(0), is all that fails.  With no inner iteration the outer loop is the
    predicate alone: three outer iterations and constraints_ok = 0, where a predicate blind to the feature stops
    after one with constraints_ok = 1."""
    R, o = vc.restatement(*REST)
    z = np.zeros(3, np.float32)
    far = np.array([3.0 - 0.2, 0.0, 77.0], np.float32) if cart else np.array([0.2, 0.0, 0.0], np.float32)
    return R.with_via(vc.entries([16], [cart], [far])), o, z


@pytest.mark.parametrize("cart", [0, 1])
def test_a_predicate_blind_to_the_feature_is_told_on_the_rest_scene(cart):
    R, o, z = rest_problem(cart)
    a0 = np.zeros((33, 3), np.float32)
    run = bc.bls_log(R, a0, obstacles(), z, z)
    blind = bc.bls_log(R, a0, obstacles(), z, z, predicate=(R.with_via(()), z))
    assert (run.stats["outer_iterations"], run.stats["constraints_ok"]) == (3, 0)
    assert (blind.stats["outer_iterations"], blind.stats["constraints_ok"]) == (1, 1)
    assert min(run.predicate) >= 1.0 and min(blind.predicate) >= 1.0
    goal = bc.TaskGoal(np.array([2.8, 0.0], np.float32))
    run = bc.bls_log(R.with_via(()), a0, obstacles(), z, goal)
    blind = bc.bls_log(R.with_via(()), a0, obstacles(), z, goal, predicate=(R.with_via(()), z))
    assert (run.stats["outer_iterations"], run.stats["constraints_ok"]) == (3, 0)
    assert (blind.stats["outer_iterations"], blind.stats["constraints_ok"]) == (1, 1)


@pytest.mark.parametrize("N,D,TB,fs,flow", [c for c in bc.gd_cases() if c[3] != "moving"])  # moving: no λ-weighted term
def test_gd_dual_tells_a_feature_left_at_the_first_lambda(N, D, TB, fs, flow):
    """The dual loop's later outer iterations step by gd_lr[1] = 1e-4 and gd_lr[2] = 1e-5: ten such steps move the
    plan little, whatever λ the feature term carries.  The mutant lies four band floors (4 · ORACLE_FLOOR) from the
    restatement's end plan at the shapes of GD_PLAN_TELLS and 1.4 … 3.2 floors at the others; what
    the raised λ moves everywhere is the loss the loop reports, by 10 % and more, against a final_loss band the GPU
    test caps at GD_LOSS_RTOL_CAP."""
    sc = bc.scene(N, D, TB, fs, flow)
    R, table, goal = bc.problem(sc, 0)
    run = bc.reference_run(N, D, TB, fs, flow, 0)
    mut = bc.gd_dual(bc._clone(R, bc.LambdaStuck), sc["alpha"][0], table, sc["s"][0], goal)
    d = float(np.abs(run.trajectories[-1] - mut.trajectories[-1]).max())
    dl = abs(run.stats["final_loss"] - mut.stats["final_loss"]) / abs(run.stats["final_loss"])
    print(f"N={N} D={D} {fs}: λ-stuck mutant moves the end trajectory by {d:.2e} ({d / ORACLE_FLOOR:.2f} floors), final_loss by "
          f"{dl:.2e} relative, counters {mut.stats} against {run.stats}")
    assert dl >= MUTANT_FACTOR * bc.GD_LOSS_RTOL_CAP
    if (N, fs) in GD_PLAN_TELLS:
        assert d >= MUTANT_FACTOR * ORACLE_FLOOR, d
