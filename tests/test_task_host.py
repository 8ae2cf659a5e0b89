"""End-effector goals without a GPU: the fp64 restatement the GPU tests measure against (tests/task_cases.py)
is checked against finite differences of itself and shown to be another function than the joint-goal cost,
the end-to-end scenes are shown to be decided by the algorithm (fp64 BLS from the IK seed and from perturbed
seeds), the IK recipe is run in numpy fp32, and the new C symbols are bound with the header's argument lists.
"""
import ctypes
import re

import numpy as np
import pytest

import moving_cases as mc
import task_cases as tc
from conftest import START, obstacles
from test_abi import HEADER
from test_moving_host import CTYPES_OF, _header_args

SHAPES = [(33, 3), (40, 7)]


def _problem(o, D, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-0.5, 0.5, D).astype(np.float32)
    g = rng.uniform(0.2, 1.6, D).astype(np.float32)
    alpha = (0.05 * rng.standard_normal((o.N, D))).astype(np.float32)
    return alpha, s, g


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("lmax", [0.0, 0.25])
@pytest.mark.parametrize("N,D", SHAPES)
def test_restatement_gradient_is_the_derivative_of_its_cost(N, D, lmax, whole):
    """Central finite differences (h = 1e-6) of the task cost in fp64 against cost_g, 1e-6 relative to max|G|,
    rows N−1 and N−2 included; and the task cost is another function than the joint-goal cost (> 1e-3 relative
    on the same α)."""
    R, o = tc.restatement(*mc.shape_argv(N, D), whole_robot=whole)
    alpha, s, g = _problem(o, D, 11 * N + D)
    p, _ = mc.crossing_tables(1, 11, 2.0, seed=N + D)
    links = [o.params.link_length[i] for i in range(D)]
    goal = tc.TaskGoal(tc.fk64(links, g) + np.array([0.3, -0.2]))
    lam = (0.5, 0.1, lmax)
    G = R.cost_g(alpha, p[0], s, goal, *lam)
    a = alpha.astype(np.float64)
    rng = np.random.default_rng(N)
    h = 1e-6
    idx = [(int(rng.integers(N)), int(rng.integers(D))) for _ in range(20)]
    idx += [(0, 0)] + [(N - 1, d) for d in range(D)] + [(N - 2, d) for d in range(D)]
    for n, d in idx:
        ap, am = a.copy(), a.copy()
        ap[n, d] += h
        am[n, d] -= h
        fd = (R.cost(ap, p[0], s, goal, *lam) - R.cost(am, p[0], s, goal, *lam)) / (2 * h)
        assert abs(fd - G[n, d]) <= 1e-6 * np.abs(G).max(), (n, d, fd, G[n, d])
    joint = R.cost(a, p[0], s, g, *lam)
    assert abs(R.cost(a, p[0], s, goal, *lam) - joint) > 1e-3 * abs(joint)
    Gj = R.cost_g(a, p[0], s, g, *lam)
    assert np.abs(G - Gj).max() > 1e-3 * np.abs(Gj).max()


def test_task_goal_leaves_the_joint_goal_restatement_alone():
    """With a goal configuration TaskRef64 is its parent to the bit, and with λsg = 0 the two goals agree."""
    R, o = tc.restatement(*mc.shape_argv(33, 3))
    P = mc.MovingRef64(o.params, *o.kernel_matrices())
    alpha, s, g = _problem(o, 3, 5)
    obs = obstacles()
    assert R.cost(alpha, obs, s, g, 0.5, 0.1, 0.25) == P.cost(alpha, obs, s, g, 0.5, 0.1, 0.25)
    np.testing.assert_array_equal(R.cost_g(alpha, obs, s, g, 0.5, 0.1, 0.25), P.cost_g(alpha, obs, s, g, 0.5, 0.1, 0.25))
    goal = tc.TaskGoal([1.0, 2.0])
    assert R.cost(alpha, obs, s, goal, 0.0, 0.1, 0.25) == pytest.approx(P.cost(alpha, obs, s, g, 0.0, 0.1, 0.25), rel=1e-14)


def _seed(o, target):
    lo, hi = tc.safety_range(o.params)
    links = [o.params.link_length[i] for i in range(3)]
    return tc.ik_seed(links, START, target, lo, hi)


@pytest.mark.parametrize("target", [tuple(t) for t in tc.E2E_TARGETS.tolist()])
@pytest.mark.parametrize("N", tc.E2E_N)
def test_e2e_scenes_are_decided_by_the_algorithm(N, target):
    """Every problem of the GPU end-to-end test reaches `constraints ok` in the fp64 BLS restatement (default
    hyper-parameters), from the IK seed and from three seeds perturbed by 1e-4·N(0, 1): the scenes are decided
    by the algorithm, not by rounding."""
    R, o = tc.restatement("--n-timesteps", N)
    q, res, _ = _seed(o, target)
    assert res < 1e-5
    goal = tc.TaskGoal(target)
    rng = np.random.default_rng(N)
    seeds = [q.astype(np.float64)] + [q + 1e-4 * rng.standard_normal(3) for _ in range(3)]
    for k, qs in enumerate(seeds):
        a0 = o.init_alpha(START, qs.astype(np.float32))
        alpha, ok, outers, inners = R.bls(a0, obstacles(), START, goal)
        _, rep = R.constraints(alpha, START, goal)
        print(f"N={N} target={target} seed {k}: ok={ok} outer={outers} inner={inners} |f-p|={rep[1]:.2e}")
        assert ok, (N, target, k, rep)


def test_ik_recipe_in_fp32():
    """The recipe of irm_ik_seed in numpy fp32 ends below 1e-5 on every target the GPU tests use (the reference
    arm from start 0; sixteen 7-DoF problems), inside the safety range."""
    _, o = tc.restatement("--n-timesteps", 33)
    lo, hi = tc.safety_range(o.params)
    links = [o.params.link_length[i] for i in range(3)]
    for target in tc.IK_TARGETS3:
        q, res, hist = tc.ik_seed(links, START, target, lo, hi)
        print(target, res, next((i for i, r in enumerate(hist) if r < 1e-5), None))
        assert res < 1e-5, (target, res)
        assert q.min() >= lo and q.max() <= hi
        assert np.linalg.norm(tc.fk64(links, q) - target.astype(np.float64)) < 1e-5
    start, targets = tc.ik_problems7()
    for s, p in zip(start, targets):
        q, res, _ = tc.ik_seed(mc.LINKS7, s, p, lo, hi)
        assert res < 1e-5, (p, res)
        assert q.min() >= lo and q.max() <= hi
    # out of reach (‖p‖ = Σ links + 1) on the axis of the stretched start: J_eeᵀ·e is exactly 0, the seed stays
    # and the residual is the missing length
    start, far = tc.out_of_reach(links)
    _, res, _ = tc.ik_seed(links, start, far, lo, hi)
    assert abs(res - 1.0) < 1e-3
    # Off that axis the 32 damped Gauss-Newton steps do not settle on the stretched pose (the residual is large
    # there, and the step ignores the curvature it brings): residuals 1.03 … 1.11 for targets 10° … 90° off
    # the start's axis, in fp32 and fp64 alike — never below the missing length, which is all that is asserted
    for ang in (10.0, 45.0, 90.0):
        p = (sum(links) + 1.0) * np.array([np.cos(np.radians(ang)), np.sin(np.radians(ang))])
        _, res, _ = tc.ik_seed(links, START, p.astype(np.float32), lo, hi)
        print("out of reach at", ang, "degrees: residual", res)
        assert res >= 1.0 - 1e-5, (ang, res)


# ------------------------------------------------------------------------------------- header and binding
TASK = ["irm_eval_cost_task", "irm_eval_cost_grad_task", "irm_constraints_task", "irm_optimize_batch_task",
        "irm_optimize_batch_task_dev", "irm_optimize_plan_task"]
IK = ["irm_ik_seed", "irm_ik_seed_dev"]


def test_task_symbols_are_bound_as_declared():
    from irm_motion_planning_amd import _abi
    from test_abi import declared_functions
    named = {"c_float_p": _abi.c_float_p, "IrmBatchDev*": ctypes.POINTER(_abi.IrmBatchDev),
             "IrmStats*": ctypes.POINTER(_abi.IrmStats), "IrmLaunchPlan*": ctypes.POINTER(_abi.IrmLaunchPlan),
             "uint8_t*": _abi.c_uint8_p}
    ctypes_of = dict(CTYPES_OF, **{"uint8_t*": "uint8_t*"})
    lib = _abi.load_library()
    declared = declared_functions()
    assert sorted(n for n in declared if n.endswith("_task") or n.endswith("_task_dev")) == sorted(TASK)
    assert sorted(n for n in declared if "ik_seed" in n) == sorted(IK)
    for name in TASK + IK:
        assert hasattr(lib, name), name
        res, args = _abi.PROTOTYPES[name]
        assert res is ctypes.c_int
        want = [named.get(w, w) for w in (ctypes_of[a] for a in _header_args(name))]
        assert args == want, (name, args, want)
    P, fp = _abi.PROTOTYPES, _abi.c_float_p
    # the _moving forms' arguments plus goal_xy (irm_constraints: its own plus goal_xy; the plan: the same)
    assert P["irm_eval_cost_task"][1] == P["irm_eval_cost_moving"][1] + [fp]
    assert P["irm_eval_cost_grad_task"][1] == P["irm_eval_cost_grad_moving"][1] + [fp]
    assert P["irm_constraints_task"][1] == P["irm_constraints"][1] + [fp]
    assert P["irm_optimize_batch_task"][1] == P["irm_optimize_batch_moving"][1] + [fp]
    assert P["irm_optimize_batch_task_dev"][1] == P["irm_optimize_batch_moving_dev"][1][:-1] + [fp, ctypes.c_void_p]
    assert P["irm_optimize_plan_task"][1] == P["irm_optimize_plan"][1]
    assert P["irm_ik_seed"][1] == [ctypes.c_void_p, fp, fp, ctypes.c_int32, fp, fp]
    assert P["irm_ik_seed_dev"][1] == P["irm_ik_seed"][1] + [ctypes.c_void_p]
    assert _abi.IRM_ABI_VERSION == 3 and re.search(r"#define IRM_ABI_VERSION 3\b", open(HEADER).read())


# sizeof of every struct of include/irm.h as the parent commit's bindings had it
STRUCT_SIZES = {"IrmBatchDev": 80, "IrmDenseReport": 40, "IrmInfo": 152, "IrmLaunchPlan": 176, "IrmParams": 544,
                "IrmStats": 32}


def test_struct_sizes_are_unchanged():
    """No struct changes layout: ctypes.sizeof of every bound struct is what it was before the feature, and no
    struct was added."""
    from irm_motion_planning_amd import _abi
    bound = {n: ctypes.sizeof(c) for n, c in vars(_abi).items()
             if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}
    assert bound == STRUCT_SIZES


def test_cli_flag_defaults_to_absent():
    from conftest import ref_args
    assert ref_args().goal_xy is None
    assert ref_args("--goal-xy", "1.348", "2.538").goal_xy == [1.348, 2.538]
