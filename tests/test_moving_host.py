"""Moving obstacles without a GPU: the fp64 restatement the GPU tests measure against (tests/moving_cases.py)
is checked against its parent and against finite differences of itself, Replanner.advance's obstacle
arithmetic bit for bit, the crossing scene is shown to be decidable, and the new C symbols are bound with
the header's argument lists.
"""
import ctypes
import re

import numpy as np
import pytest

import moving_cases as mc
from conftest import GOAL, START
from test_abi import HEADER

SHAPES = [(33, 3), (40, 7)]


def _problem(o, D, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-0.5, 0.5, D).astype(np.float32)
    g = rng.uniform(0.2, 1.6, D).astype(np.float32)
    alpha = (0.05 * rng.standard_normal((o.N, D))).astype(np.float32)
    return alpha, s, g


@pytest.mark.parametrize("N,D", SHAPES)
def test_restatement_equals_parent_at_zero_velocity(N, D):
    """w = 0: MovingRef64's cost and gradient are Ref64's to the bit (per-waypoint table and plain table)."""
    from oracle.ref64 import Ref64
    R, o = mc.restatement(*mc.shape_argv(N, D))
    t, K, dK, J = o.kernel_matrices()
    P = Ref64(o.params, K, dK, J)
    alpha, s, g = _problem(o, D, N)
    p, w = mc.crossing_tables(1, 11, 2.0, seed=N)
    tab = R.table(p[0], np.zeros_like(w[0]))
    for lam in ((0.5, 0.1, 0.0), (0.5, 0.1, 0.25), (50, 10, 1.0)):
        ref = P.cost(alpha, p[0], s, g, *lam)
        assert R.cost(alpha, tab, s, g, *lam) == ref
        assert R.cost(alpha, p[0], s, g, *lam) == ref
        Gref = P.cost_g(alpha, p[0], s, g, *lam)
        np.testing.assert_array_equal(R.cost_g(alpha, tab, s, g, *lam), Gref)
        np.testing.assert_array_equal(R.cost_g(alpha, p[0], s, g, *lam), Gref)


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("lmax", [0.0, 0.25])
@pytest.mark.parametrize("N,D", SHAPES)
def test_restatement_gradient_is_the_derivative_of_its_cost(N, D, lmax, whole):
    """Central finite differences of the moving cost in fp64 against cost_g, 1e-6 relative to max|G| — the
    gradient has no term beyond the static formula on each waypoint's own table."""
    R, o = mc.restatement(*mc.shape_argv(N, D), whole_robot=whole)
    alpha, s, g = _problem(o, D, 7 * N + D)
    p, w = mc.crossing_tables(1, 11, 2.0, seed=N + D)
    tab = R.table(p[0], w[0])
    lam = (0.5, 0.1, lmax)
    G = R.cost_g(alpha, tab, s, g, *lam)
    a = alpha.astype(np.float64)
    rng = np.random.default_rng(N)
    h = 1e-6
    idx = [(int(rng.integers(N)), int(rng.integers(D))) for _ in range(24)] + [(0, 0), (N - 1, D - 1)]
    for n, d in idx:
        ap, am = a.copy(), a.copy()
        ap[n, d] += h
        am[n, d] -= h
        fd = (R.cost(ap, tab, s, g, *lam) - R.cost(am, tab, s, g, *lam)) / (2 * h)
        assert abs(fd - G[n, d]) <= 1e-6 * np.abs(G).max(), (n, d, fd, G[n, d])
    # and it is another function than the static one
    assert abs(R.cost(a, tab, s, g, *lam) - R.cost(a, p[0], s, g, *lam)) > 1e-3 * abs(R.cost(a, p[0], s, g, *lam))


def test_advance_obstacles_bit_for_bit():
    """p' + s·w' == p + (tau + (1 − tau)·s)·w exactly, on dyadic inputs where every operation is exact."""
    from irm_motion_planning_amd.replanning import advance_obstacles
    tau = 0.25
    for O in (5, 11, 13):
        p, w = mc.dyadic_scene(O, B=3)
        p1, w1 = advance_obstacles(p, w, tau)
        assert p1.dtype == np.float32 and w1.dtype == np.float32 and p1.shape == p.shape
        np.testing.assert_array_equal(p1.astype(np.float64), p.astype(np.float64) + tau * w.astype(np.float64))
        np.testing.assert_array_equal(w1.astype(np.float64), 0.75 * w.astype(np.float64))
        for s in np.arange(0, 65) / 64.0:
            new = (p1 + np.float32(s) * w1).astype(np.float32)  # fp32, as the device forms it
            old = p.astype(np.float64) + (tau + (1 - tau) * s) * w.astype(np.float64)
            np.testing.assert_array_equal(new.astype(np.float64), old)
    # zero velocity: the table stays
    p1, w1 = advance_obstacles(p, np.zeros_like(w), 0.3)
    np.testing.assert_array_equal(p1, p)
    assert not w1.any()


def test_crossing_scene_is_decidable():
    """200 fp64 GD steps on the moving objective end at a lower moving loss and a lower largest per-waypoint
    moving potential than 200 steps against the table frozen at t = 0, by at least 10 % each — and so does the
    largest moving potential on the 129 times the GPU test's dense_check looks at (the query matrix of
    irm_query_matrices, host only, widened)."""
    R, o = mc.restatement(*mc.CROSSING_ARGV)
    p = o.params
    lam = (p.lambda_sg_constraint, p.lambda_jl_constraint, p.lambda_max_cost)
    a0 = o.init_alpha(START, GOAL)
    mov = R.table(mc.CROSSING_P, mc.CROSSING_W)
    a_m, _, n_m = R.gd_single(a0, mov, START, GOAL, 200)
    a_f, _, n_f = R.gd_single(a0, mc.CROSSING_P, START, GOAL, 200)
    assert n_m == n_f == 200
    l_m, l_f = R.cost(a_m, mov, START, GOAL, *lam), R.cost(a_f, mov, START, GOAL, *lam)
    m_m, m_f = R.max_potential(a_m, mov), R.max_potential(a_f, mov)
    print(f"moving loss {l_m:.4f} vs frozen plan {l_f:.4f}; max potential {m_m:.4f} vs {m_f:.4f}")
    assert l_m <= 0.9 * l_f, (l_m, l_f)
    assert m_m <= 0.9 * m_f, (m_m, m_f)
    from irm_motion_planning_amd import _abi
    M, N = mc.CROSSING_M, int(p.n_timesteps)
    te = np.linspace(0, 1, M, dtype=np.float32)
    kq = np.zeros((M, N), np.float32)
    _abi.check(_abi.load_library().irm_query_matrices(N, float(p.rbf_variance), te.ctypes.data_as(_abi.c_float_p), M,
                                                      kq.ctypes.data_as(_abi.c_float_p), None))
    dense = []
    for a in (a_m, a_f):
        x, y, _, _ = R._fk(kq.astype(np.float64) @ a @ R.J)
        ox = float(mc.CROSSING_P[0, 0]) + te.astype(np.float64) * float(mc.CROSSING_W[0, 0])
        oy = float(mc.CROSSING_P[0, 1]) + te.astype(np.float64) * float(mc.CROSSING_W[0, 1])
        dense.append(float((0.8 / (0.5 + 0.5 * ((x - ox) ** 2 + (y - oy) ** 2))).max()))
    print(f"max potential on {M} times {dense[0]:.4f} vs {dense[1]:.4f}")
    assert dense[0] <= 0.9 * dense[1], dense


# ------------------------------------------------------------------------------------- header and binding
CTYPES_OF = {
    "irm_ctx*": ctypes.c_void_p, "const irm_ctx*": ctypes.c_void_p, "void*": ctypes.c_void_p,
    "const float*": "c_float_p", "float*": "c_float_p", "int32_t": ctypes.c_int32, "float": ctypes.c_float,
    "const irm_batch_dev*": "IrmBatchDev*", "irm_stats*": "IrmStats*", "irm_dense_report*": "IrmDenseReport*",
    "irm_launch_plan*": "IrmLaunchPlan*",
}
MOVING = ["irm_eval_cost_moving", "irm_eval_cost_grad_moving", "irm_optimize_batch_moving",
          "irm_optimize_batch_moving_dev", "irm_dense_check_moving", "irm_dense_check_moving_dev",
          "irm_optimize_plan_moving"]


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        words = arg.split()
        out.append(" ".join(words[:-1]))  # drop the parameter's name
    return out


def test_moving_symbols_are_bound_as_declared():
    from irm_motion_planning_amd import _abi
    from test_abi import declared_functions
    named = {"c_float_p": _abi.c_float_p, "IrmBatchDev*": ctypes.POINTER(_abi.IrmBatchDev),
             "IrmStats*": ctypes.POINTER(_abi.IrmStats), "IrmDenseReport*": ctypes.POINTER(_abi.IrmDenseReport),
             "IrmLaunchPlan*": ctypes.POINTER(_abi.IrmLaunchPlan)}
    lib = _abi.load_library()
    assert sorted(n for n in declared_functions() if "moving" in n) == sorted(MOVING)
    for name in MOVING:
        assert hasattr(lib, name), name
        res, args = _abi.PROTOTYPES[name]
        assert res is ctypes.c_int
        want = [CTYPES_OF[a] for a in _header_args(name)]
        want = [named.get(w, w) for w in want]
        assert args == want, (name, args, want)
    # each takes its static twin's arguments plus the velocity pointer (the plan: the same arguments)
    for name in MOVING:
        twin = _abi.PROTOTYPES[name.replace("_moving", "")][1]
        args = _abi.PROTOTYPES[name][1]
        if name == "irm_optimize_plan_moving":
            assert args == twin
        elif name.endswith("_dev"):
            assert args == twin[:-1] + [_abi.c_float_p, ctypes.c_void_p]  # velocity before the stream
        else:
            assert args == twin + [_abi.c_float_p]
    assert _abi.IRM_ABI_VERSION == 3 and re.search(r"#define IRM_ABI_VERSION 3\b", open(HEADER).read())


def test_cli_flag_defaults_to_absent():
    from conftest import ref_args
    assert ref_args().obstacle_velocity is None
    assert ref_args("--obstacle-velocity", "0.5", "-0.25").obstacle_velocity == [0.5, -0.25]
