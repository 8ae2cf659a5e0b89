"""Via-points without a GPU: the fp64 restatement the GPU tests measure against (tests/via_cases.py) is checked
against finite differences of itself, shown to be its parent with an empty via list, and shown to tell the
mutants a via bug would give from the right answer on the GPU tests' scenes; the end-to-end scenes are shown to
be decided by the algorithm (fp64 BLS from the seed recipe and from perturbed seeds); the value object, the CLI
flags and the new C symbols are checked.
"""
import ctypes
import re

import numpy as np
import pytest

import moving_cases as mc
import task_cases as tc
import via_cases as vc
from conftest import START, GOAL, obstacles, ref_args
from test_abi import HEADER
from test_moving_host import CTYPES_OF, _header_args
from variant_shape_cases import COST_RTOL, FORWARD, GRAD_RTOL, MUTANT_FACTOR

SHAPES = [(33, 3), (40, 7)]
LAM = (5.0, 0.1)  # λsg after one escalation of the dual loop: a via-point 0.2 away then weighs 0.1 in the cost


def _problem(o, D, seed):
    return tuple(x[0] for x in mc.well_conditioned_alpha(o, 1, D, seed=seed))


def mixed_rows(N):
    """V = 4 mixed: rows (1, m, m+1, N−2) — adjacent rows and both extremes — kinds joint, xy, joint, xy."""
    m = N // 2
    return [1, m, m + 1, N - 2], [0, 1, 0, 1]


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("lmax", [0.0, 0.25])
@pytest.mark.parametrize("N,D", SHAPES)
def test_restatement_gradient_is_the_derivative_of_its_cost(N, D, lmax, whole):
    """Central finite differences (h = 1e-6) of the via cost in fp64 against cost_g, 1e-6 relative to max|G|,
    with a joint and an end-effector goal; and the via cost lies above the via-free one by the via terms."""
    R0, o = vc.restatement(*mc.shape_argv(N, D), whole_robot=whole)
    alpha, s, g = _problem(o, D, 11 * N + D)
    rows, cart = mixed_rows(N)
    R = R0.with_via(vc.entries(rows, cart, vc.near_targets(R0, alpha, rows, cart, seed=N)))
    p, _ = mc.crossing_tables(1, 11, 2.0, seed=N + D)
    links = [o.params.link_length[i] for i in range(D)]
    for goal in (g, tc.TaskGoal(tc.fk64(links, g) + np.array([0.3, -0.2]))):
        lam = (*LAM, lmax)
        G = R.cost_g(alpha, p[0], s, goal, *lam)
        a = alpha.astype(np.float64)
        rng = np.random.default_rng(N)
        h = 1e-6
        idx = [(int(rng.integers(N)), int(rng.integers(D))) for _ in range(12)]
        idx += [(m, d) for m in rows for d in range(D)]
        for n, d in idx:
            ap, am = a.copy(), a.copy()
            ap[n, d] += h
            am[n, d] -= h
            fd = (R.cost(ap, p[0], s, goal, *lam) - R.cost(am, p[0], s, goal, *lam)) / (2 * h)
            assert abs(fd - G[n, d]) <= 1e-6 * np.abs(G).max(), (n, d, fd, G[n, d])
        free = R0.cost(a, p[0], s, goal, *lam)
        # (four targets at least 0.1 away: λsg·½·Σ r² ≥ 5·0.5·4·0.01)
        assert R.cost(a, p[0], s, goal, *lam) - free > 0.099


def test_empty_via_list_is_the_parent_to_the_bit():
    R, o = vc.restatement(*mc.shape_argv(33, 3))
    P = tc.TaskRef64(o.params, *o.kernel_matrices())
    alpha, s, g = _problem(o, 3, 5)
    obs = obstacles()
    for goal in (g, tc.TaskGoal([1.0, 2.0])):
        assert R.cost(alpha, obs, s, goal, 0.5, 0.1, 0.25) == P.cost(alpha, obs, s, goal, 0.5, 0.1, 0.25)
        np.testing.assert_array_equal(R.cost_g(alpha, obs, s, goal, 0.5, 0.1, 0.25),
                                      P.cost_g(alpha, obs, s, goal, 0.5, 0.1, 0.25))
        ok0, rep0 = R.constraints(alpha, s, goal)
        ok1, rep1 = P.constraints(alpha, s, goal)
        assert ok0 == ok1
        np.testing.assert_array_equal(rep0, rep1)


# ------------------------------------------------------------------------------------------ mutants
def forward_via_cases():
    """(N, D, whole, rows, kinds) of the GPU cost / gradient test (tests/test_gpu_via.py, test 2).  The request
    for this feature named rows 63 and 64 at N = 65; row 64 is N−1 there, the goal row, which no via-point may
    name, so that case is replaced by rows (62, 63) — see the comment below."""
    out = []
    for N, D, whole in ((33, 3, 0), (64, 3, 0), (40, 7, 0), (33, 3, 1)):
        out += [(N, D, whole, (N // 2,), (0,)), (N, D, whole, (N // 2,), (1,)), (N, D, whole, *map(tuple, mixed_rows(N)))]
    # multi-wave shapes.  N = 65: row 63 is the last lane of wave 0 and the neighbour of row N−1 = 64, the only valid
    # lane of wave 1 (64 itself is the goal row: via rows end at N−2); N = 129: rows 64 and 127 = N−2
    out += [(65, 3, 0, (62, 63), (1, 0)), (129, 3, 0, (64, 127), (0, 1)), (128, 7, 0, (63, 64), (1, 0)),
            (256, 3, 0, (64, 128, 191, 254), (0, 1, 1, 0))]
    return out


def forward_batch(N, D):
    """(B, TB) of an eval_cost(_grad) call: FORWARD's where it has the shape, else one full workgroup and a
    ragged one of the largest TB (min(16/D, threads/NW))."""
    if (N, D) in FORWARD:
        return FORWARD[(N, D)]
    tb = min(16 // D, (512 if D >= 5 else 1024) // 64)
    return tb + 2, tb


def forward_via_scene(N, D, whole, rows, cart):
    """B problems of one call: well-conditioned α, different targets per problem 0.2 – 0.3 from the row."""
    R, o = vc.forward_restatement(N, D, bool(whole))
    B, TB = forward_batch(N, D)
    alpha, s, g = mc.well_conditioned_alpha(o, B, D, seed=N + D)
    targets = np.stack([vc.near_targets(R, alpha[b], rows, cart, seed=31 * N + b, lo=0.2, hi=0.3) for b in range(B)])
    O = 13 if N in (64, 129) else 11
    p, w = mc.crossing_tables(1, O, 2.0, seed=N)
    return dict(N=N, D=D, B=B, TB=TB, alpha=alpha, s=s, g=g, targets=targets, p=p[0], w=w[0], rows=list(rows),
                cart=list(cart))


def forward_via_reference(sc, R, lam, via_class=None, goal_xy=None, table=None):
    cost, grad = np.zeros(sc["B"]), np.zeros(sc["alpha"].shape)
    for b in range(sc["B"]):
        Rb = R.with_via(vc.entries(sc["rows"], sc["cart"], sc["targets"][b]))
        if via_class is not None:
            Rb = via_class(Rb)
        goal = sc["g"][b] if goal_xy is None else tc.TaskGoal(goal_xy[b])
        tb = sc["p"] if table is None else table
        cost[b] = Rb.cost(sc["alpha"][b], tb, sc["s"][b], goal, *lam)
        grad[b] = Rb.cost_g(sc["alpha"][b], tb, sc["s"][b], goal, *lam)
    return cost, grad


@pytest.mark.parametrize("N,D,whole,rows,cart", forward_via_cases())
def test_forward_scenes_tell_the_mutants_apart(N, D, whole, rows, cart):
    """On every scene of the GPU cost / gradient test each mutant — via term on row m_v ± 1, a velocity term on
    the via row, the via term dropped, Cartesian read as joint — lies at least MUTANT_FACTOR device bounds from the
    restatement in cost or gradient, for every problem; and the via-points move each cost by > 2e-3 relative."""
    sc = forward_via_scene(N, D, whole, rows, cart)
    R, _ = vc.forward_restatement(N, D, bool(whole))
    for lmax in (0.0, 0.25):
        lam = (*LAM, lmax)
        cost, grad = forward_via_reference(sc, R, lam)
        names = vc.mutants(R.with_via(vc.entries(rows, cart, sc["targets"][0])))
        for name in names:
            mcost, mgrad = forward_via_reference(sc, R, lam, via_class=lambda Rb, name=name: vc.mutants(Rb)[name])
            dc = np.abs(mcost - cost) / np.abs(cost)
            dg = np.abs(mgrad - grad).reshape(sc["B"], -1).max(1) / np.abs(grad).reshape(sc["B"], -1).max(1)
            far = (dc >= MUTANT_FACTOR * COST_RTOL) | (dg >= MUTANT_FACTOR * GRAD_RTOL)
            print(f"N={N} D={D} whole={whole} rows={rows} lmax={lmax} {name}: cost rel {dc.min():.1e} … {dc.max():.1e}, "
                  f"gradient {dg.min():.1e} … {dg.max():.1e}·max|G|")
            assert far.all(), (name, dc, dg)
            if name == "dropped":
                assert np.all(dc > 2e-3), dc


# ------------------------------------------------------------------------------------------ end to end
def _seed64(R, o, via, ridge=1e-6):
    rows, knots = vc.seed_knots(o, START, GOAL, via)
    return vc.ridge_fit64(R, vc.via_path(R.t, rows, knots, np.float64), ridge)


@pytest.mark.parametrize("name", sorted(vc.E2E_SCENES))
@pytest.mark.parametrize("N", vc.E2E_N)
def test_e2e_scenes_are_decided_by_the_algorithm(N, name):
    """Every Cartesian scene of the GPU end-to-end test reaches `constraints ok` in the fp64 BLS restatement
    (default hyper-parameters) from the via_seed recipe and from three seeds perturbed by 1e-5 relative; the
    free plan of the same problem misses a via target by more than 0.4, and the via row is crossed at speed."""
    R0, o = vc.restatement("--n-timesteps", N)
    rows, cart, tg = vc.e2e_via(name, N)
    R = R0.with_via(vc.entries(rows, cart, tg))
    a0 = _seed64(R, o, R.via)
    rng = np.random.default_rng(N)
    seeds = [a0] + [a0 * (1 + 1e-5 * rng.standard_normal(a0.shape)) for _ in range(3)]
    for k, a in enumerate(seeds):
        alpha, ok, outers, inners = R.bls(a, obstacles(), START, GOAL)
        d = R.via_dist(alpha)
        speed = [float(np.linalg.norm(R.traj_vel(alpha)[1][m])) for m in rows]
        print(f"N={N} {name} seed {k}: ok={ok} outer={outers} inner={inners} via dist {d} speed {speed}")
        assert ok, (N, name, k, d)
        assert (d < o.params.eps_position).all() and min(speed) > 1.0
    free, _, _, _ = R0.bls(o.init_alpha(START, GOAL), obstacles(), START, GOAL)
    miss = R.with_via(R.via).via_dist(free)
    print(f"N={N} {name}: the free plan misses by {miss}")
    assert miss.max() > 0.4


@pytest.mark.parametrize("N", vc.E2E_N)
def test_joint_via_point_is_reached_in_fp64(N):
    """The joint via-point of the GPU end-to-end test: via distance below eps_position (the flag is printed, not
    asserted: detours through a joint configuration can end on another sub-flag)."""
    R0, o = vc.restatement("--n-timesteps", N)
    R = R0.with_via(vc.entries([N // 2], [0], vc.E2E_JOINT[None]))
    alpha, ok, outers, _ = R.bls(_seed64(R, o, R.via), obstacles(), START, GOAL)
    d = R.via_dist(alpha)
    print(f"N={N} joint via-point: ok={ok} outer={outers} via dist {d}")
    assert d[0] < o.params.eps_position


def test_seed_recipe_passes_near_the_via_points():
    """The ridge fit rounds the kinks: the seed's own via distances stay below 0.05."""
    for N in vc.E2E_N:
        R0, o = vc.restatement("--n-timesteps", N)
        for name in vc.E2E_SCENES:
            rows, cart, tg = vc.e2e_via(name, N)
            R = R0.with_via(vc.entries(rows, cart, tg))
            d = R.via_dist(_seed64(R, o, R.via))
            print(N, name, d)
            assert d.max() < 0.05


# ------------------------------------------------------------------------------------------ the value object
def test_via_points_validation_and_time_snapping():
    from irm_motion_planning_amd.via import MAX_VIA, ViaPoints, snap_times
    assert MAX_VIA == 4
    v = ViaPoints([3, 7], [0, 1], np.zeros((2, 3)))
    assert len(v) == 2 and v.rows == [3, 7] and v.cartesian == [0, 1]
    assert v.padded(5, 3).shape == (5, 2, 3) and v.padded(5, 3).dtype == np.float32
    per = ViaPoints([3], [1], np.arange(8, dtype=np.float32).reshape(4, 1, 2))
    assert per.padded(4, 3).shape == (4, 1, 3) and per.padded(4, 3)[2, 0].tolist() == [4.0, 5.0, 0.0]
    assert len(ViaPoints.empty()) == 0 and ViaPoints.empty().padded(2, 3).shape == (2, 0, 3)
    for bad in (lambda: ViaPoints([3, 3], [0, 0], np.zeros((2, 3))), lambda: ViaPoints([5, 3], [0, 0], np.zeros((2, 3))),
                lambda: ViaPoints([0], [0], np.zeros((1, 3))), lambda: ViaPoints([1, 2, 3, 4, 5], [0] * 5, np.zeros((5, 3))),
                lambda: ViaPoints([3], [2], np.zeros((1, 3))), lambda: ViaPoints([3], [0, 1], np.zeros((1, 3))),
                lambda: ViaPoints([3, 4], [0, 0], np.zeros((3, 3))), lambda: ViaPoints([3], [0], np.zeros(3)),
                lambda: v.padded(5, 4), lambda: ViaPoints([3], [0], np.zeros((2, 1, 3))).padded(5, 3),
                lambda: ViaPoints([31], [0], np.zeros((1, 3))).check_rows(32)):
        with pytest.raises(ValueError):
            bad()
    ViaPoints([30], [0], np.zeros((1, 3))).check_rows(32)
    # snapping: the nearest support row of linspace(0, 1, N), clamped into [1, N−2]
    assert snap_times(33, [0.5]) == [16] and snap_times(33, [0.25, 0.75]) == [8, 24]
    assert snap_times(50, [1 / 3, 2 / 3]) == [16, 33]
    assert snap_times(33, [0.001, 0.999]) == [1, 31]
    assert snap_times(33, [0.26]) == [8] and snap_times(33, [0.27]) == [9]
    at = ViaPoints.at_times(33, [0.5], [1], np.array([[2.4, 1.2]], np.float32))
    assert at.rows == [16] and at.padded(1, 3)[0, 0].tolist() == [np.float32(2.4), np.float32(1.2), 0.0]
    for bad in ([0.5, 0.51], [0.0], [1.0], [0.6, 0.4]):
        with pytest.raises(ValueError):
            snap_times(33, bad)


def test_cli_flags_parse_and_default_to_absent():
    from irm_motion_planning_amd.via import via_from_args
    a = ref_args()
    assert a.via_joint is None and a.via_xy is None and via_from_args(a, 50, 3) is None
    a = ref_args("--via-xy", "0.5", "2.4", "1.2")
    assert a.via_xy == [[0.5, 2.4, 1.2]]
    v = via_from_args(a, 33, 3)
    assert v.rows == [16] and v.cartesian == [1] and v.targets.tolist() == [[np.float32(2.4), np.float32(1.2), 0.0]]
    a = ref_args("--via-xy", "0.75", "1.0", "2.2", "--via-joint", "0.25", "0.2", "1.0", "-0.3", "--via-xy", "0.5", "2.4", "1.2")
    v = via_from_args(a, 33, 3)
    assert v.rows == [8, 16, 24] and v.cartesian == [0, 1, 1]
    np.testing.assert_array_equal(v.targets[0], np.array([0.2, 1.0, -0.3], np.float32))
    with pytest.raises(ValueError):
        via_from_args(ref_args("--via-joint", "0.25", "0.2", "1.0"), 33, 3)


# ------------------------------------------------------------------------------------- header and binding
VIA = ["irm_eval_cost_via", "irm_eval_cost_grad_via", "irm_constraints_via", "irm_optimize_batch_via",
       "irm_optimize_batch_via_dev", "irm_optimize_plan_via"]
ARGC = {"irm_eval_cost_via": 14, "irm_eval_cost_grad_via": 15, "irm_constraints_via": 10, "irm_optimize_batch_via": 15,
        "irm_optimize_batch_via_dev": 6, "irm_optimize_plan_via": 6}


def test_via_symbols_are_bound_as_declared():
    """The library exports every irm_*_via symbol, bound with the header's argument list: the _task form plus a
    trailing irm_via* (irm_constraints_via: plus the via distances)."""
    from irm_motion_planning_amd import _abi
    from irm_motion_planning_amd.via import IrmVia
    from test_abi import declared_functions
    via_p = ctypes.POINTER(IrmVia)
    named = {"c_float_p": _abi.c_float_p, "IrmBatchDev*": ctypes.POINTER(_abi.IrmBatchDev),
             "IrmStats*": ctypes.POINTER(_abi.IrmStats), "IrmLaunchPlan*": ctypes.POINTER(_abi.IrmLaunchPlan),
             "uint8_t*": _abi.c_uint8_p, "IrmVia*": via_p}
    ctypes_of = dict(CTYPES_OF, **{"uint8_t*": "uint8_t*", "const irm_via*": "IrmVia*"})
    lib = _abi.load_library()
    declared = declared_functions()
    assert sorted(n for n in declared if n.endswith("_via") or n.endswith("_via_dev")) == sorted(VIA)
    P, fp = _abi.PROTOTYPES, _abi.c_float_p
    for name in VIA:
        assert hasattr(lib, name), name
        res, args = P[name]
        assert res is ctypes.c_int and len(args) == ARGC[name] == len(_header_args(name))
        want = [named.get(w, w) for w in (ctypes_of[a] for a in _header_args(name))]
        assert args == want, (name, args, want)
    assert P["irm_eval_cost_via"][1] == P["irm_eval_cost_task"][1] + [via_p]
    assert P["irm_eval_cost_grad_via"][1] == P["irm_eval_cost_grad_task"][1] + [via_p]
    assert P["irm_constraints_via"][1] == P["irm_constraints_task"][1] + [via_p, fp]
    assert P["irm_optimize_batch_via"][1] == P["irm_optimize_batch_task"][1] + [via_p]
    assert P["irm_optimize_batch_via_dev"][1] == P["irm_optimize_batch_task_dev"][1] + [via_p]
    assert P["irm_optimize_plan_via"][1] == P["irm_optimize_plan_task"][1] + [via_p]
    src = open(HEADER).read()
    assert _abi.IRM_ABI_VERSION == 3 and re.search(r"#define IRM_ABI_VERSION 3\b", src)
    assert re.search(r"#define IRM_MAX_VIA 4\b", src)


def test_irm_via_layout_matches_the_header(tmp_path):
    import os
    import subprocess
    from conftest import REPO
    from irm_motion_planning_amd.via import IrmVia
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "irm.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(irm_via), offsetof(irm_via, n_via), offsetof(irm_via, row),\n'
                   '         offsetof(irm_via, cartesian), offsetof(irm_via, target));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(IrmVia), IrmVia.n_via.offset, IrmVia.row.offset, IrmVia.cartesian.offset,
                   IrmVia.target.offset]
