"""Which C entry point a Context method reaches, and with what, without a GPU and without the library: a Context
made with Context.__new__ over a stand-in for the library that records every irm_* call.  For every combination
of obstacle velocity, end-effector goal and via-points (none, two, an empty ViaPoints) the entry point's name, the
number of arguments, which trailing arguments are NULL, the irm_via that is passed and the shape of what the
method returns are pinned — the dispatch stays what it is when the plumbing around it is rearranged.
"""
import ctypes
import itertools

import numpy as np
import pytest

from irm_motion_planning_amd import _abi
from irm_motion_planning_amd.clearance import CLEARANCE_REPORT_FIELDS
from irm_motion_planning_amd.context import Context, batch_dev
from irm_motion_planning_amd.via import IrmVia, ViaPoints

N, D, B, O, M = 8, 3, 2, 2, 5
ROWS, CART = [2, 5], [0, 1]
H = 0x1234  # the dummy context handle


def _describe(a, host):
    """What the stand-in keeps of one argument, taken while the caller's arrays are alive: None for NULL, the
    first float behind a host float pointer, the address of a device one, the fields of an irm_via passed by
    reference (with the first target value where the targets are host memory), a number as it is."""
    if a is None:
        return None
    if isinstance(a, _abi.c_float_p):
        if not a:
            return None
        return ("f32", float(a[0])) if host else ("addr", ctypes.cast(a, ctypes.c_void_p).value)
    if isinstance(a, ctypes.c_void_p):
        return a.value
    if isinstance(a, (int, float)):
        return a
    obj = getattr(a, "_obj", None)  # ctypes.byref(...)
    if isinstance(obj, IrmVia):
        first = float(ctypes.cast(obj.target, _abi.c_float_p)[0]) if host and obj.target else None
        return ("via", obj.n_via, list(obj.row[:obj.n_via]), list(obj.cartesian[:obj.n_via]), obj.target or 0, first)
    if obj is not None:
        return ("ref", type(obj).__name__)
    return ("obj", type(a).__name__) if a else None


class RecordingLib:
    """Every irm_* attribute is a callable that logs (name, described arguments) and returns 0; irm_eval_times
    returns M and irm_series_capacity 1.  The pointers of the *_dev entry points are device addresses: kept as
    numbers, never read."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if not name.startswith("irm_"):
            raise AttributeError(name)

        def fn(*args):
            self.log.append((name, [_describe(a, not name.endswith("_dev")) for a in args]))
            return {"irm_eval_times": M, "irm_series_capacity": 1}.get(name, 0)
        return fn


@pytest.fixture
def ctx():
    c = Context.__new__(Context)
    c.lib, c.N, c.D, c._h = RecordingLib(), N, D, ctypes.c_void_p(H)
    yield c
    c._h = ctypes.c_void_p()  # nothing to destroy


def _only_call(ctx):
    calls = [(n, a) for n, a in ctx.lib.log if n not in ("irm_eval_times", "irm_series_capacity")]
    assert len(calls) == 1, [n for n, _ in calls]
    name, args = calls[0]
    assert args[0] == H
    return name, args


VEL = np.array([[0.25, -0.5], [0.75, 1.5]], np.float32)
OBS = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32)
GXY = np.array([[0.5, 1.25], [-0.75, 2.0]], np.float32)
TARGETS = np.arange(1, 1 + 2 * D, dtype=np.float32).reshape(2, D)  # V×D, broadcast over the batch
ALPHA = np.zeros((B, N, D), np.float32)
START, GOAL = np.zeros((B, D), np.float32), np.ones((B, D), np.float32)


def _via(kind):
    return {"none": None, "two": ViaPoints(ROWS, CART, TARGETS), "empty": ViaPoints.empty()}[kind]


# all eight combinations of velocity, goal_xy and via-points present or absent, and the empty ViaPoints as a
# further state of each velocity / goal_xy combination
STATES = list(itertools.product([False, True], [False, True], ["none", "two", "empty"]))
IDS = [f"{'vel' if v else 'static'}-{'xy' if g else 'joint'}-via_{k}" for v, g, k in STATES]


def _suffix(vel, gxy, via):
    return "_via" if via == "two" else "_task" if gxy else "_moving" if vel else ""


def _tail(vel, gxy, via):
    """The trailing arguments of the cost, gradient and optimise families: a prefix of (vel, gxy, via)."""
    want = [("f32", float(VEL[0, 0])) if vel else None, ("f32", float(GXY[0, 0])) if gxy else None,
            ("via", 2, ROWS, CART)]
    return want[:{"": 0, "_moving": 1, "_task": 2, "_via": 3}[_suffix(vel, gxy, via)]]


def _check_tail(got, want, target_first=float(TARGETS[0, 0])):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w is not None and w[0] == "via":
            assert g[:4] == w and g[4] != 0 and g[5] == target_first  # a host target: B×V×D from TARGETS
        else:
            assert g == w


def _kw(vel, gxy, via, single=False):
    return dict(obstacle_velocity=VEL if vel else None, goal_xy=(GXY[0] if single else GXY) if gxy else None,
                via=_via(via))


@pytest.mark.parametrize("vel,gxy,via", STATES, ids=IDS)
def test_eval_cost(ctx, vel, gxy, via):
    out = ctx.eval_cost(ALPHA, OBS, START, GOAL, 0.5, 0.1, 0.25, **_kw(vel, gxy, via))
    name, args = _only_call(ctx)
    assert name == "irm_eval_cost" + _suffix(vel, gxy, via)
    assert args[5:10] == [O, B, 0.5, 0.1, 0.25]
    _check_tail(args[11:], _tail(vel, gxy, via))
    assert out.shape == (B,) and out.dtype == np.float32
    assert ctx.eval_cost(ALPHA[0], OBS, START[0], GOAL[0], 0.5, 0.1, 0.25, **_kw(vel, gxy, via, True)).shape == ()


@pytest.mark.parametrize("vel,gxy,via", STATES, ids=IDS)
def test_eval_cost_grad(ctx, vel, gxy, via):
    out = ctx.eval_cost_grad(ALPHA, OBS, START, GOAL, 0.5, 0.1, 0.25, with_cost=True, **_kw(vel, gxy, via))
    name, args = _only_call(ctx)
    assert name == "irm_eval_cost_grad" + _suffix(vel, gxy, via)
    assert args[5:10] == [O, B, 0.5, 0.1, 0.25]
    _check_tail(args[12:], _tail(vel, gxy, via))
    assert out[0].shape == (B, N, D) and out[1].shape == (B,)
    assert ctx.eval_cost_grad(ALPHA[0], OBS, START[0], GOAL[0], 0.5, 0.1, 0.25,
                              **_kw(vel, gxy, via, True)).shape == (N, D)


@pytest.mark.parametrize("gxy,via", [s[1:] for s in STATES if not s[0]], ids=[i[7:] for i, s in zip(IDS, STATES) if not s[0]])
def test_constraints(ctx, gxy, via):
    """No velocity; the _via form: goal_xy, the irm_via and the distance output; three values with a ViaPoints
    (an empty one: the existing call and a B×0 distance array), two without."""
    out = ctx.constraints(ALPHA, START, GOAL, goal_xy=GXY if gxy else None, via=_via(via))
    name, args = _only_call(ctx)
    assert name == "irm_constraints" + _suffix(False, gxy, via)
    assert args[4] == B
    want_gxy = ("f32", float(GXY[0, 0])) if gxy else None
    if via == "two":
        assert len(args) == 10 and args[7] == want_gxy and args[9] == ("f32", 0.0)
        _check_tail(args[8:9], [("via", 2, ROWS, CART)])
    else:
        assert args[7:] == ([want_gxy] if gxy else [])
    assert len(out) == (2 if via == "none" else 3)
    assert out[0].shape == (B,) and out[0].dtype == bool and out[1].shape == (B, 11)
    if via != "none":
        assert out[2].shape == (B, 2 if via == "two" else 0) and out[2].dtype == np.float32
    single = ctx.constraints(ALPHA[0], START[0], GOAL[0], goal_xy=GXY[0] if gxy else None, via=_via(via))
    assert len(single) == len(out) and isinstance(single[0], bool) and single[1].shape == (11,)
    if via != "none":
        assert single[2].shape == (2 if via == "two" else 0,)


@pytest.mark.parametrize("series", [False, True])
@pytest.mark.parametrize("vel,gxy,via", STATES, ids=IDS)
def test_optimize(ctx, vel, gxy, via, series):
    """With alpha0, so that via_seed is not entered."""
    out = ctx.optimize(START, GOAL, OBS, alpha0=ALPHA, series=series, **_kw(vel, gxy, via))
    name, args = _only_call(ctx)
    assert name == "irm_optimize_batch" + _suffix(vel, gxy, via)
    assert args[1] == ("f32", 0.0) and args[5:8] == [O, 0, B]
    assert (args[11] is not None) == series
    _check_tail(args[12:], _tail(vel, gxy, via))
    assert len(out) == (4 if series else 3)
    assert out[0].shape == out[1].shape == (B, N, D)
    assert set(out[2]) == set(_abi.STATS_FIELDS) and all(v.shape == (B,) for v in out[2].values())
    if series:
        assert out[3].shape == (B, 1, N, D)


def test_optimize_single_problem_and_per_problem_table(ctx):
    a, t, st = ctx.optimize(START[0], GOAL[0], OBS, alpha0=ALPHA[0])
    assert a.shape == t.shape == (N, D) and np.shape(st["final_loss"]) == ()
    ctx.lib.log.clear()
    per = np.stack([OBS, OBS + 1])
    ctx.optimize(START, GOAL, per, alpha0=ALPHA, obstacle_velocity=np.stack([VEL, VEL]), obstacle_stride=2 * O)
    name, args = _only_call(ctx)
    assert name == "irm_optimize_batch_moving" and args[5:8] == [O, 2 * O, B] and len(args) == 13


DEV = dict(vel=0x1000, gxy=0x2000, target=0x3000)  # device addresses: passed on, never read


@pytest.mark.parametrize("vel_from_batch", [False, True])
@pytest.mark.parametrize("vel,gxy,via", STATES, ids=IDS)
def test_optimize_dev(ctx, vel, gxy, via, vel_from_batch):
    """stream comes before the irm_via; the velocity table may ride on the batch (batch_dev's attribute)."""
    b = batch_dev(start=1, goal=2, batch=B, obstacle_velocity=DEV["vel"] if vel and vel_from_batch else 0)
    out = ctx.optimize_dev(b, stream=7, obstacle_velocity_dev=DEV["vel"] if vel and not vel_from_batch else 0,
                           goal_xy_dev=DEV["gxy"] if gxy else 0, via=_via(via), via_target_dev=DEV["target"])
    assert out is None
    name, args = _only_call(ctx)
    sfx = _suffix(vel, gxy, via)
    assert name == f"irm_optimize_batch{sfx}_dev"
    assert args[1] == ("ref", "IrmBatchDev")
    want_vel, want_gxy = ("addr", DEV["vel"]) if vel else None, ("addr", DEV["gxy"]) if gxy else None
    want = {"": [7], "_moving": [want_vel, 7], "_task": [want_vel, want_gxy, 7],
            "_via": [want_vel, want_gxy, 7, ("via", 2, ROWS, CART, DEV["target"], None)]}[sfx]
    assert args[2:] == want


@pytest.mark.parametrize("vel,gxy,via", STATES, ids=IDS)
def test_launch_plan(ctx, vel, gxy, via):
    """goal_xy wins over obstacle_velocity; the irm_via carries rows and kinds only."""
    out = ctx.launch_plan(B, n_obstacles=O, series=True, **_kw(vel, gxy, via))
    name, args = _only_call(ctx)
    assert name == "irm_optimize_plan" + _suffix(vel, gxy, via)
    assert args[1:5] == [B, O, 1, ("ref", "IrmLaunchPlan")]
    assert args[5:] == ([("via", 2, ROWS, CART, 0, None)] if via == "two" else [])
    assert set(out) == {n for n, _ in _abi.IrmLaunchPlan._fields_} and out["kernel"] == ""


@pytest.mark.parametrize("per_problem", [False, True])
@pytest.mark.parametrize("vel", [False, True])
def test_dense_check(ctx, vel, per_problem):
    obs, w = (np.stack([OBS, OBS + 1]), np.stack([VEL, VEL])) if per_problem else (OBS, VEL)
    out = ctx.dense_check(ALPHA, obs, with_cost=True, obstacle_velocity=w if vel else None)
    name, args = _only_call(ctx)
    assert name == "irm_dense_check" + ("_moving" if vel else "")
    assert args[3:6] == [O, 2 * O if per_problem else 0, B] and args[7] == ("f32", 0.0)
    assert args[8:] == ([("f32", float(VEL[0, 0]))] if vel else [])
    assert set(out) == set(_abi.DENSE_REPORT_FIELDS) | {"cost"}
    assert all(out[n].shape == (B,) for n in _abi.DENSE_REPORT_FIELDS) and out["cost"].shape == (B, M)
    assert {n for n in _abi.DENSE_REPORT_FIELDS if out[n].dtype == bool} == {"position_ok", "velocity_ok"}
    assert out["argmax_cost"].dtype == np.int32 and out["max_cost"].dtype == np.float32
    single = ctx.dense_check(ALPHA[0], OBS)
    assert set(single) == set(_abi.DENSE_REPORT_FIELDS) and all(np.shape(v) == () for v in single.values())


@pytest.mark.parametrize("vel", [False, True])
def test_clearance(ctx, vel):
    out = ctx.clearance(ALPHA, OBS, obstacle_velocity=VEL if vel else None, obstacle_radius=0.5, with_samples=True)
    name, args = _only_call(ctx)
    assert name == "irm_clearance" and len(args) == 13
    assert args[3:5] == [O, 0] and args[5] == (("f32", float(VEL[0, 0])) if vel else None)
    assert args[6] == ("f32", 0.5) and args[7:9] == [0.0, B] and args[11:] == [None, None]
    assert set(out) == set(CLEARANCE_REPORT_FIELDS) | {"clearance"}
    assert all(out[n].shape == (B,) for n in CLEARANCE_REPORT_FIELDS) and out["clearance"].shape == (B, M)
    assert {n for n in CLEARANCE_REPORT_FIELDS if out[n].dtype == bool} == {"collision_free"}


def _call(ctx, method, obs, **kw):
    if method == "optimize":
        return ctx.optimize(START, GOAL, obs, alpha0=ALPHA, **kw)
    return getattr(ctx, method)(ALPHA, obs, **kw)


@pytest.mark.parametrize("method", ["dense_check", "clearance", "optimize"])
def test_obstacle_table_errors(ctx, method):
    with pytest.raises(ValueError) as e:
        _call(ctx, method, np.zeros((3, O, 2), np.float32))
    assert str(e.value) == "per-problem obstacles must be (2, O, 2), got (3, 2, 2)"
    with pytest.raises(ValueError) as e:
        _call(ctx, method, np.zeros((B, O, 3), np.float32))
    assert str(e.value) == "per-problem obstacles must be (2, O, 2), got (2, 2, 3)"
    with pytest.raises(ValueError) as e:
        _call(ctx, method, np.zeros((O, 3), np.float32))
    assert str(e.value) == "shared obstacles must be (O, 2), got (2, 3)"
    with pytest.raises(ValueError) as e:
        _call(ctx, method, OBS, obstacle_velocity=np.zeros((3, 2), np.float32))
    assert str(e.value) == "obstacle_velocity must have the obstacles' shape (2, 2), got (3, 2)"
    assert ctx.lib.log == [] or all(n == "irm_eval_times" for n, _ in ctx.lib.log)


def test_optimize_obstacle_stride_errors(ctx):
    with pytest.raises(ValueError) as e:
        ctx.optimize(START, GOAL, np.zeros((B, O, 2), np.float32), alpha0=ALPHA, obstacle_stride=5)
    assert str(e.value) == "obstacle_stride 5 does not match obstacles (2, 2, 2)"
    with pytest.raises(ValueError) as e:
        ctx.optimize(START, GOAL, OBS, alpha0=ALPHA, obstacle_stride=4)
    assert str(e.value) == "obstacle_stride needs per-problem obstacles of shape (B, O, 2)"
    with pytest.raises(ValueError) as e:
        ctx.optimize(START, None, OBS, alpha0=ALPHA)
    assert str(e.value) == "optimize() needs a goal configuration or a goal_xy"
    assert ctx.lib.log == []


def test_empty_obstacle_table_is_no_obstacle(ctx):
    ctx.dense_check(ALPHA, np.zeros((0, 2), np.float32))
    assert _only_call(ctx)[1][3:5] == [0, 0]
