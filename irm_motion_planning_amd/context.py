"""numpy-facing wrapper of one irm_ctx (include/irm.h).

`Context` owns a device context for one (N, D, hyper-parameter) configuration
— the analogue of one reference `Trajectory` + optimizer object
(trajectory.py:23-42, optimizer_GD.py:15-51, optimizer_BLS.py:23-54).  Every
method calls a HIP kernel through the C ABI; there is no host fallback.
"""
import ctypes

import numpy as np

from . import _abi
from ._abi import IrmBatchDev, IrmDenseReport, IrmInfo, IrmLaunchPlan, IrmParams, IrmStats, check, load_library
from .clearance import (CLEARANCE_REPORT_FIELDS, SELF_CLEARANCE_REPORT_FIELDS, IrmClearanceReport,
                        IrmSelfClearanceReport, self_pairs)
from .multistart import IRM_MAX_SEEDS, IrmMultistart, IrmMultistartOut
from .via import IrmVia, ViaPoints

_fp = _abi.c_float_p


def _struct_dtype(cls):
    """The numpy record dtype of a ctypes struct of float / int32 fields."""
    return np.dtype([(name, np.float32 if ctype is ctypes.c_float else np.int32) for name, ctype in cls._fields_])


_STATS_DTYPE = _struct_dtype(IrmStats)
_REPORT_DTYPE = _struct_dtype(IrmClearanceReport)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_fp)


def _dev(addr):
    """A raw device address as the float* the *_dev entry points take (0 / None: NULL)."""
    return ctypes.cast(ctypes.c_void_p(int(addr) if addr else None), _fp)


_SUFFIX = ("", "_moving", "_task", "_via")  # an entry point's twins, each the one before it plus one trailing argument


def _rank(has_velocity, has_goal_xy, has_via):
    """Which twin a call reaches (an index into _SUFFIX): via-points select _via, else an end-effector goal _task,
    else a velocity table _moving, else the entry point itself."""
    return 3 if has_via else 2 if has_goal_xy else 1 if has_velocity else 0


def _via_struct(via, target):
    """The irm_via of a ViaPoints' rows and kinds; target: the address of the targets (B×V×D fp32), None: NULL."""
    v = IrmVia()
    v.n_via = len(via)
    for i, (r, c) in enumerate(zip(via.rows, via.cartesian)):
        v.row[i], v.cartesian[i] = r, c
    v.target = target
    return v


def _report(rep, fields, as_bool, single):
    """An array of report structs (float / int32 fields) as a dict of arrays, one per name of `fields`; those of
    `as_bool` as bool."""
    recs = np.frombuffer(rep, dtype=np.dtype(
        [(name, np.float32 if ctype is ctypes.c_float else np.int32) for name, ctype in rep._type_._fields_]))
    out = {}
    for name in fields:
        vals = recs[name].copy()
        if name in as_bool:
            vals = vals.astype(bool)
        out[name] = vals[0] if single else vals
    return out


def fit_operator(n_timesteps, rbf_variance=0.1, ridge=_abi.IRM_FIT_RIDGE_DEFAULT, n_src=0, rbf_variance_src=None,
                 t0=0.0, t1=1.0):
    """The fp64 operators of fit_alpha / transfer_alpha as the library builds them (irm_fit_operator; host only, no
    context, no device): W = (K + ρI)⁻¹ (N×N) for n_src = 0, else T = W·Kx (N×n_src) for the source grid
    linspace(0, 1, n_src), its kernel width (None: rbf_variance) and the time map [0, 1] → [t0, t1]."""
    lib = load_library()
    N, M = int(n_timesteps), int(n_src)
    out = np.zeros((max(N, 0), max(M, 0) if M else max(N, 0)), np.float64)
    if out.size == 0:
        out = np.zeros((1, 1), np.float64)  # (bad sizes: the library refuses them before it writes)
    var_src = -1.0 if rbf_variance_src is None else float(rbf_variance_src)
    check(lib.irm_fit_operator(N, float(rbf_variance), float(ridge), M, var_src, float(t0), float(t1),
                               out.ctypes.data_as(_abi.c_double_p)))
    return out


def stats_to_dict(stats):
    out = {name: np.array([getattr(s, name) for s in stats]) for name in _abi.STATS_FIELDS}
    return out


def default_jac(n_joints, jac_gaussian_mean=0.15, seed=0):
    """J = I + jgm·normal(PRNGKey(seed), (D, D)) — trajectory.py:42."""
    lib = load_library()
    out = np.zeros(n_joints * n_joints, np.float32)
    check(lib.irm_default_jac(n_joints, float(jac_gaussian_mean), seed, _ptr(out)))
    return out.reshape(n_joints, n_joints)


def parse_work_queue(groups):
    """irm_set_work_queue's argument from "off" / "auto" / a count (int or decimal string)."""
    if isinstance(groups, str):
        word = groups.strip().lower()
        if word == "off":
            return 0
        if word == "auto":
            return -1
        if not word.isdigit():
            raise ValueError(f"work queue must be 'off', 'auto' or a workgroup count, got {groups!r}")
        return int(word)
    return int(groups)


def default_params():
    p = IrmParams()
    load_library().irm_params_default(ctypes.byref(p))
    return p


class Context:
    def __init__(self, params):
        self.lib = load_library()
        self.params = params
        self.N, self.D = int(params.n_timesteps), int(params.n_joints)
        h = ctypes.c_void_p()
        check(self.lib.irm_ctx_create(ctypes.byref(h), ctypes.byref(params)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.irm_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------- queries
    def info(self):
        inf = IrmInfo()
        check(self.lib.irm_get_info(self._h, ctypes.byref(inf)))
        d = {name: getattr(inf, name) for name, _ in IrmInfo._fields_}
        d["device_name"] = d["device_name"].decode()
        d["arch"] = d["arch"].decode()
        d["build_id"] = d["build_id"].decode()
        return d

    def launch_plan(self, batch, n_obstacles=0, series=False, obstacle_velocity=None, goal_xy=None, via=None):
        """The optimiser launch optimize() runs for `batch` problems (irm_optimize_plan: filled in by
        the library's own launch dispatch, nothing launched).  obstacle_velocity not None: the launch of
        a moving call (irm_optimize_plan_moving; only whether it is given matters).  goal_xy not None: the
        launch of an end-effector-goal call (irm_optimize_plan_task; the same general kernel).  via (a
        ViaPoints; only its rows and kinds matter): the launch of a via call (irm_optimize_plan_via; the same
        general kernel); None or an empty one: the launch without via-points.  The via plan, like the
        end-effector-goal plan, is described with static obstacles: with obstacle_velocity as well the real launch
        runs the same kernel with a second obstacle table in LDS (a larger lds_bytes, possibly a smaller
        traj_per_block)."""
        pl = IrmLaunchPlan()
        n = _rank(obstacle_velocity is not None, goal_xy is not None, via is not None and len(via))
        tail = ()
        if n == 3:
            via.check_rows(self.N)
            tail = (ctypes.byref(_via_struct(via, None)),)
        check(getattr(self.lib, "irm_optimize_plan" + _SUFFIX[n])(self._h, int(batch), int(n_obstacles),
                                                                  int(bool(series)), ctypes.byref(pl), *tail))
        d = {name: getattr(pl, name) for name, _ in IrmLaunchPlan._fields_}
        d["kernel"] = d["kernel"].decode()
        return d

    def set_work_queue(self, groups):
        """Work-queue scheduling of every later optimize() on this context (irm_set_work_queue):
        "off" / 0, "auto", or the number of persistent workgroups.  Results do not depend on it."""
        check(self.lib.irm_set_work_queue(self._h, parse_work_queue(groups)))

    def work_queue_groups(self, batch, n_obstacles=0, series=False):
        """Persistent workgroups of the launch optimize() runs for `batch` problems, 0 for the static
        launch (irm_work_queue_groups: the library's own dispatch, nothing launched)."""
        n = self.lib.irm_work_queue_groups(self._h, int(batch), int(n_obstacles), int(bool(series)))
        if n < 0:
            check(n)
        return int(n)

    def kernel_matrices(self):
        N, D = self.N, self.D
        t = np.zeros(N, np.float32)
        K = np.zeros((N, N), np.float32)
        dK = np.zeros((N, N), np.float32)
        J = np.zeros((D, D), np.float32)
        check(self.lib.irm_kernel_matrices(self._h, _ptr(t), _ptr(K), _ptr(dK), _ptr(J)))
        return t, K, dK, J

    def series_capacity(self):
        return int(self.lib.irm_series_capacity(self._h))

    # ---------------------------------------------------------- batched ops
    def _batch(self, a, tail):
        a = _f32(a)
        single = a.ndim == len(tail)
        if single:
            a = a[None]
        return a, single

    def init_alpha(self, start, goal):
        s, single = self._batch(start, (self.D,))
        g, _ = self._batch(goal, (self.D,))
        out = np.zeros((s.shape[0], self.N, self.D), np.float32)
        check(self.lib.irm_init_alpha(self._h, _ptr(s), _ptr(g), s.shape[0], _ptr(out)))
        return out[0] if single else out

    def evaluate(self, alpha, which=0):
        a, single = self._batch(alpha, (self.N, self.D))
        out = np.zeros_like(a)
        check(self.lib.irm_evaluate(self._h, _ptr(a), a.shape[0], int(which), _ptr(out)))
        return out[0] if single else out

    # ------------------------------------------- evaluation at arbitrary times
    def set_eval_times(self, t):
        """The M times that eval_any / dense_check evaluate at (irm_set_eval_times: builds and uploads the
        query matrices; replaces the previous grid).  Any finite times, in any order."""
        t = _f32(t).reshape(-1)
        check(self.lib.irm_set_eval_times(self._h, _ptr(t), t.shape[0]))

    def eval_times(self):
        """The evaluation times currently set (empty if none)."""
        m = self.lib.irm_eval_times(self._h, None)
        if m < 0:
            check(m)
        t = np.zeros(m, np.float32)
        if m:
            self.lib.irm_eval_times(self._h, _ptr(t))
        return t

    def eval_any(self, alpha, which=0):
        """Positions (which 0) or velocities (which 1) at the evaluation times, (B×)M×D — trajectory.py:68-70."""
        a, single = self._batch(alpha, (self.N, self.D))
        M = int(self.lib.irm_eval_times(self._h, None))
        out = np.zeros((a.shape[0], max(M, 0), self.D), np.float32)
        check(self.lib.irm_eval_any(self._h, _ptr(a), a.shape[0], int(which), _ptr(out)))
        return out[0] if single else out

    def dense_check(self, alpha, obstacles, with_cost=False, obstacle_velocity=None):
        """Obstacle cost, joint and velocity limits on the evaluation times (irm_dense_check): a dict of
        arrays named as irm_dense_report's fields, plus `cost` ((B×)M per-sample cost) with with_cost.
        obstacles: (O, 2) shared, or (B, O, 2) one table per problem, like optimize.
        obstacle_velocity (the shape of obstacles): sample i sees obstacle o at p + t_eval[i]·w
        (irm_dense_check_moving)."""
        a, single = self._batch(alpha, (self.N, self.D))
        B = a.shape[0]
        obs, O, stride = self._obstacle_table(obstacles, B)
        M = int(self.lib.irm_eval_times(self._h, None))
        rep = (IrmDenseReport * B)()
        cost = np.zeros((B, max(M, 0)), np.float32) if with_cost else None
        suffix, tail, _keep = self._variant(obstacle_velocity, None, None, obs, B)
        check(getattr(self.lib, "irm_dense_check" + suffix)(self._h, _ptr(a), _ptr(obs), O, stride, B, rep, _ptr(cost),
                                                            *tail))
        out = _report(rep, _abi.DENSE_REPORT_FIELDS, ("position_ok", "velocity_ok"), single)
        if with_cost:
            out["cost"] = cost[0] if single else cost
        return out

    def clearance(self, alpha, obstacles, obstacle_velocity=None, obstacle_radius=None, link_radius=0.0,
                  with_samples=False, with_links=False, with_joints=False):
        """Signed clearance between the arm's links (segments between consecutive joints, each a capsule of
        link_radius) and disc obstacles on the evaluation times (irm_clearance): a dict of arrays named as
        irm_clearance_report's fields, plus `clearance` ((B×)M: every sample's minimum), `link_clearance` ((B×)D:
        every link's own minimum) and `joints` ((B×)M×D×2: the joint positions of every sample) on request.
        obstacles: (O, 2) shared, or (B, O, 2) one table per problem, like dense_check; obstacle_velocity the same
        shape (sample i sees obstacle o at p + t_eval[i]·w); obstacle_radius: a scalar, (O,) or, with per-problem
        tables, (B, O) — None: points."""
        a, single = self._batch(alpha, (self.N, self.D))
        B = a.shape[0]
        obs, O, stride = self._obstacle_table(obstacles, B)
        vel = None if obstacle_velocity is None else self._velocity(obstacle_velocity, obs)
        rad = None
        if obstacle_radius is not None and O > 0:
            want = (B, O) if stride else (O,)
            try:
                rad = _f32(np.broadcast_to(_f32(obstacle_radius), want))
            except ValueError:
                raise ValueError(f"obstacle_radius must broadcast to {want}, got {np.shape(obstacle_radius)}") from None
        M = max(int(self.lib.irm_eval_times(self._h, None)), 0)
        rep = (IrmClearanceReport * B)()
        clear = np.zeros((B, M), np.float32) if with_samples else None
        link = np.zeros((B, self.D), np.float32) if with_links else None
        joints = np.zeros((B, M, self.D, 2), np.float32) if with_joints else None
        check(self.lib.irm_clearance(self._h, _ptr(a), _ptr(obs), O, stride, _ptr(vel), _ptr(rad), float(link_radius), B,
                                     rep, _ptr(clear), _ptr(link), _ptr(joints)))
        out = _report(rep, CLEARANCE_REPORT_FIELDS, ("collision_free",), single)
        for name, arr in (("clearance", clear), ("link_clearance", link), ("joints", joints)):
            if arr is not None:
                out[name] = arr[0] if single else arr
        return out

    def self_clearance(self, alpha, link_radius=0.0, with_samples=False, with_pairs=False, with_joints=False):
        """Signed clearance between the arm's own links (every pair (a, b), a + 2 ≤ b, each link a capsule of
        link_radius) on the evaluation times (irm_self_clearance): a dict of arrays named as
        irm_self_clearance_report's fields, plus `clearance` ((B×)M: every sample's minimum), `pair_clearance`
        ((B×)P: every pair's own minimum, in the order of clearance.self_pairs) and `joints` ((B×)M×D×2: the joint
        positions of every sample, the bits of clearance()'s) on request."""
        a, single = self._batch(alpha, (self.N, self.D))
        B = a.shape[0]
        M = max(int(self.lib.irm_eval_times(self._h, None)), 0)
        rep = (IrmSelfClearanceReport * max(B, 1))()
        clear = np.zeros((B, M), np.float32) if with_samples else None
        pair = np.zeros((B, len(self_pairs(self.D))), np.float32) if with_pairs else None
        joints = np.zeros((B, M, self.D, 2), np.float32) if with_joints else None
        check(self.lib.irm_self_clearance(self._h, _ptr(a), float(link_radius), B, rep, _ptr(clear), _ptr(pair),
                                          _ptr(joints)))
        out = _report(rep, SELF_CLEARANCE_REPORT_FIELDS, ("collision_free",), False)
        out = {k: (v[0] if single else v[:B]) for k, v in out.items()}
        for name, arr in (("clearance", clear), ("pair_clearance", pair), ("joints", joints)):
            if arr is not None:
                out[name] = arr[0] if single else arr
        return out

    # ------------------------------------------------- fitting and re-timing
    def set_fit_ridge(self, ridge):
        """The ridge ρ of every later fit_alpha / transfer_alpha (irm_set_fit_ridge: rebuilds W = (K + ρI)⁻¹ and
        drops a transfer that was set).  Raises IrmError where K + ρI is not positive definite (ρ below ≈ 1e-6)."""
        check(self.lib.irm_set_fit_ridge(self._h, float(ridge)))

    def fit_alpha(self, traj):
        """α whose trajectory is the ridge fit of the waypoints traj ((B×)N×D on this context's support times) —
        irm_fit_alpha: the way into the optimiser from a recorded path or another planner's output."""
        q, single = self._batch(traj, (self.N, self.D))
        out = np.zeros_like(q)
        check(self.lib.irm_fit_alpha(self._h, _ptr(q), q.shape[0], _ptr(out)))
        return out[0] if single else out

    def set_transfer(self, n_src, t0=0.0, t1=1.0, rbf_variance_src=None):
        """The operator of transfer_alpha (irm_set_transfer): from a source grid of n_src support times
        linspace(0, 1, n_src) with kernel width rbf_variance_src (None: this context's), re-timed so that
        this context's [0, 1] is the source's [t0, t1].  Replaces the previous transfer."""
        var = -1.0 if rbf_variance_src is None else float(rbf_variance_src)
        check(self.lib.irm_set_transfer(self._h, int(n_src), var, float(t0), float(t1)))
        self._n_src = int(n_src)

    def transfer_alpha(self, alpha_src, with_start=False):
        """α on this context's grid from alpha_src ((B×)n_src×D) on the source grid (irm_transfer_alpha).  With
        with_start also the source trajectory at t0 ((B×)D): the start configuration of the re-timed plan."""
        n_src = getattr(self, "_n_src", 0)  # (0: no transfer set — the library refuses before it reads anything)
        a = _f32(alpha_src)
        single = a.ndim == 2
        if single:
            a = a[None]
        if n_src and (a.ndim != 3 or a.shape[1:] != (n_src, self.D)):
            raise _abi.IrmError(f"alpha_src must be (B, {n_src}, {self.D}) for the transfer that is set, got {a.shape}")
        B = a.shape[0]
        out = np.zeros((B, self.N, self.D), np.float32)
        start = np.zeros((B, self.D), np.float32) if with_start else None
        check(self.lib.irm_transfer_alpha(self._h, _ptr(a), B, _ptr(out), _ptr(start)))
        if single:
            out = out[0]
            start = None if start is None else start[0]
        return (out, start) if with_start else out

    def fit_alpha_dev(self, traj_dev, batch, alpha_dev, stream=0):
        """Enqueue irm_fit_alpha_dev with raw device addresses (e.g. torch data_ptr())."""
        check(self.lib.irm_fit_alpha_dev(self._h, _dev(traj_dev), int(batch), _dev(alpha_dev), ctypes.c_void_p(stream)))

    def clearance_dev(self, alpha_dev, obstacles_dev, n_obstacles, obstacle_stride, batch, report_dev,
                      obstacle_velocity_dev=0, obstacle_radius_dev=0, link_radius=0.0, clear_dev=0, link_dev=0,
                      joints_dev=0, stream=0):
        """Enqueue irm_clearance_dev with raw device addresses (e.g. torch data_ptr()); 0: that table or output is
        absent.  report_dev: batch records of 32 bytes (irm_clearance_report)."""
        rep = ctypes.cast(ctypes.c_void_p(int(report_dev)), ctypes.POINTER(IrmClearanceReport))
        check(self.lib.irm_clearance_dev(self._h, _dev(alpha_dev), _dev(obstacles_dev), int(n_obstacles),
                                         int(obstacle_stride), _dev(obstacle_velocity_dev), _dev(obstacle_radius_dev),
                                         float(link_radius), int(batch), rep, _dev(clear_dev), _dev(link_dev),
                                         _dev(joints_dev), ctypes.c_void_p(stream)))

    def self_clearance_dev(self, alpha_dev, batch, report_dev, link_radius=0.0, clear_dev=0, pair_dev=0, joints_dev=0,
                           stream=0):
        """Enqueue irm_self_clearance_dev with raw device addresses (e.g. torch data_ptr()); 0: that output is
        absent.  report_dev: batch records of 32 bytes (irm_self_clearance_report)."""
        rep = ctypes.cast(ctypes.c_void_p(int(report_dev) if report_dev else None), ctypes.POINTER(IrmSelfClearanceReport))
        check(self.lib.irm_self_clearance_dev(self._h, _dev(alpha_dev), float(link_radius), int(batch), rep,
                                              _dev(clear_dev), _dev(pair_dev), _dev(joints_dev), ctypes.c_void_p(stream)))

    def ik_seed_dev(self, start_dev, goal_xy_dev, batch, q_dev, residual_dev=0, stream=0):
        """Enqueue irm_ik_seed_dev with raw device addresses; residual_dev 0: no residual output."""
        check(self.lib.irm_ik_seed_dev(self._h, _dev(start_dev), _dev(goal_xy_dev), int(batch), _dev(q_dev),
                                       _dev(residual_dev), ctypes.c_void_p(stream)))

    def transfer_alpha_dev(self, alpha_src_dev, batch, alpha_dev, start_dev=0, stream=0):
        """Enqueue irm_transfer_alpha_dev with raw device addresses; start_dev 0: no start output."""
        check(self.lib.irm_transfer_alpha_dev(self._h, _dev(alpha_src_dev), int(batch), _dev(alpha_dev),
                                              _dev(start_dev), ctypes.c_void_p(stream)))

    def _sg(self, start, goal, B):
        s = _f32(np.broadcast_to(_f32(start), (B, self.D)))
        g = _f32(np.broadcast_to(_f32(goal), (B, self.D)))
        return s, g

    @staticmethod
    def _velocity(obstacle_velocity, obs):
        """The velocity table of a moving call: fp32, the shape of the obstacle table `obs`."""
        vel = _f32(obstacle_velocity)
        if vel.shape != obs.shape:
            raise ValueError(f"obstacle_velocity must have the obstacles' shape {obs.shape}, got {vel.shape}")
        return vel

    def _goal_xy(self, goal_xy, B):
        """The end-effector targets of a task call: fp32 B×2 (one target broadcasts over the batch)."""
        return _f32(np.broadcast_to(_f32(goal_xy), (B, 2)))

    @staticmethod
    def _obstacle_table(obstacles, B):
        """(obs, O, stride) of an obstacle table: fp32 (O, 2) shared by the B problems (stride 0) or (B, O, 2) one
        table per problem (stride 2·O floats); an empty table is O = 0."""
        obs = _f32(obstacles)
        O = obs.shape[-2] if obs.size else 0
        stride = 0
        if obs.ndim == 3:
            if obs.shape[0] != B or obs.shape[2] != 2:
                raise ValueError(f"per-problem obstacles must be ({B}, O, 2), got {obs.shape}")
            stride = 2 * O
        elif obs.size and (obs.ndim != 2 or obs.shape[1] != 2):
            raise ValueError(f"shared obstacles must be (O, 2), got {obs.shape}")
        return obs, O, stride

    @staticmethod
    def _has_via(via):
        """Does a call hold via-points?  None and an empty ViaPoints do not — the existing call."""
        if via is None or len(via) == 0:
            return False
        if not isinstance(via, ViaPoints):
            raise TypeError(f"via must be a ViaPoints, got {type(via).__name__}")
        return True

    def _variant(self, obstacle_velocity, goal_xy, via, obs, B):
        """The variant of a call with these optional inputs: (suffix of the entry point — _rank's choice, the
        trailing arguments it takes on top of the plain entry point's, the arrays those point into, to be kept
        alive for the call).  The trailing arguments are the first 0, 1, 2 or 3 of (velocity table shaped like
        `obs`, goal_xy as B×2, irm_via* with its targets as B×V×D), NULL where that input is not given."""
        n = _rank(obstacle_velocity is not None, goal_xy is not None, self._has_via(via))
        vs = tg = None
        if n == 3:
            tg = via.padded(B, self.D)
            vs = _via_struct(via, tg.ctypes.data)
        vel = None if obstacle_velocity is None else self._velocity(obstacle_velocity, obs)
        gxy = None if goal_xy is None else self._goal_xy(goal_xy, B)
        tail = (_ptr(vel), _ptr(gxy), None if vs is None else ctypes.byref(vs))[:n]
        return _SUFFIX[n], tail, (vel, gxy, vs, tg)

    def via_seed(self, start, goal, via, goal_xy=None):
        """α0 ((B×)N×D) through the via-points: the knot configurations start, each via-point in row order and
        the goal — a Cartesian via-point through ik_seed started at the previous knot's configuration, the goal
        likewise when goal_xy is given (`goal` is then not read and may be None) — interpolated linearly between
        the knots on the support times, then fit_alpha of that path."""
        s, single = self._batch(start, (self.D,))
        B = s.shape[0]
        if via is None:
            via = ViaPoints.empty()
        via.check_rows(self.N)
        tg = via.padded(B, self.D)
        knots, rows = [s], [0]
        for i, (r, c) in enumerate(zip(via.rows, via.cartesian)):
            if c:
                q, _ = self.ik_seed(knots[-1], np.ascontiguousarray(tg[:, i, :2]))
            else:
                q = tg[:, i, :]
            knots.append(_f32(q).reshape(B, self.D))
            rows.append(r)
        if goal_xy is not None:
            q, _ = self.ik_seed(knots[-1], self._goal_xy(goal_xy, B))
            knots.append(_f32(q).reshape(B, self.D))
        else:
            if goal is None:
                raise ValueError("via_seed() needs a goal configuration or a goal_xy")
            knots.append(_f32(np.broadcast_to(_f32(goal), (B, self.D))))
        rows.append(self.N - 1)
        path = via_path(self.kernel_matrices()[0], rows, knots)
        alpha = self.fit_alpha(path)
        return alpha[0] if single else alpha

    def ik_seed(self, start, goal_xy):
        """A joint configuration whose end effector is at goal_xy ((B×)2), by damped least squares started at
        `start` ((B×)D) (irm_ik_seed).  Returns (q, residual): residual = ‖f(q) − p‖; best effort — a target
        out of reach or behind the joint limits keeps a residual."""
        s, single = self._batch(start, (self.D,))
        B = s.shape[0]
        p = _f32(goal_xy)
        if p.ndim == 2 and B == 1 and p.shape[0] > 1:  # one start, several targets
            B = p.shape[0]
            s = _f32(np.broadcast_to(s, (B, self.D)))
            single = False
        p = self._goal_xy(p, B)
        q = np.zeros((B, self.D), np.float32)
        res = np.zeros(B, np.float32)
        check(self.lib.irm_ik_seed(self._h, _ptr(s), _ptr(p), B, _ptr(q), _ptr(res)))
        return (q[0], res[0]) if single else (q, res)

    def eval_cost(self, alpha, obstacles, start, goal, lsg, ljl, lmax, obstacle_velocity=None, goal_xy=None,
                  via=None):
        """obstacle_velocity (O×2): waypoint n sees obstacle o at p + t[n]·w (irm_eval_cost_moving).
        goal_xy ((B×)2): row N−1 is held to that end-effector target instead of `goal` (irm_eval_cost_task).
        via (ViaPoints): the via terms λsg·½·Σ_v r_v² join the loss (irm_eval_cost_via)."""
        a, single = self._batch(alpha, (self.N, self.D))
        B = a.shape[0]
        s, g = self._sg(start, goal, B)
        obs = _f32(obstacles).reshape(-1, 2)
        out = np.zeros(B, np.float32)
        vel = None if obstacle_velocity is None else _f32(obstacle_velocity).reshape(-1, 2)
        suffix, tail, _keep = self._variant(vel, goal_xy, via, obs, B)
        check(getattr(self.lib, "irm_eval_cost" + suffix)(self._h, _ptr(a), _ptr(s), _ptr(g), _ptr(obs), obs.shape[0], B,
                                                          float(lsg), float(ljl), float(lmax), _ptr(out), *tail))
        return out[0] if single else out

    def eval_cost_grad(self, alpha, obstacles, start, goal, lsg, ljl, lmax, with_cost=False, obstacle_velocity=None,
                       goal_xy=None, via=None):
        a, single = self._batch(alpha, (self.N, self.D))
        B = a.shape[0]
        s, g = self._sg(start, goal, B)
        obs = _f32(obstacles).reshape(-1, 2)
        grad = np.zeros_like(a)
        cost = np.zeros(B, np.float32)
        vel = None if obstacle_velocity is None else _f32(obstacle_velocity).reshape(-1, 2)
        suffix, tail, _keep = self._variant(vel, goal_xy, via, obs, B)
        check(getattr(self.lib, "irm_eval_cost_grad" + suffix)(self._h, _ptr(a), _ptr(s), _ptr(g), _ptr(obs),
                                                               obs.shape[0], B, float(lsg), float(ljl), float(lmax),
                                                               _ptr(grad), _ptr(cost), *tail))
        if single:
            grad, cost = grad[0], cost[0]
        return (grad, cost) if with_cost else grad

    def constraints(self, alpha, start, goal, goal_xy=None, via=None):
        """goal_xy ((B×)2): the goal-position check is ‖f(τ_{N−1}) − p‖ < eps_position and report[1] that
        Cartesian distance (irm_constraints_task).  via (ViaPoints, also an empty one): ok includes every via
        distance < eps_position, and the via distances ((B×)V) are returned as a third value
        (irm_constraints_via); the 11-float report is unchanged."""
        a, single = self._batch(alpha, (self.N, self.D))
        B = a.shape[0]
        s, g = self._sg(start, goal, B)
        ok = np.zeros(B, np.uint8)
        rep = np.zeros((B, 11), np.float32)
        # no velocity: the twins' trailing arguments start at goal_xy; the _via form adds the distance output
        suffix, tail, _keep = self._variant(None, goal_xy, via, None, B)
        dist = None if via is None else np.zeros((B, len(via)), np.float32)  # (an empty ViaPoints: no distances)
        if suffix == "_via":
            tail += (_ptr(dist),)
        check(getattr(self.lib, "irm_constraints" + suffix)(self._h, _ptr(a), _ptr(s), _ptr(g), B,
                                                            ok.ctypes.data_as(_abi.c_uint8_p), _ptr(rep), *tail[1:]))
        out = [ok.astype(bool), rep] + ([] if dist is None else [dist])
        if single:
            out = [bool(ok[0])] + [x[0] for x in out[1:]]
        return tuple(out)

    def fk(self, traj, with_jacobian=False):
        q, single = self._batch(traj, (self.N, self.D))
        B = q.shape[0]
        pos = np.zeros((B, 2, self.N), np.float32)
        jac = np.zeros((B, 2, self.N, self.D), np.float32) if with_jacobian else None
        check(self.lib.irm_fk(self._h, _ptr(q), B, _ptr(pos), _ptr(jac)))
        if single:
            pos = pos[0]
            jac = None if jac is None else jac[0]
        return (pos, jac) if with_jacobian else pos

    def fk_joints(self, traj):
        """Positions of every joint, B×D×2×N (robot.py:39-72 fk_joint_j for j = 1..D)."""
        q, single = self._batch(traj, (self.N, self.D))
        B = q.shape[0]
        pos = np.zeros((B, self.D, 2, self.N), np.float32)
        check(self.lib.irm_fk_joints(self._h, _ptr(q), B, _ptr(pos)))
        return pos[0] if single else pos

    def compute_cost_vg(self, f, obstacles, with_grad=True):
        x, single = self._batch(f, (2, self.N))
        B = x.shape[0]
        obs = _f32(obstacles).reshape(-1, 2)
        cv = np.zeros((B, self.N), np.float32)
        cg = np.zeros((B, 2, self.N), np.float32) if with_grad else None
        check(self.lib.irm_compute_cost_vg(self._h, _ptr(x), _ptr(obs), obs.shape[0], B, _ptr(cv), _ptr(cg)))
        if single:
            cv = cv[0]
            cg = None if cg is None else cg[0]
        return (cv, cg) if with_grad else cv

    def optimize(self, start, goal, obstacles, alpha0=None, obstacle_stride=0, series=False, obstacle_velocity=None,
                 goal_xy=None, via=None):
        """Batched Optimizer.optimize(): returns (alpha, traj, stats[, series]).
        obstacle_velocity (the shape of obstacles): the optimiser minimises the cost in which waypoint n
        sees obstacle o at p + t[n]·w (irm_optimize_batch_moving).
        goal_xy ((B×)2): the end effector of row N−1 is held to that target instead of the joint configuration
        `goal` (irm_optimize_batch_task); `goal` then feeds only the straight-line initialisation, and
        goal=None means "seed it with ik_seed(start, goal_xy)".
        via (ViaPoints): interior support rows held to joint or end-effector targets (irm_optimize_batch_via);
        without alpha0 the plan starts from via_seed(start, goal, via, goal_xy).  None (or an empty one) keeps
        the call and its initialisation as they are."""
        s, single = self._batch(start, (self.D,))
        B = s.shape[0]
        if self._has_via(via):
            via.check_rows(self.N)
            if alpha0 is None:
                alpha0 = self.via_seed(s, goal, via, goal_xy=goal_xy)
        gxy = None
        if goal_xy is not None:
            gxy = self._goal_xy(goal_xy, B)
            if goal is None:
                goal, _ = self.ik_seed(s, gxy)
        elif goal is None:
            raise ValueError("optimize() needs a goal configuration or a goal_xy")
        g, _ = self._batch(goal, (self.D,))
        obs, O, stride = self._obstacle_table(obstacles, B)
        if obs.ndim == 3 and obstacle_stride not in (0, stride):
            raise ValueError(f"obstacle_stride {obstacle_stride} does not match obstacles {obs.shape}")
        if obs.ndim != 3 and obstacle_stride:
            raise ValueError("obstacle_stride needs per-problem obstacles of shape (B, O, 2)")
        a0 = None
        if alpha0 is not None:
            a0 = _f32(alpha0).reshape(B, self.N, self.D)
        alpha = np.zeros((B, self.N, self.D), np.float32)
        traj = np.zeros_like(alpha)
        stats = (IrmStats * B)()
        cap = self.series_capacity() if series else 0
        ser = np.zeros((B, cap, self.N, self.D), np.float32) if series else None
        suffix, tail, _keep = self._variant(obstacle_velocity, gxy, via, obs, B)
        check(getattr(self.lib, "irm_optimize_batch" + suffix)(self._h, _ptr(a0), _ptr(s), _ptr(g), _ptr(obs), O, stride,
                                                               B, _ptr(alpha), _ptr(traj), stats, _ptr(ser), *tail))
        st = stats_to_dict(stats)
        if single:
            alpha, traj = alpha[0], traj[0]
            st = {k: v[0] for k, v in st.items()}
            if series:
                ser = ser[0][: int(st["series_len"])]
        if series:
            return alpha, traj, st, ser
        return alpha, traj, st

    # ------------------------------------------------------ multi-start planning
    def seed_ensemble(self, start, goal, n_seeds, seed=0, amplitude=1.0, problem_offset=0, with_waypoints=False):
        """The S seeds of every problem (irm_seed_ensemble): α of shape (B, S, N, D) — candidate 0 is init_alpha's α
        to the bit, candidate s ≥ 1 the fit of the smooth-step line plus a hashed smooth bump of amplitude up to
        `amplitude` per joint, clamped to the joint range.  A candidate depends on (seed, problem_offset + b, s)
        and its problem's start and goal only.  with_waypoints: also the waypoints the seeds were fitted to,
        (B, S, N, D).  A single start (D,) gives (S, N, D)."""
        s, single = self._batch(start, (self.D,))
        B, S = s.shape[0], int(n_seeds)
        g = _f32(np.broadcast_to(_f32(goal), (B, self.D)))
        rows = B * max(S, 0)
        alpha = np.zeros((rows, self.N, self.D), np.float32)
        way = np.zeros_like(alpha) if with_waypoints else None
        check(self.lib.irm_seed_ensemble(self._h, _ptr(s), _ptr(g), B, S, int(seed) & 0xFFFFFFFF, float(amplitude),
                                         int(problem_offset), _ptr(alpha), _ptr(way)))
        shape = ((S,) if single else (B, S)) + (self.N, self.D)
        alpha = alpha.reshape(shape)
        return (alpha, way.reshape(shape)) if with_waypoints else alpha

    def rank_candidates(self, stats, reports=None, n_seeds=None):
        """Rank B·S candidates per problem by the key (class, loss, s) (irm_rank_candidates).  stats: a dict with
        constraints_ok and final_loss, each (B, S) or (B·S,) with n_seeds; reports (optional): a dict with
        n_colliding of the same shape, or that array.  Returns (winner (B,), rank (B, S))."""
        ok = np.asarray(stats["constraints_ok"])
        if n_seeds is None:
            if ok.ndim != 2:
                raise ValueError("rank_candidates() needs n_seeds for flat (B*S,) tables")
            n_seeds = ok.shape[1]
        S = int(n_seeds)
        ok = ok.reshape(-1)
        loss = np.asarray(stats["final_loss"], np.float32).reshape(-1)
        if S < 1 or ok.shape[0] % S or loss.shape != ok.shape:
            raise ValueError(f"stats of {ok.shape[0]} / {loss.shape[0]} candidates do not divide into n_seeds={S}")
        BS = ok.shape[0]
        B = BS // S
        st = (IrmStats * max(BS, 1))()
        recs = np.frombuffer(st, dtype=_STATS_DTYPE)
        recs["constraints_ok"][:BS] = ok.astype(np.int32)
        recs["final_loss"][:BS] = loss
        rp = None
        if reports is not None:
            ncol = np.asarray(reports["n_colliding"] if isinstance(reports, dict) else reports).reshape(-1)
            if ncol.shape[0] != BS:
                raise ValueError(f"reports of {ncol.shape[0]} candidates, stats of {BS}")
            rp = (IrmClearanceReport * max(BS, 1))()
            np.frombuffer(rp, dtype=_REPORT_DTYPE)["n_colliding"][:BS] = ncol.astype(np.int32)
        winner = np.zeros(B, np.int32)
        rank = np.zeros((B, S), np.int32)
        check(self.lib.irm_rank_candidates(self._h, st, rp, B, S, winner.ctypes.data_as(_abi.c_int32_p),
                                           rank.ctypes.data_as(_abi.c_int32_p)))
        return winner, rank

    def optimize_multistart(self, start, goal, obstacles, n_seeds, seed=0, amplitude=1.0, problem_offset=0,
                            rank_clearance=False, obstacle_radius=None, link_radius=0.0, obstacle_velocity=None,
                            goal_xy=None, candidates=False, via=None, series=False, rank_self_clearance=False):
        """optimize() from S seeds per problem, ranked and gathered on the device (irm_optimize_multistart): the
        seeds of seed_ensemble, the plain optimiser launch on the B·S replicated problems, with rank_clearance the
        clearance check of every candidate on the evaluation times (set_eval_times; obstacle_radius / link_radius
        as Context.clearance takes them), the ranking by (class, loss, s) and the winner's rows.
        Returns (alpha, traj, stats, info): the winner's α, trajectory and statistics per problem; info["winner"]
        (B,) and, with candidates=True, info["alpha"], info["traj"] (B, S, N, D), info["stats"] (a dict of (B, S)
        arrays), info["rank"] (B, S) and with rank_clearance info["reports"] (a dict of (B, S) arrays).
        goal=None with goal_xy: the goal configuration is ik_seed(start, goal_xy), as in optimize().  Via-points and
        series recording have no multi-start form (IrmError).
        rank_self_clearance: also run self_clearance (link_radius) on every candidate, add its n_colliding to the
        obstacle check's counts (to zeros without rank_clearance), rank again with rank_candidates and return the
        new winner's rows from the candidate tables — host glue over the device calls; info["self_reports"] (a
        dict of (B, S) arrays) is added and info["rank"] is always present."""
        if self._has_via(via):
            raise _abi.IrmError("irm error -22: via: via-points have no multi-start form (the via seed is a path of its own)")
        if rank_self_clearance:
            return self._multistart_self(start, goal, obstacles, n_seeds, seed, amplitude, problem_offset, rank_clearance,
                                         obstacle_radius, link_radius, obstacle_velocity, goal_xy, candidates, series)
        s, single = self._batch(start, (self.D,))
        B, S = s.shape[0], int(n_seeds)
        gxy = None if goal_xy is None else self._goal_xy(goal_xy, B)
        g = None if goal is None else _f32(np.broadcast_to(_f32(goal), (B, self.D)))
        obs, O, stride = self._obstacle_table(obstacles, B)
        vel = None if obstacle_velocity is None else self._velocity(obstacle_velocity, obs)
        rad = None
        if obstacle_radius is not None and O > 0:
            want = (B, O) if stride else (O,)
            try:
                rad = _f32(np.broadcast_to(_f32(obstacle_radius), want))
            except ValueError:
                raise ValueError(f"obstacle_radius must broadcast to {want}, got {np.shape(obstacle_radius)}") from None
        ms = IrmMultistart()
        ms.n_seeds, ms.seed, ms.amplitude = S, int(seed) & 0xFFFFFFFF, float(amplitude)
        ms.problem_offset, ms.rank_clearance = int(problem_offset), int(bool(rank_clearance))
        ms.link_radius = float(link_radius)
        ms.obstacle_radius = None if rad is None else rad.ctypes.data
        rows = B * min(max(S, 0), IRM_MAX_SEEDS)
        alpha = np.zeros((B, self.N, self.D), np.float32)
        traj = np.zeros_like(alpha)
        stats = (IrmStats * max(B, 1))()
        winner = np.zeros(B, np.int32)
        out = IrmMultistartOut()
        out.winner = winner.ctypes.data
        ser = np.zeros(4, np.float32) if series else None  # (refused by the library: it names the argument)
        if candidates:
            c_alpha = np.zeros((rows, self.N, self.D), np.float32)
            c_traj = np.zeros_like(c_alpha)
            c_stats = (IrmStats * max(rows, 1))()
            c_rep = (IrmClearanceReport * max(rows, 1))()
            c_rank = np.zeros(rows, np.int32)
            out.cand_alpha, out.cand_traj, out.rank = c_alpha.ctypes.data, c_traj.ctypes.data, c_rank.ctypes.data
            out.cand_stats, out.cand_reports = ctypes.addressof(c_stats), ctypes.addressof(c_rep)
        check(self.lib.irm_optimize_multistart(self._h, ctypes.byref(ms), None, _ptr(s), _ptr(g), _ptr(obs), O, stride, B,
                                               _ptr(alpha), _ptr(traj), stats, _ptr(ser), _ptr(vel), _ptr(gxy),
                                               ctypes.byref(out)))
        st = stats_to_dict(stats[:B])
        info = {"winner": winner, "n_seeds": S}
        if candidates:
            shape = (B, S)
            recs = np.frombuffer(c_stats, dtype=_STATS_DTYPE)[:rows]
            info["alpha"], info["traj"] = c_alpha.reshape(shape + (self.N, self.D)), c_traj.reshape(shape + (self.N, self.D))
            info["stats"] = {name: recs[name].copy().reshape(shape) for name in _abi.STATS_FIELDS}
            info["rank"] = c_rank.reshape(shape)
            if rank_clearance:
                rep = _report(c_rep, CLEARANCE_REPORT_FIELDS, ("collision_free",), False)
                info["reports"] = {k: v[:rows].reshape(shape) for k, v in rep.items()}
        if single:
            alpha, traj = alpha[0], traj[0]
            st = {k: v[0] for k, v in st.items()}
            info = {k: (v[0] if isinstance(v, np.ndarray) else {n: a[0] for n, a in v.items()} if isinstance(v, dict) else v)
                    for k, v in info.items()}
        return alpha, traj, st, info

    def _multistart_self(self, start, goal, obstacles, n_seeds, seed, amplitude, problem_offset, rank_clearance,
                         obstacle_radius, link_radius, obstacle_velocity, goal_xy, candidates, series):
        """optimize_multistart(rank_self_clearance=True): the device call with its candidate tables, the
        self-clearance check of the B·S candidate α, the ranking on the summed collision counts and the winner's
        rows."""
        if int(self.lib.irm_eval_times(self._h, None)) <= 0:
            raise _abi.IrmError("irm error -22: optimize_multistart: rank_self_clearance needs an evaluation grid "
                                "(set_eval_times)")
        if not (np.isfinite(link_radius) and link_radius >= 0):
            raise _abi.IrmError("irm error -22: optimize_multistart: link_radius must be finite and >= 0")
        s, single = self._batch(start, (self.D,))
        B = s.shape[0]
        _, _, _, info = self.optimize_multistart(
            s, goal, obstacles, n_seeds, seed=seed, amplitude=amplitude, problem_offset=problem_offset,
            rank_clearance=rank_clearance, obstacle_radius=obstacle_radius if rank_clearance else None,
            link_radius=link_radius if rank_clearance else 0.0, obstacle_velocity=obstacle_velocity, goal_xy=goal_xy,
            candidates=True, series=series)
        S = info["alpha"].shape[1]
        rep = self.self_clearance(info["alpha"].reshape(B * S, self.N, self.D), link_radius=link_radius)
        info["self_reports"] = {k: np.asarray(v).reshape(B, S) for k, v in rep.items()}
        ncol = info["self_reports"]["n_colliding"].astype(np.int64)
        if rank_clearance:
            ncol = ncol + info["reports"]["n_colliding"]
        info["winner"], info["rank"] = self.rank_candidates(info["stats"], ncol, n_seeds=S)
        rows = np.arange(B)
        alpha, traj = info["alpha"][rows, info["winner"]].copy(), info["traj"][rows, info["winner"]].copy()
        st = {k: v[rows, info["winner"]].copy() for k, v in info["stats"].items()}
        if not candidates:
            info = {k: v for k, v in info.items() if k in ("winner", "n_seeds", "rank", "self_reports")}
        if single:
            alpha, traj = alpha[0], traj[0]
            st = {k: v[0] for k, v in st.items()}
            info = {k: (v[0] if isinstance(v, np.ndarray) else {n: a[0] for n, a in v.items()} if isinstance(v, dict) else v)
                    for k, v in info.items()}
        return alpha, traj, st, info

    def multistart_workspace(self, batch, n_seeds, n_obstacles=0, obstacle_stride=0):
        """Bytes of device workspace optimize_multistart_dev needs (irm_multistart_workspace)."""
        n = int(self.lib.irm_multistart_workspace(self._h, int(batch), int(n_seeds), int(n_obstacles), int(obstacle_stride)))
        if n < 0:
            check(n)
        return n

    def seed_ensemble_dev(self, start_dev, goal_dev, batch, n_seeds, alpha_dev, seed=0, amplitude=1.0, problem_offset=0,
                          waypoints_dev=0, stream=0):
        """Enqueue irm_seed_ensemble_dev with raw device addresses; waypoints_dev 0: no waypoints output."""
        check(self.lib.irm_seed_ensemble_dev(self._h, _dev(start_dev), _dev(goal_dev), int(batch), int(n_seeds),
                                             int(seed) & 0xFFFFFFFF, float(amplitude), int(problem_offset),
                                             _dev(alpha_dev), _dev(waypoints_dev), ctypes.c_void_p(stream)))

    def rank_candidates_dev(self, stats_dev, batch, n_seeds, winner_dev, reports_dev=0, rank_dev=0, stream=0):
        """Enqueue irm_rank_candidates_dev with raw device addresses (stats: 32-byte irm_stats records; reports:
        32-byte irm_clearance_report records, 0: none; rank_dev 0: no rank output)."""
        vp = lambda a: ctypes.c_void_p(int(a) if a else None)  # noqa: E731
        check(self.lib.irm_rank_candidates_dev(self._h, vp(stats_dev), vp(reports_dev), int(batch), int(n_seeds),
                                               vp(winner_dev), vp(rank_dev), ctypes.c_void_p(stream)))

    def optimize_multistart_dev(self, batch_dev, n_seeds, winner_dev, workspace_dev, workspace_bytes, seed=0,
                                amplitude=1.0, problem_offset=0, rank_clearance=False, obstacle_radius_dev=0,
                                link_radius=0.0, obstacle_velocity_dev=0, goal_xy_dev=0, cand_alpha_dev=0,
                                cand_traj_dev=0, cand_stats_dev=0, cand_reports_dev=0, rank_dev=0, stream=0):
        """Enqueue irm_optimize_multistart_dev with raw device addresses: batch_dev (IrmBatchDev of the B problems:
        alpha0 and series_out 0; its alpha_out / traj_out / stats_out receive the winner's rows), the workspace of
        multistart_workspace() bytes, winner_dev (B int32) and the optional per-candidate outputs (0: absent)."""
        ms = IrmMultistart()
        ms.n_seeds, ms.seed, ms.amplitude = int(n_seeds), int(seed) & 0xFFFFFFFF, float(amplitude)
        ms.problem_offset, ms.rank_clearance = int(problem_offset), int(bool(rank_clearance))
        ms.link_radius = float(link_radius)
        ms.obstacle_radius = int(obstacle_radius_dev) or None
        out = IrmMultistartOut()
        out.winner = int(winner_dev) or None
        out.cand_alpha, out.cand_traj = int(cand_alpha_dev) or None, int(cand_traj_dev) or None
        out.cand_stats, out.cand_reports = int(cand_stats_dev) or None, int(cand_reports_dev) or None
        out.rank = int(rank_dev) or None
        vel = obstacle_velocity_dev or getattr(batch_dev, "obstacle_velocity", 0)
        check(self.lib.irm_optimize_multistart_dev(self._h, ctypes.byref(ms), ctypes.byref(batch_dev), _dev(vel),
                                                   _dev(goal_xy_dev), ctypes.byref(out),
                                                   ctypes.c_void_p(int(workspace_dev) or None), int(workspace_bytes),
                                                   ctypes.c_void_p(stream)))

    def bls_trace_enable(self, cap=256):
        """Record the line-search log of problem 0 of every later BLS optimize (diagnostics)."""
        check(self.lib.irm_debug_bls_trace_enable(self._h, int(cap)))
        self._trace_cap = int(cap)

    def bls_trace(self, n_trials):
        """The last run's log: n_trials × 10 (outer, inner, trial, lr, new_loss, required_loss,
        accepted, loss, ‖g‖, alpha_norm) — optimizer_BLS.py:139-149, 163-166."""
        cap = getattr(self, "_trace_cap", 0)
        out = np.zeros((cap, 10), np.float32)
        n = self.lib.irm_debug_bls_trace(self._h, _ptr(out), cap)
        if n < 0:
            check(n)
        return out[: min(int(n_trials), n)]

    def optimize_dev(self, batch_dev, stream=0, obstacle_velocity_dev=0, goal_xy_dev=0, via=None, via_target_dev=0):
        """Enqueue irm_optimize_batch_dev with device pointers (IrmBatchDev).  obstacle_velocity_dev: the
        device address of the velocity table (the batch's n_obstacles / obstacle_stride), or the
        `obstacle_velocity` that batch_dev() was given; 0: the static launch.  goal_xy_dev: the device address
        of the end-effector targets (batch × 2, irm_optimize_batch_task_dev); 0: the joint goal.  via (ViaPoints;
        its rows and kinds) with via_target_dev, the device address of the targets (batch × V × D fp32):
        irm_optimize_batch_via_dev."""
        vel = obstacle_velocity_dev or getattr(batch_dev, "obstacle_velocity", 0)
        n = _rank(vel, goal_xy_dev, via is not None and len(via))
        # the twins' trailing arguments, then the stream, then the irm_via* (its target a device address)
        tail = (_dev(vel) if vel else None, _dev(goal_xy_dev) if goal_xy_dev else None)[:n] + (ctypes.c_void_p(stream),)
        if n == 3:
            via.check_rows(self.N)
            tail += (ctypes.byref(_via_struct(via, int(via_target_dev) if via_target_dev else None)),)
        check(getattr(self.lib, "irm_optimize_batch" + _SUFFIX[n] + "_dev")(self._h, ctypes.byref(batch_dev), *tail))


def via_path(t, rows, knots):
    """The piecewise-linear joint path of via_seed: B×N×D fp32 through the knot configurations `knots` (each B×D)
    at the support rows `rows` (0 first, N−1 last), linear in the support times t between them — fp32,
    q = a + w·(b − a) with w = (t[n] − t[r0]) / (t[r1] − t[r0])."""
    t = np.asarray(t, np.float32)
    B, D = knots[0].shape
    path = np.zeros((B, t.shape[0], D), np.float32)
    for (r0, a), (r1, b) in zip(zip(rows, knots), zip(rows[1:], knots[1:])):
        w = ((t[r0:r1 + 1] - t[r0]) / (t[r1] - t[r0])).astype(np.float32)
        path[:, r0:r1 + 1, :] = a[:, None, :] + w[None, :, None] * (b - a)[:, None, :]
    return path


def batch_dev(alpha0=0, start=0, goal=0, obstacles=0, n_obstacles=0, obstacle_stride=0, batch=0, alpha_out=0,
              traj_out=0, stats_out=0, series_out=0, obstacle_velocity=0):
    """Build an IrmBatchDev from raw device addresses (e.g. torch data_ptr()).  obstacle_velocity: the device
    address of the velocity table of a moving launch; it is no field of irm_batch_dev (the struct keeps its
    layout) and rides along as an attribute that Context.optimize_dev passes to the moving entry point."""
    b = IrmBatchDev()
    b.obstacle_velocity = int(obstacle_velocity or 0)
    b.alpha0, b.start, b.goal, b.obstacles = alpha0 or None, start, goal, obstacles
    b.n_obstacles, b.obstacle_stride, b.batch = n_obstacles, obstacle_stride, batch
    b.alpha_out, b.traj_out, b.stats_out, b.series_out = alpha_out or None, traj_out or None, stats_out or None, \
        series_out or None
    return b
