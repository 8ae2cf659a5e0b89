"""ctypes mirror of include/irm.h and the loader of libirm_hip.so.

The shared library is built in-tree by irm_motion_planning_amd.build (or
__graft_entry__.build()).  There is deliberately no CPU fallback: if the HIP
library is missing, or no gfx950 device is present when a context is created,
the calls raise IrmError.
"""
import ctypes
import os

from . import clearance as _clearance  # irm_clearance_report's mirror
from . import multistart as _multistart  # irm_multistart's and irm_multistart_out's mirrors
from . import via as _via  # irm_via's mirror lives with the via-point value object

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IRM_LIB") or os.path.join(HERE, "libirm_hip.so")

IRM_ABI_VERSION = 3
IRM_MAX_JOINTS = 8
IRM_MAX_TIMESTEPS = 512
IRM_MAX_OBSTACLES = 64
IRM_MAX_LR = 32
IRM_MAX_EVAL_TIMES = 4096
IRM_FIT_RIDGE_DEFAULT = 1e-6

IRM_OPT_GD = 0
IRM_OPT_BLS = 1

c_float_p = ctypes.POINTER(ctypes.c_float)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)
c_double_p = ctypes.POINTER(ctypes.c_double)


class IrmError(RuntimeError):
    """Raised for a negative return code of the C ABI (message from irm_last_error)."""


class IrmParams(ctypes.Structure):
    _fields_ = [
        ("n_timesteps", ctypes.c_int32),
        ("n_joints", ctypes.c_int32),
        ("optimizer", ctypes.c_int32),
        ("max_inner_iteration", ctypes.c_int32),
        ("max_outer_iteration", ctypes.c_int32),
        ("max_bls_iteration", ctypes.c_int32),
        ("constraint_violating_dependant_loss", ctypes.c_int32),
        ("n_gd_lr", ctypes.c_int32),
        ("rbf_variance", ctypes.c_float),
        ("loop_loss_reduction", ctypes.c_float),
        ("lambda_constraint_increase", ctypes.c_float),
        ("lambda_sg_constraint", ctypes.c_float),
        ("lambda_jl_constraint", ctypes.c_float),
        ("eps_position", ctypes.c_float),
        ("eps_velocity", ctypes.c_float),
        ("lambda_max_cost", ctypes.c_float),
        ("lambda_reg", ctypes.c_float),
        ("joint_safety_limit", ctypes.c_float),
        ("bls_lr_start", ctypes.c_float),
        ("bls_alpha", ctypes.c_float),
        ("bls_beta_plus", ctypes.c_float),
        ("bls_beta_minus", ctypes.c_float),
        ("max_joint_velocity", ctypes.c_float),
        ("max_joint_position", ctypes.c_float),
        ("min_joint_position", ctypes.c_float),
        ("gd_lr", ctypes.c_float * IRM_MAX_LR),
        ("link_length", ctypes.c_float * IRM_MAX_JOINTS),
        ("jac", ctypes.c_float * (IRM_MAX_JOINTS * IRM_MAX_JOINTS)),
        ("operator_rank", ctypes.c_int32),
        ("operator_tol", ctypes.c_float),
        ("device", ctypes.c_int32),
        ("record_series", ctypes.c_int32),
        ("max_series", ctypes.c_int32),
        ("traj_per_block", ctypes.c_int32),
        ("whole_robot_cost", ctypes.c_int32),
    ]


class IrmStats(ctypes.Structure):
    _fields_ = [
        ("inner_iterations", ctypes.c_int32),
        ("outer_iterations", ctypes.c_int32),
        ("grad_evals", ctypes.c_int32),
        ("cost_evals", ctypes.c_int32),
        ("bls_trials", ctypes.c_int32),
        ("constraints_ok", ctypes.c_int32),
        ("series_len", ctypes.c_int32),
        ("final_loss", ctypes.c_float),
    ]


STATS_FIELDS = [f[0] for f in IrmStats._fields_]


class IrmInfo(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("n_timesteps", ctypes.c_int32),
        ("n_joints", ctypes.c_int32),
        ("operator_rank", ctypes.c_int32),
        ("operator_trunc", ctypes.c_float),
        ("traj_per_block", ctypes.c_int32),
        ("num_cus", ctypes.c_int32),
        ("lds_bytes_optimize", ctypes.c_int32),
        ("device_name", ctypes.c_char * 64),
        ("arch", ctypes.c_char * 32),
        ("build_id", ctypes.c_char * 24),
    ]


class IrmLaunchPlan(ctypes.Structure):
    _fields_ = [
        ("kernel", ctypes.c_char * 128),
        ("lean", ctypes.c_int32),
        ("flow", ctypes.c_int32),
        ("waypoints_per_lane", ctypes.c_int32),
        ("threads", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("lds_bytes", ctypes.c_int32),
        ("traj_per_block", ctypes.c_int32),
        ("rank_z", ctypes.c_int32),
        ("rank_dir", ctypes.c_int32),
        ("rank_g", ctypes.c_int32),
        ("lam16", ctypes.c_float),
        ("lam24", ctypes.c_float),
    ]


class IrmBatchDev(ctypes.Structure):
    _fields_ = [
        ("alpha0", ctypes.c_void_p),
        ("start", ctypes.c_void_p),
        ("goal", ctypes.c_void_p),
        ("obstacles", ctypes.c_void_p),
        ("n_obstacles", ctypes.c_int32),
        ("obstacle_stride", ctypes.c_int32),
        ("batch", ctypes.c_int32),
        ("pad_", ctypes.c_int32),
        ("alpha_out", ctypes.c_void_p),
        ("traj_out", ctypes.c_void_p),
        ("stats_out", ctypes.c_void_p),
        ("series_out", ctypes.c_void_p),
    ]


class IrmDenseReport(ctypes.Structure):
    _fields_ = [
        ("max_cost", ctypes.c_float),
        ("avg_cost", ctypes.c_float),
        ("argmax_cost", ctypes.c_int32),
        ("max_position", ctypes.c_float),
        ("min_position", ctypes.c_float),
        ("max_abs_velocity", ctypes.c_float),
        ("argmax_abs_velocity", ctypes.c_int32),
        ("position_ok", ctypes.c_int32),
        ("velocity_ok", ctypes.c_int32),
        ("pad_", ctypes.c_int32),
    ]


DENSE_REPORT_FIELDS = [f[0] for f in IrmDenseReport._fields_ if f[0] != "pad_"]


def _variants(base, args, moving=None, task=None, via=None, last=()):
    """The rows of one family: `base` and its _moving, _task and _via twins (each given as the argument types it
    appends to the twin before it; None: the family has no such twin), every one followed by `last` (the _dev
    forms: the stream).  `base` "a_dev" names its twins a_moving_dev, …"""
    stem, dev = (base[:-4], "_dev") if base.endswith("_dev") else (base, "")
    rows, args = {base: (ctypes.c_int, list(args) + list(last))}, list(args)
    for suffix, extra in (("_moving", moving), ("_task", task), ("_via", via)):
        if extra is not None:
            args = args + list(extra)
            rows[stem + suffix + dev] = (ctypes.c_int, args + list(last))
    return rows


_i32, _f, _h = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p
_via_p = ctypes.POINTER(_via.IrmVia)
_COST = [_h, c_float_p, c_float_p, c_float_p, c_float_p, _i32, _i32, _f, _f, _f, c_float_p]
_OPTIMIZE = [_h, c_float_p, c_float_p, c_float_p, c_float_p, _i32, _i32, _i32, c_float_p, c_float_p,
             ctypes.POINTER(IrmStats), c_float_p]
_DENSE = [_h, c_float_p, c_float_p, _i32, _i32, _i32, ctypes.POINTER(IrmDenseReport), c_float_p]
_PLAN = [_h, _i32, _i32, _i32, ctypes.POINTER(IrmLaunchPlan)]
_CLEARANCE = [_h, c_float_p, c_float_p, _i32, _i32, c_float_p, c_float_p, _f, _i32,
              ctypes.POINTER(_clearance.IrmClearanceReport), c_float_p, c_float_p, c_float_p]
_SELF_CLEARANCE = [_h, c_float_p, _f, _i32, ctypes.POINTER(_clearance.IrmSelfClearanceReport), c_float_p, c_float_p,
                   c_float_p]

# name -> (restype, argtypes); every symbol include/irm.h declares.
PROTOTYPES = {
    "irm_params_default": (None, [ctypes.POINTER(IrmParams)]),
    "irm_default_jac": (ctypes.c_int, [_i32, _f, ctypes.c_uint32, c_float_p]),
    "irm_ctx_create": (ctypes.c_int, [ctypes.POINTER(_h), ctypes.POINTER(IrmParams)]),
    "irm_ctx_destroy": (None, [_h]),
    "irm_last_error": (ctypes.c_char_p, []),
    "irm_get_info": (ctypes.c_int, [_h, ctypes.POINTER(IrmInfo)]),
    "irm_kernel_matrices": (ctypes.c_int, [_h, c_float_p, c_float_p, c_float_p, c_float_p]),
    "irm_init_alpha": (ctypes.c_int, [_h, c_float_p, c_float_p, _i32, c_float_p]),
    "irm_evaluate": (ctypes.c_int, [_h, c_float_p, _i32, _i32, c_float_p]),
    "irm_fk": (ctypes.c_int, [_h, c_float_p, _i32, c_float_p, c_float_p]),
    "irm_fk_joints": (ctypes.c_int, [_h, c_float_p, _i32, c_float_p]),
    "irm_compute_cost_vg": (ctypes.c_int, [_h, c_float_p, c_float_p, _i32, _i32, c_float_p, c_float_p]),
    "irm_series_capacity": (_i32, [_h]),
    "irm_set_work_queue": (ctypes.c_int, [_h, _i32]),
    "irm_work_queue_groups": (ctypes.c_int, [_h, _i32, _i32, _i32]),
    "irm_query_matrices": (ctypes.c_int, [_i32, _f, c_float_p, _i32, c_float_p, c_float_p]),
    "irm_set_eval_times": (ctypes.c_int, [_h, c_float_p, _i32]),
    "irm_eval_times": (_i32, [_h, c_float_p]),
    "irm_eval_any": (ctypes.c_int, [_h, c_float_p, _i32, _i32, c_float_p]),
    "irm_fit_operator": (ctypes.c_int, [_i32, _f, _f, _i32, _f, _f, _f, c_double_p]),
    "irm_set_fit_ridge": (ctypes.c_int, [_h, _f]),
    "irm_fit_alpha": (ctypes.c_int, [_h, c_float_p, _i32, c_float_p]),
    "irm_set_transfer": (ctypes.c_int, [_h, _i32, _f, _f, _f]),
    "irm_transfer_alpha": (ctypes.c_int, [_h, c_float_p, _i32, c_float_p, c_float_p]),
    "irm_fit_alpha_dev": (ctypes.c_int, [_h, c_float_p, _i32, c_float_p, _h]),
    "irm_transfer_alpha_dev": (ctypes.c_int, [_h, c_float_p, _i32, c_float_p, c_float_p, _h]),
    # Moving obstacles, end-effector goals and via-points: each twin takes the arguments of the one before it and
    # appends its own — the velocity table, goal_xy (B×2), an irm_via* — every one NULL for the existing call.
    # irm_constraints has no velocity and its _via form a distance output; the _dev forms end in the stream
    # (the via form: before the irm_via*); the launch plans differ only in name, but for the irm_via*.
    **_variants("irm_eval_cost", _COST, [c_float_p], [c_float_p], [_via_p]),
    **_variants("irm_eval_cost_grad", _COST + [c_float_p], [c_float_p], [c_float_p], [_via_p]),
    **_variants("irm_constraints", [_h, c_float_p, c_float_p, c_float_p, _i32, c_uint8_p, c_float_p],
                task=[c_float_p], via=[_via_p, c_float_p]),
    **_variants("irm_optimize_batch", _OPTIMIZE, [c_float_p], [c_float_p], [_via_p]),
    **_variants("irm_optimize_batch_dev", [_h, ctypes.POINTER(IrmBatchDev)], [c_float_p], [c_float_p], last=[_h]),
    "irm_optimize_batch_via_dev": (ctypes.c_int, [_h, ctypes.POINTER(IrmBatchDev), c_float_p, c_float_p, _h, _via_p]),
    **_variants("irm_optimize_plan", _PLAN, [], [], [_via_p]),
    **_variants("irm_dense_check", _DENSE, [c_float_p]),
    **_variants("irm_dense_check_dev", _DENSE, [c_float_p], last=[_h]),
    # clearance of the links against disc obstacles (velocity and radius tables nullable)
    "irm_clearance": (ctypes.c_int, _CLEARANCE),
    "irm_clearance_dev": (ctypes.c_int, _CLEARANCE + [_h]),
    # clearance of the links against each other
    "irm_self_clearance": (ctypes.c_int, _SELF_CLEARANCE),
    "irm_self_clearance_dev": (ctypes.c_int, _SELF_CLEARANCE + [_h]),
    "irm_ik_seed": (ctypes.c_int, [_h, c_float_p, c_float_p, _i32, c_float_p, c_float_p]),
    "irm_ik_seed_dev": (ctypes.c_int, [_h, c_float_p, c_float_p, _i32, c_float_p, c_float_p, _h]),
    # multi-start planning: seed ensembles, ranking, and the call (descriptor, irm_optimize_batch_task's arguments,
    # the candidates' outputs; the _dev form: irm_batch_dev, the two tables, outputs, workspace, its bytes, stream)
    "irm_seed_ensemble": (ctypes.c_int, [_h, c_float_p, c_float_p, _i32, _i32, ctypes.c_uint32, _f, _i32, c_float_p,
                                         c_float_p]),
    "irm_seed_ensemble_dev": (ctypes.c_int, [_h, c_float_p, c_float_p, _i32, _i32, ctypes.c_uint32, _f, _i32, c_float_p,
                                             c_float_p, _h]),
    "irm_rank_candidates": (ctypes.c_int, [_h, ctypes.POINTER(IrmStats), ctypes.POINTER(_clearance.IrmClearanceReport),
                                           _i32, _i32, c_int32_p, c_int32_p]),
    "irm_rank_candidates_dev": (ctypes.c_int, [_h, _h, _h, _i32, _i32, _h, _h, _h]),
    "irm_multistart_workspace": (ctypes.c_int64, [_h, _i32, _i32, _i32, _i32]),
    "irm_optimize_multistart": (ctypes.c_int, [_h, ctypes.POINTER(_multistart.IrmMultistart)] + _OPTIMIZE[1:] +
                                [c_float_p, c_float_p, ctypes.POINTER(_multistart.IrmMultistartOut)]),
    "irm_optimize_multistart_dev": (ctypes.c_int, [_h, ctypes.POINTER(_multistart.IrmMultistart),
                                                   ctypes.POINTER(IrmBatchDev), c_float_p, c_float_p,
                                                   ctypes.POINTER(_multistart.IrmMultistartOut), _h, ctypes.c_int64, _h]),
    "irm_build_id": (ctypes.c_char_p, []),
    "irm_debug_phase_profile": (ctypes.c_int, [_h, ctypes.POINTER(ctypes.c_uint64), _i32]),
    "irm_debug_bls_trace_enable": (ctypes.c_int, [_h, _i32]),
    "irm_debug_bls_trace": (ctypes.c_int, [_h, c_float_p, _i32]),
}

_LIB = None


def load_library(path=None):
    """Load libirm_hip.so (in-tree build).  Raises IrmError if it is missing."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise IrmError(
            f"{path} not found: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()')"
        )
    # One HIP runtime per process.  torch ships its own libamdhip64 (SONAME libamdhip64.so.7,
    # but torch's libraries NEED it as "libamdhip64.so"): loaded after ours, the loader maps a
    # second runtime and torch then finds "No HIP GPUs".  Loaded first, ours resolves to torch's
    # copy by SONAME.  So torch, when present, is imported before the library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path == LIB_PATH:
        _LIB = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load_library().irm_last_error()
        raise IrmError(f"irm error {rc}: {msg.decode() if msg else ''}")
    return rc
