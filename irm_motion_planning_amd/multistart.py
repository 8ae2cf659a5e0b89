"""Multi-start planning (irm_optimize_multistart, include/irm.h): the ctypes mirrors of its descriptor irm_multistart
and of irm_multistart_out.

They live here, like irm_via's mirror in via.py and the clearance report's in clearance.py, and not among the structs
of _abi.py, whose set is pinned to the layouts every earlier binding had; _abi.py's prototypes refer to them."""
import ctypes

IRM_MAX_SEEDS = 64


class IrmMultistart(ctypes.Structure):
    """ctypes mirror of irm_multistart (32 bytes)."""
    _fields_ = [
        ("n_seeds", ctypes.c_int32),          # S in [1, IRM_MAX_SEEDS]
        ("seed", ctypes.c_uint32),
        ("amplitude", ctypes.c_float),        # A >= 0, finite
        ("problem_offset", ctypes.c_int32),   # global index of the call's problem 0
        ("rank_clearance", ctypes.c_int32),   # 1: rank with the clearance check's n_colliding
        ("link_radius", ctypes.c_float),
        ("obstacle_radius", ctypes.c_void_p),  # nullable
    ]


class IrmMultistartOut(ctypes.Structure):
    """ctypes mirror of irm_multistart_out: winner (B) and the nullable per-candidate outputs (B·S rows)."""
    _fields_ = [
        ("winner", ctypes.c_void_p),
        ("cand_alpha", ctypes.c_void_p),
        ("cand_traj", ctypes.c_void_p),
        ("cand_stats", ctypes.c_void_p),
        ("cand_reports", ctypes.c_void_p),
        ("rank", ctypes.c_void_p),
    ]


def candidate_class(constraints_ok, n_colliding=None):
    """The class of the ranking key (class, loss, s): 2·(not constraints_ok) + (n_colliding > 0); the NaN-loss class 4
    is the ranking's own."""
    import numpy as np
    cls = 2 * (np.asarray(constraints_ok) == 0).astype(np.int32)
    if n_colliding is not None:
        cls = cls + (np.asarray(n_colliding) > 0).astype(np.int32)
    return cls
