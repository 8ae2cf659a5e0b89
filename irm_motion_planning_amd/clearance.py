"""The reports of the clearance checks (irm_clearance, irm_self_clearance; include/irm.h): the ctypes mirrors of
irm_clearance_report and irm_self_clearance_report.

They live here, like irm_via's mirror in via.py, and not among the structs of _abi.py, whose set is pinned to the
layouts every earlier binding had; _abi.py's prototypes refer to them."""
import ctypes


class IrmClearanceReport(ctypes.Structure):
    """ctypes mirror of irm_clearance_report (32 bytes, one per trajectory)."""
    _fields_ = [
        ("min_clearance", ctypes.c_float),
        ("argmin_time", ctypes.c_int32),      # indices into t_eval, links, obstacles; -1 without obstacles
        ("argmin_link", ctypes.c_int32),
        ("argmin_obstacle", ctypes.c_int32),
        ("n_colliding", ctypes.c_int32),      # samples with clearance < 0
        ("first_colliding", ctypes.c_int32),  # the first such index into t_eval, or -1
        ("collision_free", ctypes.c_int32),   # n_colliding == 0
        ("pad_", ctypes.c_int32),
    ]


CLEARANCE_REPORT_FIELDS = [f[0] for f in IrmClearanceReport._fields_ if f[0] != "pad_"]


class IrmSelfClearanceReport(ctypes.Structure):
    """ctypes mirror of irm_self_clearance_report (32 bytes, one per trajectory)."""
    _fields_ = [
        ("min_clearance", ctypes.c_float),
        ("argmin_time", ctypes.c_int32),      # indices into t_eval and the links (a + 2 <= b); -1 with D <= 2
        ("argmin_link_a", ctypes.c_int32),
        ("argmin_link_b", ctypes.c_int32),
        ("n_colliding", ctypes.c_int32),      # samples with a colliding pair (crossing, or clearance < 0)
        ("first_colliding", ctypes.c_int32),  # the first such index into t_eval, or -1
        ("collision_free", ctypes.c_int32),   # n_colliding == 0
        ("n_crossing", ctypes.c_int32),       # samples where some pair crosses
    ]


SELF_CLEARANCE_REPORT_FIELDS = [f[0] for f in IrmSelfClearanceReport._fields_]


def self_pairs(n_joints):
    """The link pairs (a, b), a + 2 <= b, of a D-link arm in the order of pair_out: (0,2), (0,3), …, (D-3, D-1)."""
    return [(a, b) for a in range(n_joints) for b in range(a + 2, n_joints)]
