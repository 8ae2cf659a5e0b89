"""The report of the clearance check (irm_clearance, include/irm.h): the ctypes mirror of irm_clearance_report.

It lives here, like irm_via's mirror in via.py, and not among the structs of _abi.py, whose set is pinned to the
layouts every earlier binding had; _abi.py's prototypes refer to it."""
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
