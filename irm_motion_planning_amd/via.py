"""Via-points: interior support rows held to joint or Cartesian targets (include/irm.h, irm_via).

A `ViaPoints` names up to MAX_VIA support rows of a plan (strictly increasing, each in 1 … N−2), a kind per row
(joint configuration or end-effector position) and the targets.  The row table and the kinds are shared by a
batch; the targets are per problem.  Host-only: numpy and the ctypes mirror of irm_via, no device, no library.
"""
import ctypes

import numpy as np

MAX_VIA = 4  # IRM_MAX_VIA of include/irm.h


class IrmVia(ctypes.Structure):
    """ctypes mirror of irm_via (include/irm.h)."""
    _fields_ = [
        ("n_via", ctypes.c_int32),
        ("row", ctypes.c_int32 * MAX_VIA),
        ("cartesian", ctypes.c_int32 * MAX_VIA),
        ("target", ctypes.c_void_p),
    ]


class ViaPoints:
    """rows: V support rows; cartesian: V flags (False: all D target values are a joint configuration, True: the
    first two are an end-effector position (x, y), the rest ignored); targets: V×D for one problem (broadcast over
    a batch) or B×V×D.  A Cartesian target may also be given with 2 columns when every via-point is Cartesian —
    `padded(B, D)` fills the rest with zeros."""

    def __init__(self, rows, cartesian, targets):
        self.rows = [int(r) for r in np.asarray(rows, dtype=np.int64).reshape(-1)]
        cart = np.asarray(cartesian).reshape(-1)
        if cart.size == 1 and len(self.rows) > 1:
            cart = np.repeat(cart, len(self.rows))
        if any(c not in (0, 1, False, True) for c in cart.tolist()):
            raise ValueError(f"cartesian must hold 0 / 1 flags, got {cart.tolist()}")
        self.cartesian = [int(bool(c)) for c in cart.tolist()]
        V = len(self.rows)
        if V > MAX_VIA:
            raise ValueError(f"at most {MAX_VIA} via-points, got {V}")
        if len(self.cartesian) != V:
            raise ValueError(f"cartesian must have one flag per row ({V}), got {len(self.cartesian)}")
        if any(b <= a for a, b in zip(self.rows, self.rows[1:])):
            raise ValueError(f"via rows must be strictly increasing, got {self.rows}")
        if any(r < 1 for r in self.rows):
            raise ValueError(f"via rows must lie in [1, N-2], got {self.rows}")
        t = np.asarray(targets, dtype=np.float32)
        if V == 0:
            t = np.zeros((0, 0), np.float32)
        elif t.ndim not in (2, 3) or t.shape[-2] != V:
            raise ValueError(f"targets must be ({V}, D) or (B, {V}, D), got {t.shape}")
        self.targets = t

    def __len__(self):
        return len(self.rows)

    @classmethod
    def empty(cls):
        return cls([], [], np.zeros((0, 0), np.float32))

    @classmethod
    def at_times(cls, ctx_or_n, times, cartesian, targets):
        """Via-points at plan times in (0, 1): each time snaps to the nearest support row of linspace(0, 1, N)
        inside [1, N−2] (ctx_or_n: a Context or N).  Two times that snap to one row are refused; the times must
        increase."""
        return cls(snap_times(ctx_or_n, times), cartesian, targets)

    def check_rows(self, N):
        if self.rows and self.rows[-1] > N - 2:
            raise ValueError(f"via rows must lie in [1, N-2={N - 2}], got {self.rows}")

    def padded(self, B, D):
        """The targets as the library reads them: contiguous fp32 B×V×D."""
        V = len(self)
        t = self.targets
        if V == 0:
            return np.zeros((B, 0, D), np.float32)
        if t.shape[-1] != D:
            if t.shape[-1] == 2 and all(self.cartesian) and D >= 2:
                pad = np.zeros(t.shape[:-1] + (D,), np.float32)
                pad[..., :2] = t
                t = pad
            else:
                raise ValueError(f"targets must have D={D} columns, got {t.shape}")
        if t.ndim == 3 and t.shape[0] not in (1, B):
            raise ValueError(f"targets must be ({V}, {D}) or ({B}, {V}, {D}), got {t.shape}")
        return np.array(np.broadcast_to(t, (B, V, D)), dtype=np.float32, order="C")  # (a writable copy)

    def read_entries_finite(self, B, D):
        """Is every target entry the library reads finite — all D of a joint via-point, the first two of an
        end-effector one (the rest may hold anything)?"""
        t = self.padded(B, D)
        return all(np.all(np.isfinite(t[:, v, :2 if c else D])) for v, c in enumerate(self.cartesian))


def snap_times(ctx_or_n, times):
    """The support rows of plan times in (0, 1): row = round(time·(N−1)) clamped to [1, N−2] (ties to the earlier
    row)."""
    N = int(getattr(ctx_or_n, "N", ctx_or_n))
    if N < 3:
        raise ValueError(f"via-points need N >= 3 support rows, got {N}")
    rows = []
    for tm in np.asarray(times, dtype=np.float64).reshape(-1).tolist():
        if not (0.0 < tm < 1.0):
            raise ValueError(f"a via time must lie in (0, 1), got {tm}")
        r = int(np.ceil(tm * (N - 1) - 0.5))
        rows.append(min(max(r, 1), N - 2))
    for a, b in zip(rows, rows[1:]):
        if b == a:
            raise ValueError(f"two via times snap to support row {a} (N={N}): move one or use more waypoints")
        if b < a:
            raise ValueError(f"via times must increase, got rows {rows}")
    return rows


def via_from_args(args, N, D):
    """The ViaPoints of the CLI flags --via-joint T q1 … qD and --via-xy T X Y (both repeatable, T a plan time in
    (0, 1)) on N support rows, sorted by time; None without either flag."""
    entries = []
    for item in getattr(args, "via_joint", None) or []:
        item = [float(x) for x in item]
        if len(item) != 1 + D:
            raise ValueError(f"--via-joint takes a time and {D} joint values, got {len(item)} numbers")
        entries.append((item[0], 0, item[1:]))
    for item in getattr(args, "via_xy", None) or []:
        item = [float(x) for x in item]
        if len(item) != 3:
            raise ValueError(f"--via-xy takes a time and X Y, got {len(item)} numbers")
        if D < 2:
            raise ValueError("--via-xy needs at least two joints")
        entries.append((item[0], 1, item[1:] + [0.0] * (D - 2)))
    if not entries:
        return None
    entries.sort(key=lambda e: e[0])
    return ViaPoints.at_times(N, [e[0] for e in entries], [e[1] for e in entries],
                              np.asarray([e[2] for e in entries], np.float32))
