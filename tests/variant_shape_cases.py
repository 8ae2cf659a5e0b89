"""Shapes and scenes of the variant-shape tests: moving obstacles and end-effector goals where a trajectory
spans several waves (N > 64) and where several problems share a workgroup (TB > 1).

tests/test_gpu_variant_shapes.py runs them on the device, tests/test_variant_shapes_host.py shows on the CPU
that the yardstick — `TaskRef64` of tests/task_cases.py, which is `MovingRef64` with the end row's terms —
tells the right answer from the ones a multi-wave or slot bug would give, and checks the seeds.  Nothing is
restated here: the restatements, `crossing_tables`, `dyadic_scene`, `well_conditioned_alpha`, `shape_argv`
and `targets_near` are the ones the N ≤ 64 suites use.

One lane per (trajectory, waypoint): NW = N rounded up to 64 lanes, WPT = NW/64 waves per trajectory, TB
trajectories per workgroup (irm_operator.cpp, choose_shape).

| N (D = 3)  | WPT | what it reaches                                                                        |
|------------|-----|----------------------------------------------------------------------------------------|
| 65         | 2   | the second wave holds one valid lane, the task row; t[64] = 1, times n/64 exact in fp32 |
| 100        | 2   | a ragged second wave                                                                   |
| 128        | 2   | C3's shape: the static call runs k_lean, a moving / task call k_optimize<DynShape<3>>  |
| 129        | 3   | the task row alone in the third wave; times n/128 exact                                |
| 256        | 4   | operators read from L2, not register-resident; 1024 threads at TB = 4                  |
| 128, D = 7 | 2   | C7's shape: TB = 2 in 256 threads                                                      |
| 500        | 8   | TB = 1, the LDS nearly full                                                            |
"""
import functools

import numpy as np

import moving_cases as mc
import task_cases as tc
from test_gpu_task import targets_near

COST_RTOL = 1e-5     # cost against the restatement, relative (tests/test_gpu_moving.py)
GRAD_RTOL = 2e-4     # gradient against the restatement, relative to max|G|
ORACLE_FLOOR = 5e-3  # the band floor for device-vs-restatement iterates (tests/test_gpu_parity.py)
MUTANT_FACTOR = 4.0  # a mutant of the restatement lies at least this many bounds away from it

KINDS = ("moving", "task", "both")

# ------------------------------------------------------------------------------------------ optimiser variants
# What a moving or task optimize() runs, as launch_plan reports it on the MI355X:
# (N, D, traj_per_block) -> (threads of the instantiation, threads launched, operators, REGOPS or "-") of
# k_optimize<DynShape<D>, threads, operators, REGOPS, GD | BLS>.  Batches of a few workgroups are padded to 512
# threads (choose_shape); with more workgroups than half the CUs, TB = 2 at N = 128 launches 256 threads of
# k_optimize<DynShape<D>,256,OPS_LDS,REGOPS,…> (the tests that do so pass the thread count).  N = 129 at TB = 4 is a
# fifth variant: 768 threads of the 1024-thread instantiation, operators staged in LDS without the register copy.
OPTIMIZE = {
    (33, 3, 5): (512, 512, "OPS_LDS", "REGOPS"), (64, 3, 5): (512, 512, "OPS_LDS", "REGOPS"),
    (65, 3, 4): (512, 512, "OPS_LDS", "REGOPS"), (100, 3, 4): (512, 512, "OPS_LDS", "REGOPS"),
    (128, 3, 2): (512, 512, "OPS_LDS", "REGOPS"), (128, 3, 4): (512, 512, "OPS_LDS", "REGOPS"),
    (128, 7, 2): (512, 512, "OPS_LDS", "REGOPS"), (129, 3, 4): (1024, 768, "OPS_LDS", "-"),
    (256, 3, 2): (512, 512, "OPS_L2", "-"), (256, 3, 4): (1024, 1024, "OPS_L2", "-"), (500, 3, 1): (512, 512, "OPS_L2", "-"),
}

# ------------------------------------------------------------------------------------------ 1. k_forward
# (N, D) -> (B, TB): irm_eval_cost(_grad)_* take the largest TB that fits — min(16/D, threads/NW), 1024 threads
# (512 at D ≥ 5) — so B problems of one call run as ⌈B/TB⌉ workgroups, the last one ragged.
FORWARD = {(65, 3): (7, 5), (100, 3): (7, 5), (128, 3): (7, 5), (129, 3): (7, 5), (256, 3): (6, 4), (128, 7): (3, 2),
           (500, 3): (3, 2)}
# the whole-robot case: a multi-wave N with the task row alone in its wave
FORWARD_WHOLE = (129, 3)
LMAX = (0.0, 0.25)
# (N, D, whole) -> seeds of (well_conditioned_alpha, crossing_tables): the first for which some problem of the call
# has its arg-max waypoint at n ≥ 64 with the moving table and some problem with the table frozen at t = 0, each
# by a margin the max-cost term shows, and each feature moves every problem's cost by more than 2e-3 relative
# (tests/test_variant_shapes_host.py checks it)
FORWARD_SEEDS = {(65, 3, 0): (4, 3), (100, 3, 0): (0, 0), (128, 3, 0): (1, 0), (129, 3, 0): (3, 0), (256, 3, 0): (0, 0),
                 (128, 7, 0): (1, 0), (500, 3, 0): (0, 0), (129, 3, 1): (0, 0)}


def obstacles_of(N):
    """O ∈ {11, 13}: the straight-line block of 9–12 obstacles, and the pair loop with sentinel padding."""
    return 13 if N in (100, 129) else 11


@functools.lru_cache(maxsize=None)
def restatement(N, D, whole=False, extra=()):
    return tc.restatement(*mc.shape_argv(N, D), *extra, whole_robot=bool(whole))


def links_of(o, D):
    return [float(o.params.link_length[i]) for i in range(D)]


@functools.lru_cache(maxsize=None)
def forward_scene(N, D, whole=False):
    """B problems of one eval_cost(_grad) call: α of moderate size with its own start / goal, one target per
    problem, one obstacle table with velocities for the call."""
    R, o = restatement(N, D, whole)
    B, TB = FORWARD[(N, D)]
    O = obstacles_of(N)
    seed_a, seed_t = FORWARD_SEEDS[(N, D, int(whole))]
    alpha, s, g = mc.well_conditioned_alpha(o, B, D, seed=seed_a)
    links = links_of(o, D)
    p, w = mc.crossing_tables(B, O, 0.8 * float(sum(links)), seed=seed_t)
    xy = targets_near(links, g, N + D)
    return dict(N=N, D=D, whole=bool(whole), B=B, TB=TB, O=O, alpha=alpha, s=s, g=g, p=p[0], w=w[0], xy=xy, links=links)


def forward_reference(sc, kind, lam, R=None, table=None, xy=None):
    """(cost B, gradient B×N×D) of the restatement for a forward scene.  kind: which feature is on.  R, table,
    xy: a mutant restatement / obstacle table / target list in place of the scene's own."""
    R = R or restatement(sc["N"], sc["D"], sc["whole"])[0]
    if table is None:
        table = R.table(sc["p"], sc["w"]) if kind in ("moving", "both") else sc["p"]
    xy = sc["xy"] if xy is None else xy
    cost, grad = np.zeros(sc["B"]), np.zeros(sc["alpha"].shape)
    for b in range(sc["B"]):
        goal = tc.TaskGoal(xy[b]) if kind in ("task", "both") else sc["g"][b]
        cost[b] = R.cost(sc["alpha"][b], table, sc["s"][b], goal, *lam)
        grad[b] = R.cost_g(sc["alpha"][b], table, sc["s"][b], goal, *lam)
    return cost, grad


def argmax_waypoints(sc, kind):
    """The restatement's arg-max waypoint of the obstacle potential per problem (the max-cost term's row)."""
    R = restatement(sc["N"], sc["D"], sc["whole"])[0]
    table = R.table(sc["p"], sc["w"]) if kind in ("moving", "both") else sc["p"]
    return np.array([int(np.argmax(R.waypoint_cost(R.traj_vel(sc["alpha"][b])[0], table))) for b in range(sc["B"])])


def forward_cases():
    """(N, D, whole, kind, lmax) of test 1."""
    out = [(N, D, 0, kind, lmax) for (N, D) in FORWARD for kind in KINDS for lmax in LMAX]
    return out + [(*FORWARD_WHOLE, 1, "both", lmax) for lmax in LMAX]


# ------------------------------------------------------------------------------------------ 4. GD iterates
GD_STEPS = 15
GD_ARGV = ("--optimizer-name", "gd", "--max-outer-iteration", "1", "--loop-loss-reduction=-1e30", "--max-inner-iteration",
           str(GD_STEPS), "--lambda-max-cost", "0")
# (N, D) -> (B, traj_per_block): N = 65 and 128 with a full workgroup of 4 and a ragged one of 2, N = 256 with 4 + 1
ITERATES = {(65, 3): (6, 4), (128, 3): (6, 4), (256, 3): (5, 4)}


@functools.lru_cache(maxsize=None)
def iterate_scene(N, D):
    """B problems of one optimize() call, per-problem tables of 11 crossing obstacles.  α0 is the
    well-conditioned α with start and goal taken from its own end rows (fp32), not initTrajectory's line as at
    N ≤ 64: the line fit is a numerically singular solve (max|α0| = 6.5e3 at N = 65), the static launch from it
    lies e_static = 8.1e-3 / 1.4e-3 / 8.2e-3 from the restatement at N = 65 / 128 / 256 (MI355X), and
    at N = 65 the band 2·e_static = 1.6e-2 would sit right under the 1.9e-2 by which dropping the end row's term
    moves the plan — less than the 4·ORACLE_FLOOR the host test asks of every mutant.  From this α0 e_static is
    2e-7 … 1.3e-6, the band is the floor, and the closest mutant lies 4.7e-2 away."""
    R, o = restatement(N, D, False, GD_ARGV)
    B, TB = ITERATES[(N, D)]
    O = 11
    alpha, _, _ = mc.well_conditioned_alpha(o, B, D, seed=7 * N + D)
    s = np.stack([R.traj_vel(alpha[b])[0][0] for b in range(B)]).astype(np.float32)
    g = np.stack([R.traj_vel(alpha[b])[0][-1] for b in range(B)]).astype(np.float32)
    links = links_of(o, D)
    p, w = mc.crossing_tables(B, O, 0.8 * float(sum(links)), seed=N)
    xy = targets_near(links, g, N)
    return dict(N=N, D=D, B=B, TB=TB, O=O, alpha=alpha, s=s, g=g, p=p, w=w, xy=xy, links=links)


def iterate_reference(sc, kind, R=None, tables=None, xy=None):
    """Trajectories (B×N×D, fp64) after GD_STEPS steps of the restatement.  kind "static": neither feature."""
    R = R or restatement(sc["N"], sc["D"], False, GD_ARGV)[0]
    xy = sc["xy"] if xy is None else xy
    out = np.zeros(sc["alpha"].shape)
    for b in range(sc["B"]):
        if tables is not None:
            table = tables[b]
        else:
            table = R.table(sc["p"][b], sc["w"][b]) if kind in ("moving", "both") else sc["p"][b]
        goal = tc.TaskGoal(xy[b]) if kind in ("task", "both") else sc["g"][b]
        a, _, n = R.gd_single(sc["alpha"][b], table, sc["s"][b], goal, GD_STEPS)
        assert n == GD_STEPS
        out[b] = R.traj_vel(a)[0]
    return out


@functools.lru_cache(maxsize=None)
def iterate_plans(N, D, kind):
    """iterate_reference of the scene of (N, D), computed once per session."""
    return iterate_reference(iterate_scene(N, D), kind)
