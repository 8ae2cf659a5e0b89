"""Host-side logic on CPU: the drop-in CLI surface, the trajectory-space operator
the kernel is built on (checked in fp64 numpy against the α-space update of the
reference), and bench.py's problem generation / sharding / flop model.
"""
import numpy as np
import pytest

from conftest import obstacles, oracle_for, ref_args

# main.py:13-102 of the reference: flag -> default (read off its argparser).
REFERENCE_FLAGS = {
    "profiling": False, "extended_vis": False, "n_measurements": 1, "n_times": 1, "optimizer_name": "bls",
    "jit_loop": True, "n_timesteps": 50, "rbf_variance": 0.1, "jac_gaussian_mean": 0.15,
    "max_inner_iteration": 200, "loop_loss_reduction": 1e-3, "max_outer_iteration": 10,
    "lambda_constraint_increase": 10, "lambda_sg_constraint": 0.5, "lambda_jl_constraint": 0.1,
    "eps_position": 0.01, "eps_velocity": 0.01, "lambda_max_cost": 0.5, "lambda_reg": 1e-4,
    "constraint_violating_dependant_loss": True, "joint_safety_limit": 0.98, "max_bls_iteration": 20,
    "bls_lr_start": 0.2, "bls_alpha": 0.01, "bls_beta_plus": 1.2, "bls_beta_minus": 0.5,
    "gd_lr": [2e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-8, 1e-8, 1e-8, 1e-8], "n_joints": 3,
    "link_length": [1.5, 1.0, 0.5], "max_joint_velocity": 7, "max_joint_position": 2, "min_joint_position": -1,
}


def test_cli_surface_matches_reference():
    a = vars(ref_args())
    for k, v in REFERENCE_FLAGS.items():
        assert k in a, k
        assert a[k] == v, (k, a[k], v)
    # same spelling as the reference (it mixes - and _ in the BLS β flags)
    b = ref_args("--bls-beta_plus", 1.5, "--bls-beta_minus", 0.25, "--jit-loop", "FALSE", "--extended-vis", "true")
    assert b.bls_beta_plus == 1.5 and b.bls_beta_minus == 0.25 and b.jit_loop is False and b.extended_vis is True
    with pytest.raises(SystemExit):
        ref_args("--optimizer-name", "adam")


# ---------------------------------------------------------------------------
# The trajectory-space, rank-R formulation used by k_optimize
# ---------------------------------------------------------------------------

def operator(N):
    """F = L·V_R with L = [K; dK] and V_R the top-R eigenvectors of LᵀL (fp64)."""
    _, K, dK, J = oracle_for("--n-timesteps", N).kernel_matrices()
    L = np.vstack([K, dK]).astype(np.float64)
    w, V = np.linalg.eigh(L.T @ L)
    w, V = w[::-1], V[:, ::-1]
    R = 16
    while R < N and w[R] / w[0] >= 1e-12:  # irm_operator.cpp auto rank: σ_R²/σ_0² < 1e-12
        R += 16
    R = min(R, N)
    return L, L @ V[:, :R], R, K.astype(np.float64), dK.astype(np.float64), J.astype(np.float64)


@pytest.mark.parametrize("N", [50, 64, 128, 256])
def test_low_rank_operator_reproduces_alpha_space_update(N):
    """One GD step in α-space, α' = c·α − lr·(Kᵀa + dKᵀb)Jᵀ, maps to waypoint space as
    [T'; V'] = c·[T; V] − lr·L·Lᵀ[a; b]·JᵀJ.  The kernel replaces L·Lᵀ by F·Fᵀ of rank
    R ≤ 32; the truncation must be far below fp32 resolution (rel. 1e-6)."""
    L, F, R, K, dK, J = operator(N)
    assert R <= 32  # k_optimize's register-resident operator limit (IRM_MAX_LR analogue)
    rng = np.random.default_rng(N)
    a = rng.standard_normal((N, 3))
    b = rng.standard_normal((N, 3))
    ab = np.vstack([a, b])
    G_alpha = (K.T @ a + dK.T @ b) @ J.T  # trajectory.py:284-297
    full = L @ (G_alpha @ J)  # Δ[T; V] per unit step
    low = F @ (F.T @ ab) @ (J.T @ J)
    assert np.abs(full - low).max() <= 1e-6 * np.abs(full).max()


@pytest.mark.parametrize("N", [50, 128])
def test_bls_norms_in_reduced_space(N):
    """optimizer_BLS.py:160-170: ‖G‖_F and Σ(Gᵀ·Ĝ) from the rank-R coefficients
    y = Fᵀ[a; b] — ‖G‖² = Σ_r (y·JᵀJ)·y and alpha_norm·‖G‖ = Σ_r (uᵀy)², u = Jᵀ1."""
    L, F, R, K, dK, J = operator(N)
    rng = np.random.default_rng(1)
    ab = rng.standard_normal((2 * N, 3))
    G = L.T @ ab @ J.T
    # G = V_R·y·Jᵀ up to the truncation, and V_R has orthonormal columns: ‖G‖ = ‖y·Jᵀ‖
    y = F.T @ ab
    assert abs(np.sum((y @ J.T) ** 2) - np.sum(G ** 2)) <= 1e-9 * np.sum(G ** 2)
    u = J.T @ np.ones(3)
    alpha_norm = np.sum(G.T @ (G / np.linalg.norm(G)))
    # Σ(GᵀĜ) = Σ_{i,j}(GᵀG)_{ij}/‖G‖ = ‖G·1‖²/‖G‖ = ‖y·u‖²/‖G‖
    assert abs(alpha_norm * np.linalg.norm(G) - np.sum((y @ u) ** 2)) <= 1e-9 * np.sum(G ** 2) * 3


# ---------------------------------------------------------------------------
# bench.py host logic
# ---------------------------------------------------------------------------

def test_bench_problems_shard_disjointly():
    import bench
    for cfg in ("c3", "c4", "c5", "c7"):
        _, B, N, D, O, _ = bench.CONFIGS[cfg]
        s0, g0, o0 = bench.make_problem(cfg, 2, 0)
        s1, g1, o1 = bench.make_problem(cfg, 2, 1)
        sa, ga, oa = bench.make_problem(cfg, 1, 0)
        assert s0.shape == (B, D) and g0.shape == (B, D) and o0.shape == (O, 2)
        np.testing.assert_array_equal(o0, o1)  # shared environment
        np.testing.assert_array_equal(s0, sa)  # rank 0's shard does not depend on world size
        assert not np.array_equal(s0, s1)
        assert s0.dtype == np.float32 and o0.dtype == np.float32
    _, _, obs4 = bench.make_problem("c4", 1, 0)
    assert np.all(np.linalg.norm(obs4, axis=1) >= 0.5) and np.all(np.abs(obs4) <= 3.5)


def test_bench_flop_model():
    import bench
    exec_f, ref_f = bench.flops_per_iteration(128, 3, 11, 32)
    assert ref_f == 12 * 128 * 128 * 3 + 10 * 128 * 9 + 22 * 128 * 11 == 632320
    assert 0 < exec_f < ref_f
    # k_lean at R = 32: stage 1 rank 32, residual z and direction rank 16, G rank 24
    # (the α update: k_lean's two-FMA residual, 7·N·D)
    assert exec_f == (2 * 32 + 2 * 16 + 4 * 16 + 2 * 24) * 128 * 3 + 8 * 128 * 9 + 35 * 128 * 3 + 14 * 128 * 11 == 122240
    gen_f, _ = bench.flops_per_iteration(128, 3, 11, 32, lean=False)  # k_optimize: every stage at R
    assert gen_f == 10 * 32 * 128 * 3 + 8 * 128 * 9 + 42 * 128 * 3 + 14 * 128 * 11 == 167936


def test_bench_kernel_label_is_the_library_plan():
    """bench.py labels the kernel from irm_optimize_plan (the library's own dispatch; the GPU test
    test_gpu_parity.py::test_launch_plan_names_the_dispatched_kernel checks the plans per config)."""
    import bench
    plan = {"kernel": "k_lean<FixShape<3,128,32>,512,1,FULL,GD1>", "flow": 0, "waypoints_per_lane": 1,
            "traj_per_block": 4, "threads": 512, "rank_z": 16, "rank_dir": 16, "rank_g": 24}
    lab = bench.plan_label(plan)
    assert lab.startswith("irm::k_lean<FixShape<3,128,32>,512,1,FULL,GD1> (GD single loop")
    assert "4 trajectories per 512-thread workgroup" in lab and "16/16/24" in lab
    f1, _ = bench.flops_per_iteration(128, 3, 11, 32, ranks=(16, 16, 24))
    f2, _ = bench.flops_per_iteration(128, 3, 11, 32)
    assert f1 == f2 == 122240


def test_bench_args_bench_mode():
    import bench
    a = bench.make_args("c3", False, 200)
    assert a.loop_loss_reduction == -1e30 and a.max_outer_iteration == 1 and a.max_inner_iteration == 200
    assert a.optimizer_name == "gd" and int(a.n_timesteps) == 128
    a5 = bench.make_args("c5", False, 200)
    assert a5.n_joints == 7 and len(a5.link_length) == 7


def test_oracle_bench_mode_runs_exactly_max_inner():
    """Bench mode: every trajectory runs exactly max_inner GD iterations."""
    import bench
    from irm_motion_planning_amd.params import params_from_args
    from oracle.oracle import Oracle
    args = bench.make_args("c3", False, 12)
    o = Oracle(params_from_args(args))
    s, g, obs = bench.make_problem("c3", 1, 0)
    _, st = o.optimize_batch(None, s[:4], g[:4], obs, n_threads=2)
    assert [x["grad_evals"] for x in st] == [12] * 4
    assert obstacles().shape == (11, 2)
