/*
 * irm.h — C ABI of the MI355X-native RKHS trajectory optimiser
 * (drop-in for the hot path of simongroeger/irm_motion_planning).
 *
 * The reference has no FFI layer: its de-facto operator boundary is the
 * Python object API that main.py drives:
 *   Optimizer(args) / .optimize()        main.py:109-122, optimizer_GD.py:54-65,
 *                                        optimizer_BLS.py:57-62
 *   Trajectory.evaluate                  trajectory.py:63-65
 *   Trajectory.initTrajectory            trajectory.py:73-78
 *   Trajectory.compute_trajectory_cost   trajectory.py:271-281
 *   Trajectory.compute_trajectory_cost_g trajectory.py:284-297
 *   Trajectory.constraintsFulfilled      trajectory.py:129-137
 *   Robot.fk / Robot.jacobian            robot.py:29-36, 75-87
 *   environment.compute_cost(_vg)        environment.py:32-58
 * Each entry point below names the reference symbol it replaces.  The
 * Python host layer (irm_motion_planning_amd/) binds these with ctypes.
 *
 * Conventions
 *   - Arrays are C-contiguous float32, row-major.  A batch of B trajectories
 *     of N waypoints and D joints is B×N×D (waypoint-major, as np.savetxt
 *     writes a reference trajectory).  Obstacles are O×2.
 *   - Host-pointer entry points copy in, compute on the context's device and
 *     synchronise before returning.  *_dev entry points take device pointers
 *     and a hipStream_t (as void*) and only enqueue.
 *   - Return 0 on success, a negative IRM_E* code on failure; the message is
 *     available from irm_last_error() (thread-local).  Nothing here calls
 *     exit(); the reference's exit(-1) cases are reported as IRM_EINVAL.
 *   - One context per device per thread.  There is no CPU fallback: a
 *     context cannot be created without a gfx950 device.
 */
#ifndef IRM_H_
#define IRM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRM_ABI_VERSION 3

#define IRM_MAX_JOINTS 8       /* D  */
#define IRM_MAX_TIMESTEPS 512  /* N  */
#define IRM_MAX_OBSTACLES 64   /* O  */
#define IRM_MAX_LR 32          /* len(--gd-lr) */

#define IRM_OK 0
#define IRM_EINVAL (-22)
#define IRM_ENOMEM (-12)
#define IRM_EDEVICE (-19)
#define IRM_EKERNEL (-5)

#define IRM_OPT_GD 0  /* optimizer_GD.GradientDescentOptimizer            */
#define IRM_OPT_BLS 1 /* optimizer_BLS.BacktrackingLineSearchOptimizer    */

/* Hyper-parameters: every field of main.py's argparser (main.py:13-102) that
 * reaches the optimiser, with the same meaning.  Fill with irm_params_default
 * and override. */
typedef struct irm_params {
    int32_t n_timesteps;         /* --n-timesteps (N), main.py:33          */
    int32_t n_joints;            /* --n-joints (D), main.py:89             */
    int32_t optimizer;           /* IRM_OPT_GD | IRM_OPT_BLS, main.py:27   */
    int32_t max_inner_iteration; /* main.py:41                             */
    int32_t max_outer_iteration; /* main.py:47                             */
    int32_t max_bls_iteration;   /* main.py:73                             */
    int32_t constraint_violating_dependant_loss; /* bool, main.py:67      */
    int32_t n_gd_lr;             /* number of valid entries in gd_lr      */
    float rbf_variance;          /* σ of the RBF kernel, main.py:35        */
    float loop_loss_reduction;   /* main.py:43                             */
    float lambda_constraint_increase; /* main.py:49                        */
    float lambda_sg_constraint;  /* main.py:52                             */
    float lambda_jl_constraint;  /* main.py:54                             */
    float eps_position;          /* main.py:57; a length with goal_xy (below) */
    float eps_velocity;          /* main.py:59                             */
    float lambda_max_cost;       /* main.py:63                             */
    float lambda_reg;            /* main.py:65                             */
    float joint_safety_limit;    /* main.py:69                             */
    float bls_lr_start;          /* main.py:75                             */
    float bls_alpha;             /* main.py:77                             */
    float bls_beta_plus;         /* main.py:79                             */
    float bls_beta_minus;        /* main.py:81                             */
    float max_joint_velocity;    /* main.py:93                             */
    float max_joint_position;    /* main.py:95                             */
    float min_joint_position;    /* main.py:97                             */
    float gd_lr[IRM_MAX_LR];     /* --gd-lr, main.py:85                    */
    float link_length[IRM_MAX_JOINTS];           /* main.py:91             */
    float jac[IRM_MAX_JOINTS * IRM_MAX_JOINTS];  /* J (D×D), trajectory.py:42;
                                                    irm_default_jac fills it */
    /* --- build-only knobs (no reference counterpart) --- */
    int32_t operator_rank;  /* rank R of the kernel operator used inside the
                               optimiser loop: 0 = auto (smallest multiple of
                               16 whose truncation is below operator_tol),
                               -1 = dense (exact [K;dK]), >0 = explicit. */
    float operator_tol;     /* auto-rank tolerance on σ_R²/σ_0² (1e-12)   */
    int32_t device;         /* HIP device ordinal                          */
    int32_t record_series;  /* keep per-iteration snapshots (--extended-vis) */
    int32_t max_series;     /* snapshot capacity per trajectory (0 = auto) */
    int32_t traj_per_block; /* trajectories per workgroup (0 = auto)       */
    /* --- additive cost variant (ABI 2) --- */
    int32_t whole_robot_cost; /* 0: end-effector obstacle cost (the reference's,
                                 trajectory.py:113-126); 1: summed over every
                                 joint position fk_j, j = 1..D (robot.py:39-72;
                                 DevBlog-Theme/blog-post.html:491-498)       */
} irm_params;

/* Per-trajectory statistics of one optimize() call. */
typedef struct irm_stats {
    int32_t inner_iterations; /* accepted inner-loop steps, all outer iterations */
    int32_t outer_iterations; /* outer (λ) iterations executed               */
    int32_t grad_evals;       /* compute_trajectory_cost_g equivalents       */
    int32_t cost_evals;       /* compute_trajectory_cost equivalents         */
    int32_t bls_trials;       /* BLS trial evaluations (0 for GD)            */
    int32_t constraints_ok;   /* constraintsFulfilled at exit (0/1)          */
    int32_t series_len;       /* snapshots written (record_series)           */
    float final_loss;         /* loss at the returned α with the final λ's   */
} irm_stats;

/* Context / device facts (filled by irm_get_info). */
typedef struct irm_info {
    int32_t abi_version;
    int32_t n_timesteps;
    int32_t n_joints;
    int32_t operator_rank;      /* R actually used                         */
    float operator_trunc;       /* σ_R²/σ_0² dropped by the truncation     */
    int32_t traj_per_block;     /* TB used by the optimiser kernel         */
    int32_t num_cus;
    int32_t lds_bytes_optimize; /* LDS per optimiser workgroup             */
    char device_name[64];
    char arch[32];
    char build_id[24];          /* = irm_build_id(): source hash of the build */
} irm_info;

/* Device-pointer batch for irm_optimize_batch_dev.  All pointers are device
 * pointers; nullable outputs may be 0. */
typedef struct irm_batch_dev {
    const float* alpha0;   /* B×N×D initial α (or 0: start from the straight
                              line of initTrajectory, computed on device)    */
    const float* start;    /* B×D                                            */
    const float* goal;     /* B×D                                            */
    const float* obstacles;/* O×2 (obstacle_stride 0) or B×O×2               */
    int32_t n_obstacles;   /* O                                              */
    int32_t obstacle_stride; /* 0: shared environment; else floats between
                                consecutive trajectories' obstacle sets      */
    int32_t batch;         /* B                                              */
    int32_t pad_;
    float* alpha_out;      /* B×N×D final α (nullable)                       */
    float* traj_out;       /* B×N×D final K α J (nullable)                   */
    irm_stats* stats_out;  /* B (nullable)                                   */
    float* series_out;     /* B×max_series×N×D snapshots (nullable)          */
} irm_batch_dev;

typedef struct irm_ctx irm_ctx;

/* Defaults of main.py's argparser (main.py:13-102), N=50, D=3, BLS. */
void irm_params_default(irm_params* p);

/* J = I + jgm·normal(PRNGKey(seed), (D,D)), legacy threefry2x32 as
 * jax.random.normal draws it — trajectory.py:42. */
int irm_default_jac(int32_t n_joints, float jac_gaussian_mean, uint32_t seed, float* jac_out);

int irm_ctx_create(irm_ctx** out, const irm_params* params);
void irm_ctx_destroy(irm_ctx* ctx);
const char* irm_last_error(void);
int irm_get_info(const irm_ctx* ctx, irm_info* out);

/* t (N), K (N×N), dK (N×N), J (D×D) exactly as Trajectory.__init__ builds
 * them — trajectory.py:14-19, 35-48 (any output may be NULL). */
int irm_kernel_matrices(const irm_ctx* ctx, float* t, float* km, float* dkm, float* jac);

/* Trajectory.initTrajectory — trajectory.py:73-78: α0 = solve(K, line·J⁻¹)
 * for B start/goal pairs (B×D each) → B×N×D. */
int irm_init_alpha(irm_ctx* ctx, const float* start, const float* goal, int32_t batch, float* alpha_out);

/* Trajectory.evaluate — trajectory.py:63-65: out = M·α·J with M = K
 * (which = 0) or dK (which = 1), for B trajectories. */
int irm_evaluate(irm_ctx* ctx, const float* alpha, int32_t batch, int32_t which, float* out);

/* Trajectory.compute_trajectory_cost — trajectory.py:271-281. */
int irm_eval_cost(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                  const float* obstacles, int32_t n_obstacles, int32_t batch,
                  float lambda_sg, float lambda_jl, float lambda_max, float* cost_out);

/* Trajectory.compute_trajectory_cost_g — trajectory.py:284-297 (cost_out
 * nullable: the cost at α is produced by the same pass). */
int irm_eval_cost_grad(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                       const float* obstacles, int32_t n_obstacles, int32_t batch,
                       float lambda_sg, float lambda_jl, float lambda_max,
                       float* grad_out, float* cost_out);

/* Trajectory.constraintsFulfilled(Verbose) — trajectory.py:129-180 with
 * robot.py:90-113.  report_out (nullable) holds, per trajectory, the 7
 * numbers constraintsFulfilledVerbose prints: ‖τ0−s‖, ‖τN−1−g‖, ‖v0‖,
 * ‖vN−1‖, max τ, min τ, max|v|, plus the 4 sub-flags as floats (11). */
int irm_constraints(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                    int32_t batch, uint8_t* ok_out, float* report_out);

/* Robot.fk + Robot.jacobian — robot.py:29-36, 75-87: pos_out B×2×N,
 * jac_out B×2×N×D (nullable). */
int irm_fk(irm_ctx* ctx, const float* traj, int32_t batch, float* pos_out, float* jac_out);

/* Robot.fk_joint_1..3 — robot.py:39-72 (generalised to j = 1..D): position of
 * joint j (FK of the first j links) for every waypoint, pos_out B×D×2×N
 * (pos_out[b][j-1] = fk_joint_j(traj[b]); fk_joint_D = fk).  ABI 2. */
int irm_fk_joints(irm_ctx* ctx, const float* traj, int32_t batch, float* pos_out);

/* environment.compute_cost_vg — environment.py:46-58 (cost_g nullable ⇒
 * compute_cost, environment.py:32-43): f B×2×N → cost_v B×N, cost_g B×2×N. */
int irm_compute_cost_vg(irm_ctx* ctx, const float* f, const float* obstacles, int32_t n_obstacles,
                        int32_t batch, float* cost_v, float* cost_g);

/* Optimizer.optimize() for a batch — optimizer_GD.py:54-232 /
 * optimizer_BLS.py:57-213 (jit variants), one persistent launch.  alpha0 may
 * be NULL (start from initTrajectory on device).  Outputs nullable. */
int irm_optimize_batch(irm_ctx* ctx, const float* alpha0, const float* start, const float* goal,
                       const float* obstacles, int32_t n_obstacles, int32_t obstacle_stride,
                       int32_t batch, float* alpha_out, float* traj_out, irm_stats* stats_out,
                       float* series_out);

/* Same, device pointers, enqueue-only on `stream` (hipStream_t). */
int irm_optimize_batch_dev(irm_ctx* ctx, const irm_batch_dev* args, void* stream);

/* Workspace sizing for irm_optimize_batch_dev callers that pass series_out. */
int32_t irm_series_capacity(const irm_ctx* ctx);

/* The optimiser launch that irm_optimize_batch(_dev) runs for `batch` problems with n_obstacles
 * obstacles (record_series: series_out passed; the context's own irm_params.record_series counts
 * too, as in the launch).  Filled in by the launch dispatch itself with nothing launched, so it
 * names the kernel that actually runs (bench.py's flop model and kernel label come from here).
 * The plan assumes one obstacle table shared by the batch (obstacle_stride 0): per-problem tables
 * take more LDS per workgroup and may run fewer trajectories per workgroup.  ABI 3; no reference
 * counterpart. */
typedef struct irm_launch_plan {
    char kernel[128];           /* template instance, e.g. k_lean<FixShape<3,128,32>,512,1,FULL,GD1> */
    int32_t lean;               /* 1: k_lean, 0: k_optimize                                */
    int32_t flow;               /* 0 GD single loop, 1 GD dual loop, 2 BLS                 */
    int32_t waypoints_per_lane;
    int32_t threads;            /* per workgroup                                           */
    int32_t grid;               /* workgroups                                              */
    int32_t lds_bytes;          /* per workgroup                                           */
    int32_t traj_per_block;
    int32_t rank_z;             /* operator rank of the rounding-residual projection (0: V_R = I) */
    int32_t rank_dir;           /* ... of the waypoint direction F·y''                     */
    int32_t rank_g;             /* ... of the α-space gradient G = V_R·y'' (0: V_R = I, a copy) */
    float lam16;                /* λ_16/λ_0 of [K; dK]ᵀ[K; dK] as built (0: not in the operator) */
    float lam24;                /* λ_24/λ_0                                                */
} irm_launch_plan;
int irm_optimize_plan(const irm_ctx* ctx, int32_t batch, int32_t n_obstacles, int32_t record_series,
                      irm_launch_plan* out);

/* Work queue: an opt-in scheduling mode of irm_optimize_batch(_dev) for the GD dual-loop and BLS
 * flows, whose problems end after very different numbers of rounds.  The launch runs `groups`
 * persistent workgroups; a workgroup slot whose problem has finished writes that problem's outputs,
 * claims the next unsolved problem index from a device counter and loads it.  Results (α, trajectory,
 * every irm_stats field) are bit-identical to the static launch.
 *   groups = 0   off (the default: one workgroup per traj_per_block problems, as before)
 *   groups > 0   that many persistent workgroups
 *   groups = -1  auto: num_cus × the resident workgroups per CU of the kernel that runs, for the
 *                flows where the queue measured faster (D = 3, N = 128, four problems
 *                per 512-thread workgroup, BLS and GD dual loop); the static launch otherwise
 * Other values, or a NULL ctx, return IRM_EINVAL.  The setting applies to every later
 * irm_optimize_batch(_dev) on the context; contexts that never call this take IRM_WORK_QUEUE=off|auto|<n>
 * from the environment (unset: off).  A launch keeps the static launch — and the query below returns
 * 0 — when `groups` would cover every workgroup of the static launch (groups ≥ ⌈batch/traj_per_block⌉),
 * when it records a series, and when it dispatches to a kernel without the queue (the GD single loop,
 * k_optimize, the dense operator, two waypoints per lane, shapes other than D = 3 at N = 50 / 64 / 128 and
 * D = 7 at N = 128).
 * The 4-byte counter belongs to the context and is set by stream work ahead of the kernel
 * (enqueue-only for _dev): at most one queued launch per context may be in flight.
 * Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout; no reference counterpart. */
int irm_set_work_queue(irm_ctx* ctx, int32_t groups);
/* The persistent workgroups that a launch of these arguments would run (the arguments of
 * irm_optimize_plan), 0 for the static launch, a negative IRM_E* code on failure.  Filled in by the
 * launch dispatch itself with nothing launched.  While the queue is active irm_optimize_plan reports
 * this number as `grid` and a kernel label ending in ",QUEUE>". */
int irm_work_queue_groups(const irm_ctx* ctx, int32_t batch, int32_t n_obstacles, int32_t record_series);

/* Evaluation at arbitrary times (eval_any): the trajectory is the RKHS function q(t) = K(·, t)·α·J,
 * v(t) = dK(·, t)·α·J for any t (DevBlog-Theme/blog-post.html:119-131; Trajectory.eval_any,
 * trajectory.py:68-70).  A context holds one grid of M evaluation times and its query matrices Kq, dKq
 * (M×N): row i is the evaluation time t_eval[i], column j the support time t[j], and the entry is
 * kernel_f(t[j], t_eval[i]) in the arithmetic of K / dK (fp32 d = t[j] − t_eval[i]), so t_eval = t
 * gives K and dK themselves.  (The reference's eval_any hands create_kernel_matrix its arguments in the
 * other order and is never called; this is what its km / dkm and the blog's formula define.)
 * Times need not be sorted nor lie in [0, 1]; a non-finite time, or M outside [1, IRM_MAX_EVAL_TIMES],
 * is IRM_EINVAL.  Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout. */
#define IRM_MAX_EVAL_TIMES 4096
/* Kq, dKq (M×N, row = evaluation time) for N support times linspace(0,1,N) as Trajectory.__init__ builds
 * them; outputs nullable.  Needs no context and no device. */
int irm_query_matrices(int32_t n_timesteps, float rbf_variance, const float* t_eval, int32_t M, float* kq, float* dkq);
/* Builds and uploads Kq / dKq for t_eval (M); replaces the previous grid. */
int irm_set_eval_times(irm_ctx* ctx, const float* t_eval, int32_t M);
/* The M currently set (0 if none; a negative IRM_E* code on failure); t_out (nullable) receives the times. */
int32_t irm_eval_times(const irm_ctx* ctx, float* t_out);
/* blog :121-131 / trajectory.py:68-70: out (B×M×D) = Kq·α·J (which 0) or dKq·α·J (which 1), with
 * irm_evaluate's arithmetic (fp64 sum of the exact products over m = 0..N−1, one rounding, then ·J the
 * same way).  IRM_EINVAL before any irm_set_eval_times; batch = 0 is a no-op. */
int irm_eval_any(irm_ctx* ctx, const float* alpha, int32_t batch, int32_t which, float* out);
/* Limits and obstacle clearance of B trajectories on the M evaluation times (one record per trajectory).
 * The start/goal terms are not part of it: they live on the support grid's end points (irm_constraints). */
typedef struct irm_dense_report {
    float max_cost, avg_cost;          /* obstacle cost over the M times: end effector, or whole robot if the context says so */
    int32_t argmax_cost;               /* first index into t_eval attaining max_cost */
    float max_position, min_position;  /* over times and joints, as trajectory.max()/min() in constraintsFulfilledVerbose */
    float max_abs_velocity;
    int32_t argmax_abs_velocity;       /* first index into t_eval */
    int32_t position_ok, velocity_ok;  /* robot.py:104-113 applied to the M samples */
    int32_t pad_;
} irm_dense_report;
/* obstacles: O×2 (obstacle_stride 0) or one table per trajectory, as irm_optimize_batch takes them.
 * cost_out: B×M per-sample obstacle cost, nullable. */
int irm_dense_check(irm_ctx* ctx, const float* alpha, const float* obstacles, int32_t n_obstacles, int32_t obstacle_stride,
                    int32_t batch, irm_dense_report* report_out, float* cost_out);
/* Same, device pointers, enqueue-only on `stream` (hipStream_t). */
int irm_dense_check_dev(irm_ctx* ctx, const float* alpha_dev, const float* obstacles_dev, int32_t n_obstacles,
                        int32_t obstacle_stride, int32_t batch, irm_dense_report* report_dev, float* cost_dev, void* stream);

/* Fitting and re-timing (fit_alpha, transfer_alpha): project a trajectory that is known by its N waypoints
 * on this context's support grid, or by the α of another support grid, onto this context's grid.  Both are
 * the ridge fit of DESIGN.md §2: with t the context's support times and K its fp32 kernel matrix,
 *   W = (K + ρI)⁻¹                                  N×N fp64, symmetric to the bit: Cholesky of the fp32 entries of K
 *                                                    widened, factored in extended precision, rounded to fp64 once
 *   T = W·Kx,  Kx[i][j] = rbf_kernel(t_src[j], s_i)  N×n_src, t_src = linspace(0, 1, n_src), kernel width σ_src,
 *                                                    s_i = t0 + (t1 − t0)·t_i in fp32, Kx in irm_query_matrices'
 *                                                    fp32 arithmetic, widened
 * so that K·(T·α_src)·J is the ridge-smoothed source trajectory at the mapped times s_i (the remaining motion
 * from t0 to t1 stretched to unit time: velocities are (t1 − t0) times the source's).  The device applies the
 * operators in fp64, one FMA chain per output element in the order m = 0, 1, …, one rounding to fp32:
 *   fit       α[n][k]  = fp32( Σ_m W[n][m]·( Σ_d Q[m][d]·Jinv[d][k] ) )      Jinv: the context's fp32 J⁻¹
 *   transfer  α'[n][k] = fp32( Σ_m T[n][m]·α_src[m][k] )
 *   start_out[k] = the source trajectory at s_0 = t0, in irm_eval_any's arithmetic for the single time t0
 * A problem's result does not depend on the rest of its batch.  ρ (a float, widened) must be finite and > 0;
 * a Cholesky factorisation that meets a non-positive pivot is IRM_EINVAL (the fp32-rounded K stops being
 * positive definite below ρ ≈ 1e-6).  n_src must lie in [2, IRM_MAX_TIMESTEPS]; t0, t1 finite, t0 < t1.
 * W is built at first use with the context's ridge; W and T live on the device in fp64, transposed.
 * Outputs must not overlap inputs.  Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout;
 * no reference counterpart. */
#define IRM_FIT_RIDGE_DEFAULT 1e-6f
/* Host only, no context, no device (like irm_query_matrices): out = W (n×n, n_src = 0) or T (n×n_src,
 * n_src > 0; rbf_variance_src ≤ 0: rbf_variance), row-major fp64, for n support times linspace(0, 1, n). */
int irm_fit_operator(int32_t n, float rbf_variance, float ridge, int32_t n_src, float rbf_variance_src, float t0,
                     float t1, double* out);
/* The ridge of every later fit / transfer on the context: rebuilds W and drops a transfer that was set.  On
 * failure the context keeps its previous ridge, W and transfer. */
int irm_set_fit_ridge(irm_ctx* ctx, float ridge);
/* α (B×N×D) whose trajectory K·α·J is the ridge fit of the waypoints traj (B×N×D); batch = 0 is a no-op. */
int irm_fit_alpha(irm_ctx* ctx, const float* traj, int32_t batch, float* alpha_out);
/* Builds and uploads T for a source grid of n_src support times, kernel width rbf_variance_src (≤ 0: the
 * context's) and the time map [0, 1] → [t0, t1]; replaces the previous transfer. */
int irm_set_transfer(irm_ctx* ctx, int32_t n_src, float rbf_variance_src, float t0, float t1);
/* α' (B×N×D) from α_src (B×n_src×D); start_out (B×D, nullable) receives the source trajectory at t0.
 * IRM_EINVAL before any irm_set_transfer; batch = 0 is a no-op. */
int irm_transfer_alpha(irm_ctx* ctx, const float* alpha_src, int32_t batch, float* alpha_out, float* start_out);
/* Same, device pointers, enqueue-only on `stream` (hipStream_t); the first fit on a context builds and
 * uploads W before it enqueues. */
int irm_fit_alpha_dev(irm_ctx* ctx, const float* traj_dev, int32_t batch, float* alpha_dev, void* stream);
int irm_transfer_alpha_dev(irm_ctx* ctx, const float* alpha_src_dev, int32_t batch, float* alpha_dev,
                           float* start_dev, void* stream);

/* Moving obstacles: constant-velocity prediction inside a plan.  Every obstacle o has a velocity w_o
 * (displacement per unit of plan time; the plan runs over t ∈ [0, 1]), and a waypoint at plan time τ sees
 * obstacle o at
 *   x = fmaf(τ, w_x, p_x),  y = fmaf(τ, w_y, p_y)         fp32, one fused multiply-add per coordinate
 * From there the potential's arithmetic is the static one's (environment.py:46-58 as the kernels evaluate it).
 * τ is the support time t[n] — the fp32 value irm_kernel_matrices returns — for the cost, the gradient and
 * every round of the optimiser, and t_eval[i] for irm_dense_check_moving.  The obstacle moves with time, not
 * with α: the gradient is the static formula with each waypoint's own obstacle positions, no new term; the
 * max-cost term, the mean weighting and the whole-robot cost (every joint position of waypoint n sees the
 * table at t[n]) compose unchanged.
 * obstacle_velocity is fp32 with the shape and stride of `obstacles` (O×2 shared, or one table per problem
 * at obstacle_stride).  NULL means the static call: the same dispatch and the same bits as the entry point
 * without _moving.  An all-zero table gives the same kernel's static result to the bit (fmaf(τ, 0, p) = p).
 * A moving optimiser launch runs the general kernel k_optimize<DynShape<D>> (as a whole-robot launch does;
 * the shape-specialised k_lean kernels and the work queue have no moving variant) with a second obstacle
 * table in LDS; where no trajectories-per-workgroup fits the 160 KiB the call is IRM_EINVAL (possible at
 * N = 512 with many per-problem obstacles) — nothing falls back to the static table.
 * Host-pointer entry points reject a non-finite velocity with IRM_EINVAL; the _dev entry points cannot see
 * the values and do not check them.  irm_compute_cost_vg takes free points without times and stays static.
 * Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout; no reference counterpart. */
int irm_eval_cost_moving(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                         const float* obstacles, int32_t n_obstacles, int32_t batch,
                         float lambda_sg, float lambda_jl, float lambda_max, float* cost_out,
                         const float* obstacle_velocity);
int irm_eval_cost_grad_moving(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                              const float* obstacles, int32_t n_obstacles, int32_t batch,
                              float lambda_sg, float lambda_jl, float lambda_max,
                              float* grad_out, float* cost_out, const float* obstacle_velocity);
int irm_optimize_batch_moving(irm_ctx* ctx, const float* alpha0, const float* start, const float* goal,
                              const float* obstacles, int32_t n_obstacles, int32_t obstacle_stride,
                              int32_t batch, float* alpha_out, float* traj_out, irm_stats* stats_out,
                              float* series_out, const float* obstacle_velocity);
/* Device pointers, enqueue-only on `stream`; the velocity table uses args->n_obstacles / obstacle_stride. */
int irm_optimize_batch_moving_dev(irm_ctx* ctx, const irm_batch_dev* args, const float* obstacle_velocity_dev,
                                  void* stream);
int irm_dense_check_moving(irm_ctx* ctx, const float* alpha, const float* obstacles, int32_t n_obstacles,
                           int32_t obstacle_stride, int32_t batch, irm_dense_report* report_out, float* cost_out,
                           const float* obstacle_velocity);
int irm_dense_check_moving_dev(irm_ctx* ctx, const float* alpha_dev, const float* obstacles_dev, int32_t n_obstacles,
                               int32_t obstacle_stride, int32_t batch, irm_dense_report* report_dev, float* cost_dev,
                               const float* obstacle_velocity_dev, void* stream);
/* irm_optimize_plan for a moving launch of the same arguments: the kernel such a launch runs. */
int irm_optimize_plan_moving(const irm_ctx* ctx, int32_t batch, int32_t n_obstacles, int32_t record_series,
                             irm_launch_plan* out);

/* Clearance: the signed distance between the arm's links and disc obstacles on the evaluation times — does the
 * arm touch anything, and by how much does it miss?  The obstacle potential is a cost at points (the end effector,
 * or the joints with whole_robot_cost); a link is the segment between two joints and can pass over an obstacle
 * that both of its joints clear.  For trajectory b, evaluation time i of the context's grid (irm_set_eval_times),
 * link l = 0 … D−1 and obstacle o, everything in fp32 and in this order:
 *   q        the position sample at t_eval[i], irm_eval_any's arithmetic and bits
 *   c_l      = c_{l−1} + q_l                                  (c_0 = q_0), and the rounding of that addition kept:
 *   τ_l      = τ_{l−1} + ((c_{l−1} − (c_l − b)) + (q_l − b)),  b = c_l − c_{l−1},  τ_0 = 0      (two-sum: the bracket
 *              is exactly (c_{l−1} + q_l) − c_l, so c_l + τ_l is the angle sum to second order)
 *   sn0, cs0 = the kernels' sincos of c_l (the polynomial of the obstacle potential's FK; sincosf above 1e4 rad)
 *   sn, cs   = fmaf(τ_l, cs0, sn0), fmaf(−τ_l, sn0, cs0)      sin and cos of c_l + τ_l to first order in τ_l.  Without
 *              it the fp32 prefix sum alone moves a joint of a 7-link arm by 1.3e-6 at angles of 13 rad
 *   x_l      = fmaf(L_l, cs_l, x_{l−1}),  y_l = fmaf(L_l, sn_l, y_{l−1}),  p_{−1} = (0, 0): the joint positions, in
 *              the order of the potential's FK (to the bit where every τ_l is 0)
 *   link l   the segment from p_{l−1} to p_l, with direction e = (L_l·cs_l, L_l·sn_l) — one product each, not the
 *              difference of two positions — and inverse squared length w_l = 1/(L_l·L_l), an IEEE division
 *   obstacle the table entry, or on a moving launch fmaf(t_eval[i], w, p) per coordinate as irm_dense_check_moving
 *   u        = o − p_{l−1}                                    per coordinate
 *   s        = min(max(fmaf(u_y, e_y, u_x·e_x)·w_l, 0), 1)    the projection onto the segment, clamped
 *   r        = (fmaf(−s, e_x, u_x), fmaf(−s, e_y, u_y))
 *   d        = sqrt(fmaf(r_y, r_y, r_x·r_x))                  the IEEE (correctly rounded) square root
 *   g        = (d − radius_o) − link_radius                   the signed clearance, in that order
 * radius_o is 0 without a radius table; link_radius ≥ 0 is one scalar for the whole arm (a capsule per link).
 * Sample i has c_i = min over (l, o) of g and collides iff c_i < 0 (g = 0, touching, does not); the report's
 * minimum is min over i of c_i.  Ties go to the lexicographically lowest (i, l, o).  With no obstacles every c_i
 * and the minimum are +INFINITY, every argmin is −1 and nothing collides.  link_out[l] is the minimum of g over
 * the samples and obstacles for link l alone.  The verdict covers the M samples, not the time between them; the
 * links are not checked against each other here (irm_self_clearance below does that).
 * obstacle_radius: O floats shared by the batch (obstacle_stride 0), else one table per problem at
 * obstacle_stride/2 floats (an odd stride with a radius table is IRM_EINVAL).  obstacle_velocity: as
 * irm_dense_check_moving; NULL and an all-zero table give the same bits.  IRM_EINVAL: no evaluation grid, a
 * negative batch, n_obstacles outside [0, IRM_MAX_OBSTACLES], obstacles missing with n_obstacles > 0, a negative or
 * non-finite link_radius and, on the host entry point (which sees the values), a negative or non-finite radius or
 * a non-finite velocity.  batch = 0 is a no-op.  A problem's result does not depend on the rest of the batch.
 * Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout; no reference counterpart. */
typedef struct irm_clearance_report {
    float min_clearance;
    int32_t argmin_time, argmin_link, argmin_obstacle; /* indices into t_eval, links, obstacles; -1 if n_obstacles = 0 */
    int32_t n_colliding, first_colliding;              /* samples with c_i < 0; first index into t_eval or -1 */
    int32_t collision_free;                            /* n_colliding == 0 */
    int32_t pad_;
} irm_clearance_report;
/* report_out: B records.  clear_out B×M (c_i), link_out B×D, joints_out B×M×D×2 (x_l, y_l of every sample, the
 * positions the distances were taken from): each nullable. */
int irm_clearance(irm_ctx* ctx, const float* alpha, const float* obstacles, int32_t n_obstacles, int32_t obstacle_stride,
                  const float* obstacle_velocity, const float* obstacle_radius, float link_radius, int32_t batch,
                  irm_clearance_report* report_out, float* clear_out, float* link_out, float* joints_out);
/* Same, device pointers, enqueue-only on `stream` (hipStream_t). */
int irm_clearance_dev(irm_ctx* ctx, const float* alpha_dev, const float* obstacles_dev, int32_t n_obstacles,
                      int32_t obstacle_stride, const float* obstacle_velocity_dev, const float* obstacle_radius_dev,
                      float link_radius, int32_t batch, irm_clearance_report* report_dev, float* clear_dev,
                      float* link_dev, float* joints_dev, void* stream);

/* Self-clearance: the signed distance between the arm's own links on the evaluation times — does the arm touch
 * itself?  irm_clearance checks the links against obstacles and not against each other; the optimiser's cost sees
 * points only, so nothing stops a plan that folds the arm through itself.  For trajectory b, evaluation time i of
 * the context's grid (irm_set_eval_times) and the link pairs (a, b) with 0 ≤ a, a + 2 ≤ b ≤ D − 1 — adjacent links
 * share a joint and are never a pair — in lexicographic order (0,2), (0,3), …, (D−3, D−1), P = (D−1)(D−2)/2 of
 * them, everything in fp32 and in this order:
 *   q, c_l, τ_l, sn, cs, p_l   irm_clearance's, bit for bit (one shared prefix in the kernels), p_{−1} = (0, 0)
 *   e_l, w_l   = (L_l·cs_l, L_l·sn_l), 1/(L_l·L_l)              irm_clearance's link direction and inverse squared length
 *   segment l  from A = p_{l−1} to p_l with direction e_l; the far end point is the stored joint position p_l, not A + e
 *   dist(x; A, e, w):  u = x − A                                  per coordinate
 *                      s = min(max(fmaf(u_y, e_y, u_x·e_x)·w, 0), 1)
 *                      r = (fmaf(−s, e_x, u_x), fmaf(−s, e_y, u_y))
 *                      d = sqrt(fmaf(r_y, r_y, r_x·r_x))          the IEEE (correctly rounded) square root
 *   orient(x; A, e) = fmaf(u_x, e_y, −(u_y·e_x)),  u = x − A     which side of the link's line x lies on
 *   d1, o1     = dist, orient(p_{b−1}; link a)      d2, o2 = dist, orient(p_b; link a)
 *   d3, o3     = dist, orient(p_{a−1}; link b)      d4, o4 = dist, orient(p_a; link b)
 *   crossing   o1 and o2 have strictly opposite signs and o3 and o4 have strictly opposite signs: the signs are
 *              compared, not a product (which can underflow to 0 or lose its sign), and a zero is not a sign — the
 *              end-point distances cover touching and collinear overlap
 *   d          = 0 if the pair crosses, else min(d1, d2, d3, d4)
 *   g          = d − 2·link_radius                                the signed clearance of two capsules
 * The pair collides iff it crosses or g < 0 (g = 0 without a crossing, touching, does not — irm_clearance's
 * convention; with link_radius = 0 a collision is exactly a crossing).  Sample i has c_i = min over the pairs of g
 * and collides iff one of its pairs does; the report's minimum is min over i of c_i.  Ties go to the
 * lexicographically lowest (i, a, b).  With P = 0 (D ≤ 2) every c_i and the minimum are +INFINITY, every argmin is
 * −1 and nothing collides.  pair_out[p] is the minimum of g over the samples for pair p alone, in the pair order.
 * The verdict covers the M samples, not the time between them; one radius for the whole arm; the base is no body.
 * IRM_EINVAL: no evaluation grid, a negative batch, a negative or non-finite link_radius, a NULL alpha or report.
 * batch = 0 is a no-op.  A problem's result does not depend on the rest of the batch.
 * Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout; no reference counterpart. */
typedef struct irm_self_clearance_report {
    float min_clearance;
    int32_t argmin_time, argmin_link_a, argmin_link_b; /* indices into t_eval and the links (a + 2 ≤ b); -1 if D ≤ 2 */
    int32_t n_colliding, first_colliding;              /* samples with a colliding pair; first index into t_eval or -1 */
    int32_t collision_free;                            /* n_colliding == 0 */
    int32_t n_crossing;                                /* samples where some pair crosses */
} irm_self_clearance_report;
/* report_out: B records.  clear_out B×M (c_i), pair_out B×P, joints_out B×M×D×2 (x_l, y_l of every sample: the bits
 * of irm_clearance's joints_out for the same α and grid): each nullable. */
int irm_self_clearance(irm_ctx* ctx, const float* alpha, float link_radius, int32_t batch,
                       irm_self_clearance_report* report_out, float* clear_out, float* pair_out, float* joints_out);
/* Same, device pointers, enqueue-only on `stream` (hipStream_t); allocates nothing. */
int irm_self_clearance_dev(irm_ctx* ctx, const float* alpha_dev, float link_radius, int32_t batch,
                           irm_self_clearance_report* report_dev, float* clear_dev, float* pair_dev, float* joints_dev,
                           void* stream);

/* End-effector goals: plan to a Cartesian target.  A problem may carry goal_xy = (p_x, p_y); row N−1 of the
 * trajectory is then held to the target through the end-effector FK f (robot.py:29-36) and its 2×D Jacobian
 * J_ee (robot.py:75-87) instead of to the joint configuration `goal`.  Three places change, nothing else:
 *   loss (trajectory.py:187)        ½‖T[N−1] − g‖²        becomes  ½‖f(T[N−1]) − p‖²
 *   gradient input a[N−1]           λsg·(T[N−1] − g)      becomes  λsg·J_ee(T[N−1])ᵀ·(f(T[N−1]) − p)
 *   constraintsFulfilled            ‖T[N−1] − g‖ < eps_position  becomes  ‖f(T[N−1]) − p‖ < eps_position
 * The goal-velocity term, the start terms, the obstacle term (end effector or whole robot, static or moving)
 * and the joint-limit terms are untouched.  The Jacobian is the end effector's also with whole_robot_cost = 1.
 * f and J_ee are the values the waypoint's own evaluation forms (the FK that feeds the obstacle potential), no
 * second FK.  fp32 order, with e_x = f_x − p_x, e_y = f_y − p_y:
 *   r²    = fmaf(e_y, e_y, e_x·e_x)                   in place of Σ_d (T[N−1][d] − g[d])²
 *   ge[d] = fmaf(J_y[d], e_y, J_x[d]·e_x)             in place of T[N−1][d] − g[d]
 * and from there the joint-goal arithmetic (½·r² into the loss, sqrtf(r²) against eps_position, λsg·ge[d] into
 * a[N−1][d]).  eps_position therefore bounds a length (the unit of the link lengths) in such a call, where it
 * bounds radians in a joint-goal call.
 * goal_xy is B×2 fp32.  NULL means the existing call: the same dispatch and the same bits as the entry point
 * without _task (including which launches stay on the shape-specialised k_lean kernels).  `goal` (B×D) is
 * still passed; it feeds only the straight-line initialisation when alpha0 is NULL.  obstacle_velocity stays
 * nullable (the _task forms are the superset of the _moving forms).  An end-effector-goal optimiser launch runs
 * the general kernel k_optimize<DynShape<D>>, every flow (GD single loop, GD dual loop, BLS), with series
 * recording if asked; k_lean and the work queue have no such variant (a queued context runs the static launch
 * for such a call), and a shape that does not fit the LDS is IRM_EINVAL.  irm_stats.final_loss and
 * constraints_ok follow the task loss and the task constraint; report[1] of irm_constraints_task is
 * ‖f(τ_{N−1}) − p‖.  Host-pointer entry points reject a non-finite goal_xy with IRM_EINVAL; the _dev entry
 * points cannot see the values.  The reference's --gd-lr schedule was tuned for the joint-space penalty: with
 * default hyper-parameters the end-to-end guarantee (constraints_ok from an IK seed) is stated for BLS.
 * Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout; no reference counterpart. */
int irm_eval_cost_task(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                       const float* obstacles, int32_t n_obstacles, int32_t batch,
                       float lambda_sg, float lambda_jl, float lambda_max, float* cost_out,
                       const float* obstacle_velocity, const float* goal_xy);
int irm_eval_cost_grad_task(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                            const float* obstacles, int32_t n_obstacles, int32_t batch,
                            float lambda_sg, float lambda_jl, float lambda_max,
                            float* grad_out, float* cost_out, const float* obstacle_velocity,
                            const float* goal_xy);
int irm_constraints_task(irm_ctx* ctx, const float* alpha, const float* start, const float* goal, int32_t batch,
                         uint8_t* ok_out, float* report_out, const float* goal_xy);
int irm_optimize_batch_task(irm_ctx* ctx, const float* alpha0, const float* start, const float* goal,
                            const float* obstacles, int32_t n_obstacles, int32_t obstacle_stride,
                            int32_t batch, float* alpha_out, float* traj_out, irm_stats* stats_out,
                            float* series_out, const float* obstacle_velocity, const float* goal_xy);
/* Device pointers, enqueue-only on `stream`; goal_xy_dev is args->batch × 2. */
int irm_optimize_batch_task_dev(irm_ctx* ctx, const irm_batch_dev* args, const float* obstacle_velocity_dev,
                                const float* goal_xy_dev, void* stream);
/* irm_optimize_plan for an end-effector-goal launch of the same arguments: the kernel such a launch runs. */
int irm_optimize_plan_task(const irm_ctx* ctx, int32_t batch, int32_t n_obstacles, int32_t record_series,
                           irm_launch_plan* out);
/* IK seed: a joint configuration whose end effector is at goal_xy, by damped least squares started at `start`
 * (B×D), one problem per lane, fp32.  32 iterations of
 *   e = f(q) − p;  dq = −J_eeᵀ·(J_ee·J_eeᵀ + μ²I)⁻¹·e, μ = 0.1, the 2×2 system solved in closed form;
 *   dq scaled so that max|dq| ≤ 0.5;  q ← clamp(q + dq, joint_safety_limit·min_joint_position,
 *                                                      joint_safety_limit·max_joint_position)
 * q_out (B×D) is the last q and residual_out (B, nullable) its ‖f(q) − p‖.  Best effort: a target outside the
 * reach or behind the joint limits keeps a residual and the call still returns IRM_OK — which is why the
 * residual is an output.  One branch only (the one the damped steps from `start` lead to).  A problem's result
 * does not depend on its batch.  irm_ik_seed rejects a non-finite goal_xy with IRM_EINVAL. */
int irm_ik_seed(irm_ctx* ctx, const float* start, const float* goal_xy, int32_t batch, float* q_out,
                float* residual_out);
int irm_ik_seed_dev(irm_ctx* ctx, const float* start_dev, const float* goal_xy_dev, int32_t batch, float* q_dev,
                    float* residual_dev, void* stream);

/* Via-points: hold interior support rows to joint or Cartesian targets.  A call may carry V via-points,
 * 1 ≤ V ≤ IRM_MAX_VIA.  Via-point v names a support row m_v (strictly increasing, each in [1, N−2]) and a kind;
 * the row table and the kinds are shared by the batch (a row is a via row for every problem), the targets are
 * per problem: target is B×V×D fp32.  A joint via-point (cartesian = 0) uses all D values c; an end-effector
 * via-point (cartesian = 1, D ≥ 2) uses the first two values p and ignores the rest.  Three places change,
 * nothing else:
 *   loss         += λsg · ½ · Σ_v r_v²
 *   a[m_v]       += λsg · ge_v            (position gradient input of row m_v only)
 *   constraints  :  ok  &=  sqrtf(r_v²) < eps_position   for every v
 * Joint:        e[d] = T[m_v][d] − c[d], ge_v = e, r_v² = Σ_d e[d]² accumulated as the same kernel accumulates
 *               row N−1 against `goal` (cost / gradient / constraints: a += e·e; the optimiser: fmaf(e, e, a)).
 * End effector: e = f(T[m_v]) − p, r_v² = fmaf(e_y, e_y, e_x·e_x), ge_v[d] = fmaf(J_y[d], e_y, J_x[d]·e_x) — the
 *               end-effector-goal order above, f and J_ee from the waypoint's own evaluation (no second FK);
 *               J_ee is the end effector's also with whole_robot_cost = 1.
 * The velocity of a via row is free: no term enters b, and the sparse-velocity logic of the optimiser keeps seeing
 * only rows 0 and N−1 — the robot passes through a via-point, it does not stop there (chaining two plans would).
 * fp32 order of the loss: the via terms join the start/goal position sum in index order after the existing two,
 *   cost / gradient / constraints:  s = 0.5·a0 + 0.5·a1;           then for v = 0 … V−1:  s = s + 0.5·r_v²
 *   the optimiser:                  s = fmaf(0.5, a0, 0.5·a1);     then for v = 0 … V−1:  s = fmaf(0.5, r_v², s)
 * and λsg·ge_v[d] enters a[m_v][d] where λsg·(T[N−1] − g)[d] enters a[N−1][d] (one fmaf onto the obstacle term).
 * λsg is the call's or round's current value: the dual loop and BLS escalate it with the rest until eps_position
 * holds.  irm_stats.final_loss and constraints_ok follow the via loss and the via constraint.  Via-points compose
 * with goal_xy, obstacle_velocity (both stay nullable: the _via forms are the superset of the _task forms),
 * whole_robot_cost, per-problem obstacle tables and series recording.
 * via = NULL or n_via = 0 is the existing call: the same dispatch and the same bits as the _task entry point
 * (including which launches stay on the shape-specialised k_lean kernels and on the work queue).  A via launch
 * runs the general kernel k_optimize<DynShape<D>>, every flow, as moving and end-effector-goal launches do;
 * k_lean and the work queue have no via variant (a queued context runs the static launch for such a call).  The
 * via words r_v² take IRM_MAX_VIA floats of LDS per trajectory of a workgroup; a shape that no longer fits is
 * IRM_EINVAL.
 * IRM_EINVAL (with a message): V outside [0, IRM_MAX_VIA]; a row outside [1, N−2] or rows not strictly
 * increasing; a cartesian value other than 0 or 1; a Cartesian via-point at D = 1; a NULL target with V > 0; in
 * the host-pointer forms a non-finite value among the target entries that are read (D per joint via-point, 2 per
 * end-effector one).  The _dev form cannot see the values.
 * Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout; no reference counterpart. */
#define IRM_MAX_VIA 4
typedef struct irm_via {
    int32_t n_via;
    int32_t row[IRM_MAX_VIA];        /* strictly increasing, each in [1, N−2] */
    int32_t cartesian[IRM_MAX_VIA];  /* 0 joint target, 1 end-effector target */
    const float* target;             /* B×V×D (host pointer; device pointer in the _dev form) */
} irm_via;
int irm_eval_cost_via(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                      const float* obstacles, int32_t n_obstacles, int32_t batch,
                      float lambda_sg, float lambda_jl, float lambda_max, float* cost_out,
                      const float* obstacle_velocity, const float* goal_xy, const irm_via* via);
int irm_eval_cost_grad_via(irm_ctx* ctx, const float* alpha, const float* start, const float* goal,
                           const float* obstacles, int32_t n_obstacles, int32_t batch,
                           float lambda_sg, float lambda_jl, float lambda_max,
                           float* grad_out, float* cost_out, const float* obstacle_velocity,
                           const float* goal_xy, const irm_via* via);
/* via_dist_out: B×V, nullable, sqrtf(r_v²).  The 11-float report is the _task form's; ok_out includes the via
 * flags. */
int irm_constraints_via(irm_ctx* ctx, const float* alpha, const float* start, const float* goal, int32_t batch,
                        uint8_t* ok_out, float* report_out, const float* goal_xy, const irm_via* via,
                        float* via_dist_out);
int irm_optimize_batch_via(irm_ctx* ctx, const float* alpha0, const float* start, const float* goal,
                           const float* obstacles, int32_t n_obstacles, int32_t obstacle_stride,
                           int32_t batch, float* alpha_out, float* traj_out, irm_stats* stats_out,
                           float* series_out, const float* obstacle_velocity, const float* goal_xy,
                           const irm_via* via);
/* Device pointers, enqueue-only on `stream`; via->target is a device pointer, args->batch × V × D (the struct
 * itself is read on the host, during the call). */
int irm_optimize_batch_via_dev(irm_ctx* ctx, const irm_batch_dev* args, const float* obstacle_velocity_dev,
                               const float* goal_xy_dev, void* stream, const irm_via* via);
/* irm_optimize_plan for a via launch of the same arguments: the kernel such a launch runs.  Only n_via, row and
 * cartesian are read (target may be NULL); via = NULL is irm_optimize_plan_task.  Like irm_optimize_plan_task it
 * takes no velocity table: it describes the launch with static obstacles.  A via launch that also carries
 * obstacle_velocity runs the same kernel with the second obstacle table in LDS, so its lds_bytes is larger and,
 * where that no longer fits, its traj_per_block smaller than reported here. */
int irm_optimize_plan_via(const irm_ctx* ctx, int32_t batch, int32_t n_obstacles, int32_t record_series,
                          irm_launch_plan* out, const irm_via* via);

/* Multi-start planning: seed ensembles ranked and gathered on the device.  One optimize call is one descent from
 * one seed in a landscape that is not convex; a multi-start call runs S seeds per problem in one launch and keeps
 * the best by a stated order.  Candidates are rows, problem-major: candidate s of problem b is row b·S + s,
 * 1 ≤ S ≤ IRM_MAX_SEEDS.
 *
 * The ensemble.  Candidate 0 is the α of the straight-line initialisation, bit for bit (the expression
 * α0 = u⊗(s·J⁻¹) + w⊗(g·J⁻¹) of Trajectory.initTrajectory as this library evaluates it); its waypoints output is
 * the plain line, base below.  Candidate s ≥ 1 has the waypoints, fp32, for support row n and joint d
 *   base = fmaf(c_n, goal_d − start_d, start_d)          c_n: the smooth step 6t⁵ − 15t⁴ + 10t³ of the support time
 *                                                        t_n, the fp32 table the operator build forms
 *   q    = fmaf(φ_n, a, base)                            φ_n = 16·(p·p), p = t_n·(1 − t_n), fp32: value and slope 0
 *                                                        at both ends, peak 1; a host-built table, uploaded once
 *   q    = min(max(q, lo), hi)                           lo / hi = joint_safety_limit·min / max_joint_position, the
 *                                                        bounds the IK seed clamps to
 * and its α is the ridge fit's arithmetic on these waypoints (Fitting and re-timing above: the same fp64 FMA chains,
 * the same W, one rounding), so it is bit-identical to the fit of the waypoints output.  The amplitude is
 *   a = fmaf(2A, U, −A),  U = (h >> 8)·2⁻²⁴ (exact in fp32),
 *   h = fmix32(fmix32(fmix32(fmix32(seed ^ 0x243F6A88) + (problem_offset + b)) + s) + d)
 * in uint32 arithmetic, fmix32 being MurmurHash3's finaliser (h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13;
 * h *= 0xC2B2AE35; h ^= h >> 16).  A candidate depends on (seed, problem_offset + b, s, d) and its problem's start
 * and goal only — not on S, the batch or the rest of it: ensembles nest (the first 4 candidates of 8 are the 4 of 4)
 * and a shard that passes its first problem's global index as problem_offset reproduces the unsharded rows.
 * A = 0 gives S copies of the clamped line behind candidate 0.
 *
 * The ranking.  The key of a candidate is (class, loss, s), compared lexicographically:
 *   class = 2·(constraints_ok == 0) + (n_colliding > 0)     (without reports: 2·(constraints_ok == 0))
 *   loss  = final_loss; a NaN loss puts the candidate in class 4 with its loss compared as +INFINITY
 *   ties go to the lower s (−0 and +0 compare equal)
 * rank[b·S + s] is the position of candidate s in its problem's order (a permutation of 0 … S−1) and winner[b] the
 * candidate at position 0.  One wave per problem, one lane per candidate.
 *
 * The call.  On one stream: seeds → the per-problem rows (start, goal, goal_xy, per-problem obstacle, velocity and
 * radius tables) replicated S times → the existing optimiser launch of irm_optimize_batch_dev (its _moving / _task
 * twin with a velocity table / goal_xy) on the B·S problems with alpha0 = the seeds → with rank_clearance the
 * existing clearance check on the B·S results → ranking → the winner's rows gathered into the B-sized outputs.
 * Every candidate is therefore, to the bit, the plain optimize of its replicated problem from its seed, its report
 * the plain clearance check of its α, and n_seeds = 1 is the plain optimize from the straight-line α.  With goal_xy
 * and a NULL goal the goal configuration (of every candidate) is the IK seed's for (start, goal_xy).
 * IRM_EINVAL (with a message naming the argument): n_seeds outside [1, IRM_MAX_SEEDS]; a negative or non-finite
 * amplitude; a negative problem_offset; rank_clearance without an evaluation grid; obstacle_radius or a non-zero
 * link_radius without rank_clearance; alpha0 (the seeds are the call's own); series recording (series_out, or a
 * context that records); a workspace smaller than the sizing function's answer.  Via-points have no multi-start form:
 * the via seed is a path of its own.
 * The _dev forms only enqueue and allocate nothing (the first seed call on a context uploads the fit operator and
 * the c / φ tables before it enqueues): the caller passes workspace_bytes ≥ the sizing function's answer for the same
 * batch, n_seeds, n_obstacles and obstacle_stride, 256-byte aligned.  Outputs must not overlap inputs or the
 * workspace.  Additive symbols: IRM_ABI_VERSION stays 3 and no struct changes layout; no reference counterpart. */
#define IRM_MAX_SEEDS 64
typedef struct irm_multistart {
    int32_t n_seeds;               /* S */
    uint32_t seed;
    float amplitude;               /* A ≥ 0, finite: the bump amplitudes are uniform in [−A, A) */
    int32_t problem_offset;        /* global index of this call's problem 0 (a shard's offset), ≥ 0 */
    int32_t rank_clearance;        /* 1: run the clearance check on every candidate and rank with n_colliding */
    float link_radius;             /* of the clearance check */
    const float* obstacle_radius;  /* of the clearance check, nullable: O shared, or per problem at obstacle_stride/2
                                      (host pointer; device pointer in the _dev form) */
} irm_multistart;
/* What a multi-start call returns beside the winner's rows; every pointer but winner nullable (host pointers; device
 * pointers in the _dev form). */
typedef struct irm_multistart_out {
    int32_t* winner;                     /* B */
    float* cand_alpha;                   /* B·S×N×D */
    float* cand_traj;                    /* B·S×N×D */
    irm_stats* cand_stats;               /* B·S */
    irm_clearance_report* cand_reports;  /* B·S; written with rank_clearance only */
    int32_t* rank;                       /* B·S */
} irm_multistart_out;
/* alpha_out B·S×N×D; waypoints_out B·S×N×D, nullable.  batch = 0 is a no-op. */
int irm_seed_ensemble(irm_ctx* ctx, const float* start, const float* goal, int32_t batch, int32_t n_seeds,
                      uint32_t seed, float amplitude, int32_t problem_offset, float* alpha_out, float* waypoints_out);
int irm_seed_ensemble_dev(irm_ctx* ctx, const float* start_dev, const float* goal_dev, int32_t batch, int32_t n_seeds,
                          uint32_t seed, float amplitude, int32_t problem_offset, float* alpha_dev,
                          float* waypoints_dev, void* stream);
/* stats B·S, reports B·S (nullable); winner_out B, rank_out B·S (nullable). */
int irm_rank_candidates(irm_ctx* ctx, const irm_stats* stats, const irm_clearance_report* reports, int32_t batch,
                        int32_t n_seeds, int32_t* winner_out, int32_t* rank_out);
int irm_rank_candidates_dev(irm_ctx* ctx, const irm_stats* stats_dev, const irm_clearance_report* reports_dev,
                            int32_t batch, int32_t n_seeds, int32_t* winner_dev, int32_t* rank_dev, void* stream);
/* Bytes of device workspace of the _dev call below (every optional table and output counted); negative IRM_E* code
 * on failure. */
int64_t irm_multistart_workspace(const irm_ctx* ctx, int32_t batch, int32_t n_seeds, int32_t n_obstacles,
                                 int32_t obstacle_stride);
/* The arguments of irm_optimize_batch_task behind the descriptor (alpha0 and series_out must be NULL); alpha_out,
 * traj_out, stats_out: the winner's rows (B), each nullable; out->winner B. */
int irm_optimize_multistart(irm_ctx* ctx, const irm_multistart* ms, const float* alpha0, const float* start,
                            const float* goal, const float* obstacles, int32_t n_obstacles, int32_t obstacle_stride,
                            int32_t batch, float* alpha_out, float* traj_out, irm_stats* stats_out, float* series_out,
                            const float* obstacle_velocity, const float* goal_xy, const irm_multistart_out* out);
/* Device pointers, enqueue-only on `stream`: args as irm_optimize_batch_dev takes it (batch = B; alpha0 and
 * series_out 0; goal may be 0 with goal_xy_dev); the two structs are read on the host, during the call. */
int irm_optimize_multistart_dev(irm_ctx* ctx, const irm_multistart* ms, const irm_batch_dev* args,
                                const float* obstacle_velocity_dev, const float* goal_xy_dev,
                                const irm_multistart_out* out, void* workspace_dev, int64_t workspace_bytes,
                                void* stream);

/* Build id of the library: the first 16 hex digits of the SHA-256 over every file of
 * irm_motion_planning_amd/csrc and include/irm.h, the compile flags of every unit and the build
 * variant (build.py source_hash); "unknown" otherwise.
 * __graft_entry__.smoke() compares it with the checked-out sources.  ABI 3. */
const char* irm_build_id(void);

/* Diagnostics: per-workgroup phase cycle counters of the last optimize
 * launch (24 uint64 per workgroup).  Only a library built with
 * -DIRM_PHASE_PROFILE records them; otherwise returns IRM_EINVAL.  Returns
 * the number of workgroups written. */
int irm_debug_phase_profile(irm_ctx* ctx, uint64_t* out, int32_t max_blocks);

/* Diagnostics: line-search log of problem 0 of every later BLS optimize on this
 * context — one record of 10 floats per trial, the values optimizer_BLS.py
 * computes at optimizer_BLS.py:139-149 (trial) and :163-166 (inner-loop head):
 * outer, inner, trial, lr, new_loss, required_loss, accepted, loss, ‖g‖,
 * alpha_norm.  cap records are kept (0 disables).  The record count of a run is
 * that problem's irm_stats.bls_trials (at most cap are stored). */
int irm_debug_bls_trace_enable(irm_ctx* ctx, int32_t cap);
/* Copy up to cap records of the last run's log; returns the number copied. */
int irm_debug_bls_trace(irm_ctx* ctx, float* out, int32_t cap);

#ifdef __cplusplus
}
#endif

#endif /* IRM_H_ */
