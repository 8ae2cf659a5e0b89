// irm_host.cpp — C ABI (include/irm.h) of the MI355X trajectory optimiser.
//
// Context creation is a sequence: validate, probe the device, build_operators (irm_operator.cpp:
// everything Trajectory.__init__ builds plus the operators F = L·V_R of the trajectory-space
// formulation, DESIGN.md §2, on the host and without a HIP call), upload the buffers of
// irm::kOperatorBuffers to HBM, fill_kparams, the work-queue counter, the shape probe
// (choose_shape) and the stream.  This file holds the device side of it and the C ABI's calls.
// All per-call numerics run in irm_kernels.hip; there is no CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/irm.h"
#include "irm_kernels.hpp"
#include "irm_operator.hpp"

using irm::KParams;
using irm::erfinv_f64;
using irm::kernel_matrices;
using irm::support_times;
using irm::threefry2x32;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(IRM_EKERNEL, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

}  // namespace

// ================================================================ context
struct irm_ctx {
    irm_params p{};
    int N = 0, D = 0, R = 0, NK = 0, MP = 0, RP = 0;
    float trunc = 0.f;
    // λ_16/λ_0, λ_24/λ_0 of the operator actually built (0 where the component is not in it): the
    // lean kernel's per-stage rank cuts (direction / residual at rank 16, G at rank 24) are exact to
    // fp32 only while these are at fp32 noise, so they gate it (lean_rank_cut_ok)
    float lam16 = 0.f, lam24 = 0.f;
    std::vector<float> t, K, dK, J;
    KParams kp{};
    // device: the operator buffers, one per row of irm::kOperatorBuffers
    float* d_ops[irm::kNumOperatorBuffers] = {};
    // host-API staging
    void* d_io = nullptr;
    size_t io_bytes = 0;
    hipStream_t stream = nullptr;
    int num_cus = 0;
    char name[64] = {0}, arch[32] = {0};
    int tb_opt = 1, ops_lds = 0, lds_opt = 0;
    int max_series = 0;
    unsigned long long* d_prof = nullptr;  // IRM_PHASE_PROFILE builds only
    int prof_blocks = 0, prof_cap = 0;
    float* d_trace = nullptr;  // BLS line-search log of problem 0 (irm_debug_bls_trace)
    int trace_cap = 0;
    int32_t* d_queue = nullptr;  // the work queue's problem counter (kp.queue; the request is kp.queue_groups)
    // evaluation times of irm_eval_any / irm_dense_check (irm_set_eval_times) and their query matrices on
    // the device, transposed ([N][M])
    std::vector<float> t_eval;
    float *d_KqT = nullptr, *d_dKqT = nullptr;
    // moving obstacles: the support times t[n] on the device (kp.tsup, uploaded once at creation) and the
    // evaluation times of irm_dense_check_moving (with the query matrices)
    float *d_t = nullptr, *d_teval = nullptr;
    // fitting and re-timing (irm_fit_alpha, irm_transfer_alpha): the ridge ρ, the Cholesky factor of K + ρI
    // (extended precision, see fit_factor; empty until first use), Wᵀ and Tᵀ on the device in fp64 ([source row][waypoint]) and the source grid's
    // fp32 query row at t0 (xfer_src = 0: no transfer set)
    float fit_ridge = IRM_FIT_RIDGE_DEFAULT;
    std::vector<long double> fit_L;
    double *d_WT = nullptr, *d_TT = nullptr;
    float* d_kq0 = nullptr;
    int xfer_src = 0;
    // multi-start seeds (irm_seed_ensemble): the smooth step c of the operator build, and c (N) then the bump φ (N)
    // on the device (uploaded at first use)
    std::vector<float> cvec;
    float* d_cphi = nullptr;
};

namespace {

int ensure_io(irm_ctx* c, size_t bytes) {
    if (bytes <= c->io_bytes) return 0;
    if (c->d_io) (void)hipFree(c->d_io);
    c->d_io = nullptr;
    c->io_bytes = 0;
    bytes = std::max<size_t>(bytes, 1 << 20);
    HIP_TRY(hipMalloc(&c->d_io, bytes));
    c->io_bytes = bytes;
    return 0;
}

int upload(float** dst, const std::vector<float>& src) {
    HIP_TRY(hipMalloc(dst, std::max<size_t>(src.size(), 4) * sizeof(float)));
    if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// choose_shape for a launch of this context's configuration
int choose_shape(const irm_ctx* c, int B, bool optimizer, KParams& kp, int* lds_bytes_out) {
    return irm::choose_shape(c->N, c->D, c->NK, c->RP, c->MP, c->p.traj_per_block, c->num_cus, B, optimizer, kp,
                             lds_bytes_out);
}

int set_device(const irm_ctx* c) {
    HIP_TRY(hipSetDevice(c->p.device));
    return 0;
}

}  // namespace

extern "C" {

void irm_params_default(irm_params* p) {
    memset(p, 0, sizeof(*p));
    p->n_timesteps = 50;
    p->n_joints = 3;
    p->optimizer = IRM_OPT_BLS;
    p->max_inner_iteration = 200;
    p->max_outer_iteration = 10;
    p->max_bls_iteration = 20;
    p->constraint_violating_dependant_loss = 1;
    const float lr[10] = {2e-3f, 1e-4f, 1e-5f, 1e-6f, 1e-7f, 1e-8f, 1e-8f, 1e-8f, 1e-8f, 1e-8f};
    p->n_gd_lr = 10;
    for (int i = 0; i < 10; ++i) p->gd_lr[i] = lr[i];
    p->rbf_variance = 0.1f;
    p->loop_loss_reduction = 1e-3f;
    p->lambda_constraint_increase = 10.f;
    p->lambda_sg_constraint = 0.5f;
    p->lambda_jl_constraint = 0.1f;
    p->eps_position = 0.01f;
    p->eps_velocity = 0.01f;
    p->lambda_max_cost = 0.5f;
    p->lambda_reg = 1e-4f;
    p->joint_safety_limit = 0.98f;
    p->bls_lr_start = 0.2f;
    p->bls_alpha = 0.01f;
    p->bls_beta_plus = 1.2f;
    p->bls_beta_minus = 0.5f;
    p->max_joint_velocity = 7.f;
    p->max_joint_position = 2.f;
    p->min_joint_position = -1.f;
    p->link_length[0] = 1.5f;
    p->link_length[1] = 1.0f;
    p->link_length[2] = 0.5f;
    irm_default_jac(3, 0.15f, 0u, p->jac);
    p->operator_rank = 0;
    p->operator_tol = 1e-12f;
    p->device = 0;
}

int irm_default_jac(int32_t D, float jgm, uint32_t seed, float* jac_out) {
    if (D < 1 || D > IRM_MAX_JOINTS || !jac_out) return fail(IRM_EINVAL, "irm_default_jac: bad arguments");
    const int n = D * D, odd = n & 1, half = (n + odd) / 2;
    std::vector<uint32_t> cnt(2 * half, 0u), bits(2 * half, 0u);
    for (int i = 0; i < n; ++i) cnt[i] = (uint32_t)i;
    for (int i = 0; i < half; ++i) {
        uint32_t x0 = cnt[i], x1 = cnt[half + i];
        threefry2x32(0u, seed, x0, x1);  // PRNGKey(seed) = [0, seed]
        bits[i] = x0;
        bits[half + i] = x1;
    }
    const float lo = nextafterf(-1.f, 0.f);
    for (int i = 0; i < n; ++i) {
        uint32_t fb = (bits[i] >> 9) | 0x3F800000u;
        float f;
        memcpy(&f, &fb, 4);
        f -= 1.f;
        float u = std::max(lo, f * (1.f - lo) + lo);
        float z = (float)sqrt(2.0) * (float)erfinv_f64((double)u);
        jac_out[i] = ((i / D) == (i % D) ? 1.f : 0.f) + jgm * z;
    }
    return IRM_OK;
}

const char* irm_last_error(void) { return g_err.c_str(); }

int irm_ctx_create(irm_ctx** out, const irm_params* p) {
    if (!out || !p) return fail(IRM_EINVAL, "irm_ctx_create: null argument");
    *out = nullptr;
    const int N = p->n_timesteps, D = p->n_joints;
    if (N < 2 || N > IRM_MAX_TIMESTEPS) return fail(IRM_EINVAL, "n_timesteps=%d outside [2, %d]", N, IRM_MAX_TIMESTEPS);
    if (D < 1 || D > IRM_MAX_JOINTS) return fail(IRM_EINVAL, "n_joints=%d outside [1, %d]", D, IRM_MAX_JOINTS);
    if (p->optimizer != IRM_OPT_GD && p->optimizer != IRM_OPT_BLS) return fail(IRM_EINVAL, "unknown optimizer %d", p->optimizer);
    if (p->optimizer == IRM_OPT_GD && p->max_outer_iteration > p->n_gd_lr)
        return fail(IRM_EINVAL, "max_outer_iteration and dual_lr do not match");  // optimizer_GD.py:34-36
    if (p->n_gd_lr > IRM_MAX_LR) return fail(IRM_EINVAL, "at most %d --gd-lr entries", IRM_MAX_LR);
    if (p->max_bls_iteration < 1 && p->optimizer == IRM_OPT_BLS) return fail(IRM_EINVAL, "max_bls_iteration must be >= 1");
    if (!(p->rbf_variance > 0.f)) return fail(IRM_EINVAL, "rbf_variance must be > 0");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= p->device || p->device < 0)
        return fail(IRM_EDEVICE, "no HIP device %d (found %d): this library has no CPU fallback", p->device, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, p->device));
    if (!strstr(prop.gcnArchName, "gfx950"))
        return fail(IRM_EDEVICE, "device %d is %s; this build targets gfx950 (MI355X) only", p->device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(p->device));

    std::unique_ptr<irm_ctx, void (*)(irm_ctx*)> c(new irm_ctx(), irm_ctx_destroy);  // destroyed on every early return
    c->p = *p;
    c->N = N;
    c->D = D;
    c->num_cus = prop.multiProcessorCount;
    snprintf(c->name, sizeof(c->name), "%s", prop.name);
    snprintf(c->arch, sizeof(c->arch), "%s", prop.gcnArchName);

    irm::HostOperators ops;
    if (const char* err = irm::build_operators(*p, ops)) return fail(IRM_EINVAL, "%s", err);
    c->R = ops.R;
    c->RP = ops.RP;
    c->NK = ops.NK;
    c->MP = ops.MP;
    c->trunc = ops.trunc;
    c->lam16 = ops.lam16;
    c->lam24 = ops.lam24;
    KParams& kp = c->kp;
    for (int i = 0; i < irm::kNumOperatorBuffers; ++i) {
        const irm::OperatorBuffer& b = irm::kOperatorBuffers[i];
        if (upload(&c->d_ops[i], ops.*b.host)) {
            std::string e = g_err;
            return fail(IRM_ENOMEM, "%s", e.c_str());
        }
        kp.*b.dev = c->d_ops[i];
    }
    if (const char* err = irm::fill_kparams(*p, ops, kp)) return fail(IRM_EINVAL, "%s", err);
    c->cvec = std::move(ops.cvec);
    c->t = std::move(ops.t);  // kept for irm_kernel_matrices, the eval times and the fit
    if (upload(&c->d_t, c->t)) {
        std::string e = g_err;
        return fail(IRM_ENOMEM, "%s", e.c_str());
    }
    kp.tsup = c->d_t;
    c->K = std::move(ops.K);
    c->dK = std::move(ops.dK);
    c->J = std::move(ops.J);
    c->max_series = kp.max_series;
    kp.num_cus = c->num_cus;
    if (hipMalloc(&c->d_queue, 256) != hipSuccess) return fail(IRM_ENOMEM, "hipMalloc of the work-queue counter failed");
    kp.queue = c->d_queue;

    {
        KParams probe = c->kp;
        probe.O = IRM_MAX_OBSTACLES;
        c->tb_opt = choose_shape(c.get(), 1 << 20, true, probe, &c->lds_opt);
        c->ops_lds = probe.ops_in_lds;
    }
    if (c->tb_opt <= 0) return fail(IRM_EINVAL, "configuration N=%d D=%d R=%d does not fit the 160 KiB LDS", N, D, c->R);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return fail(IRM_EDEVICE, "hipStreamCreate failed");
    *out = c.release();
    return IRM_OK;
}

void irm_ctx_destroy(irm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->p.device);
    for (float* b : c->d_ops)
        if (b) (void)hipFree(b);
    if (c->d_io) (void)hipFree(c->d_io);
    if (c->d_prof) (void)hipFree(c->d_prof);
    if (c->d_trace) (void)hipFree(c->d_trace);
    if (c->d_queue) (void)hipFree(c->d_queue);
    if (c->d_KqT) (void)hipFree(c->d_KqT);
    if (c->d_dKqT) (void)hipFree(c->d_dKqT);
    if (c->d_t) (void)hipFree(c->d_t);
    if (c->d_teval) (void)hipFree(c->d_teval);
    if (c->d_WT) (void)hipFree(c->d_WT);
    if (c->d_TT) (void)hipFree(c->d_TT);
    if (c->d_kq0) (void)hipFree(c->d_kq0);
    if (c->d_cphi) (void)hipFree(c->d_cphi);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int irm_get_info(const irm_ctx* c, irm_info* out) {
    if (!c || !out) return fail(IRM_EINVAL, "irm_get_info: null argument");
    memset(out, 0, sizeof(*out));
    out->abi_version = IRM_ABI_VERSION;
    out->n_timesteps = c->N;
    out->n_joints = c->D;
    out->operator_rank = c->R;
    out->operator_trunc = c->trunc;
    out->traj_per_block = c->tb_opt;
    out->num_cus = c->num_cus;
    out->lds_bytes_optimize = c->lds_opt;
    snprintf(out->device_name, sizeof(out->device_name), "%s", c->name);
    snprintf(out->arch, sizeof(out->arch), "%s", c->arch);
    snprintf(out->build_id, sizeof(out->build_id), "%s", irm_build_id());
    return IRM_OK;
}

int32_t irm_series_capacity(const irm_ctx* c) { return c ? c->max_series : 0; }

int irm_debug_bls_trace_enable(irm_ctx* c, int32_t cap) {
    if (!c || cap < 0) return fail(IRM_EINVAL, "irm_debug_bls_trace_enable: bad argument");
    if (set_device(c)) return IRM_EDEVICE;
    if (c->d_trace) (void)hipFree(c->d_trace);
    c->d_trace = nullptr;
    c->trace_cap = 0;
    if (cap == 0) return IRM_OK;
    HIP_TRY(hipMalloc(&c->d_trace, (size_t)cap * irm::kTraceW * sizeof(float)));
    HIP_TRY(hipMemset(c->d_trace, 0, (size_t)cap * irm::kTraceW * sizeof(float)));
    c->trace_cap = cap;
    return IRM_OK;
}

int irm_debug_bls_trace(irm_ctx* c, float* out, int32_t cap) {
    if (!c || !out || cap < 0) return fail(IRM_EINVAL, "irm_debug_bls_trace: bad argument");
    if (!c->d_trace) return fail(IRM_EINVAL, "line-search log not enabled (irm_debug_bls_trace_enable)");
    if (set_device(c)) return IRM_EDEVICE;
    const int n = std::min(cap, c->trace_cap);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->d_trace, (size_t)n * irm::kTraceW * sizeof(float), hipMemcpyDeviceToHost));
    return n;
}

int irm_debug_phase_profile(irm_ctx* c, uint64_t* out, int32_t max_blocks) {
    if (!c || !out) return fail(IRM_EINVAL, "null argument");
#if defined(IRM_PHASE_PROFILE) || defined(IRM_DIV_CHECK)
    if (set_device(c)) return IRM_EDEVICE;
    const int n = std::min(max_blocks, c->prof_blocks);
    if (n <= 0 || !c->d_prof) return 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->d_prof, (size_t)n * irm::kProfPhases * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return n;
#else
    (void)max_blocks;
    return fail(IRM_EINVAL, "library built without IRM_PHASE_PROFILE");
#endif
}

int irm_kernel_matrices(const irm_ctx* c, float* t, float* km, float* dkm, float* jac) {
    if (!c) return fail(IRM_EINVAL, "null context");
    if (t) memcpy(t, c->t.data(), sizeof(float) * c->N);
    if (km) memcpy(km, c->K.data(), sizeof(float) * c->K.size());
    if (dkm) memcpy(dkm, c->dK.data(), sizeof(float) * c->dK.size());
    if (jac) memcpy(jac, c->J.data(), sizeof(float) * c->J.size());
    return IRM_OK;
}

// ----------------------------------------------------- host-pointer calls
namespace {

struct Stage {
    irm_ctx* c;
    size_t off = 0;
    char* base() { return (char*)c->d_io; }
    // reserve 256-B aligned slice
    size_t take(size_t bytes) {
        size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

int check_obs(int O) {
    if (O < 0 || O > IRM_MAX_OBSTACLES) return fail(IRM_EINVAL, "n_obstacles=%d outside [0, %d]", O, IRM_MAX_OBSTACLES);
    return 0;
}

// obstacle_stride: 0 = one shared O×2 table, else floats between consecutive problems' tables (≥ 2·O)
int check_stride(int O, int stride) {
    if (stride != 0 && (stride < 2 * O || stride < 0))
        return fail(IRM_EINVAL, "obstacle_stride=%d must be 0 (shared) or >= 2*n_obstacles=%d", stride, 2 * O);
    return 0;
}

// a host velocity table (n floats): every entry finite
int check_vel(const char* fn, const float* vel, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(vel[i])) return fail(IRM_EINVAL, "%s: obstacle_velocity[%zu] is not finite", fn, i);
    return 0;
}

// a host table of end-effector targets (B×2): every entry finite
int check_goal_xy(const char* fn, const float* gxy, size_t B) {
    for (size_t i = 0; i < 2 * B; ++i)
        if (!std::isfinite(gxy[i])) return fail(IRM_EINVAL, "%s: goal_xy[%zu] is not finite", fn, i);
    return 0;
}

// The via table of a call: V, rows, kinds and the target pointer (include/irm.h).  via = NULL or n_via = 0 is
// no via-point (returns 0 with *V = 0).  host: the targets are host memory — every entry that is read is finite.
int check_via(const char* fn, const irm_ctx* c, const irm_via* via, size_t B, bool host, bool need_target, int* V) {
    *V = 0;
    if (!via || via->n_via == 0) return 0;
    const int N = c->N, D = c->D, nv = via->n_via;
    if (nv < 0 || nv > IRM_MAX_VIA) return fail(IRM_EINVAL, "%s: n_via=%d outside [0, %d]", fn, nv, IRM_MAX_VIA);
    for (int v = 0; v < nv; ++v) {
        if (via->row[v] < 1 || via->row[v] > N - 2)
            return fail(IRM_EINVAL, "%s: via row[%d]=%d outside [1, N-2=%d]", fn, v, via->row[v], N - 2);
        if (v && via->row[v] <= via->row[v - 1])
            return fail(IRM_EINVAL, "%s: via rows must be strictly increasing (row[%d]=%d after %d)", fn, v, via->row[v],
                        via->row[v - 1]);
        if (via->cartesian[v] != 0 && via->cartesian[v] != 1)
            return fail(IRM_EINVAL, "%s: via cartesian[%d]=%d (0 joint target, 1 end-effector target)", fn, v,
                        via->cartesian[v]);
        if (via->cartesian[v] && D < 2)
            return fail(IRM_EINVAL, "%s: an end-effector via-point needs D >= 2 (D=%d)", fn, D);
    }
    if (need_target && !via->target) return fail(IRM_EINVAL, "%s: via target is NULL with n_via=%d", fn, nv);
    if (host && via->target) {
        for (size_t b = 0; b < B; ++b)
            for (int v = 0; v < nv; ++v) {
                const int used = via->cartesian[v] ? 2 : D;
                for (int d = 0; d < used; ++d)
                    if (!std::isfinite(via->target[(b * nv + v) * D + d]))
                        return fail(IRM_EINVAL, "%s: via target[%zu][%d][%d] is not finite", fn, b, v, d);
            }
    }
    *V = nv;
    return 0;
}

// the via table into a launch's parameters; target_dev: the targets on the device (B×V×D)
void set_via(KParams& kp, const irm_via* via, int V, const float* target_dev) {
    if (V <= 0) return;
    kp.via = 1;
    kp.n_via = V;
    for (int v = 0; v < V; ++v) {
        kp.via_row[v] = via->row[v];
        kp.via_cart[v] = via->cartesian[v];
    }
    kp.via_target = target_dev;
}

// What a moving, an end-effector-goal and a via call add to the plain one, each nullable: the obstacles'
// velocities (the obstacle table's shape), the end-effector targets (B×2), the via-points and, of
// irm_constraints_via, the via distances out (B×V).
struct Variant {
    const float* vel = nullptr;
    const float* gxy = nullptr;
    const irm_via* via = nullptr;
    float* vdist = nullptr;
};

// A variant into a launch's parameters.  dev: the tables on the device (the callers stage host tables
// themselves), read for a moving / an end-effector-goal launch; its via gives the V rows and kinds, via_target the
// targets on the device (B×V×D).
void set_variant(KParams& kp, bool moving, bool task, const Variant& dev, int V, const float* via_target) {
    if (moving) {
        kp.moving = 1;
        kp.obs_vel = dev.vel;
    }
    if (task) {
        kp.task = 1;
        kp.goal_xy = dev.gxy;
    }
    set_via(kp, dev.via, V, via_target);
}

// a launch for which choose_shape found no trajectories-per-workgroup; fn_moving, fn_via: the entry point a
// moving and a via launch are reported under
int fail_no_shape(const char* fn_moving, const char* fn_via, const irm_ctx* c, const KParams& kp, int O, int stride) {
    if (kp.moving)
        return fail(IRM_EINVAL, "%s: no workgroup shape fits the 160 KiB LDS for N=%d with O=%d %s obstacles and the moving "
                    "table (positions and velocities: twice the obstacle words)", fn_moving, c->N, O, stride ? "per-problem" : "shared");
    if (kp.via) return fail(IRM_EINVAL, "%s: no workgroup shape fits the 160 KiB LDS for N=%d with the via words", fn_via, c->N);
    return fail(IRM_EINVAL, "no workgroup shape fits LDS");
}

// Run one forward-family kernel on B host trajectories (v: host tables; v.vdist with mode 3).
int run_forward(irm_ctx* c, int mode, const float* alpha, const float* start, const float* goal, const float* obs,
                int O, int B, float lsg, float ljl, float lmax, int which, float* out0, float* out1, uint8_t* ok,
                Variant v) {
    if (set_device(c)) return IRM_EDEVICE;
    if (B < 0 || !alpha) return fail(IRM_EINVAL, "bad batch arguments");
    int V = 0;
    if (check_via("irm_eval_cost(_grad)_via / irm_constraints_via", c, v.via, (size_t)std::max(B, 0), true, B > 0, &V))
        return IRM_EINVAL;
    if (check_obs(O)) return IRM_EINVAL;
    if (!obs || O == 0) v.vel = nullptr;  // no obstacle, nothing moves
    if (v.vel && check_vel("irm_eval_cost(_grad)_moving", v.vel, (size_t)O * 2)) return IRM_EINVAL;
    if (v.gxy && check_goal_xy("irm_eval_cost(_grad)_task / irm_constraints_task", v.gxy, (size_t)B)) return IRM_EINVAL;
    if (B == 0) return IRM_OK;
    const int N = c->N, D = c->D;
    const size_t nd = (size_t)B * N * D;
    Stage st{c};
    const size_t o_alpha = st.take(nd * 4), o_s = st.take((size_t)B * D * 4), o_g = st.take((size_t)B * D * 4),
                 o_obs = st.take((size_t)std::max(O, 1) * 8), o_out0 = st.take(std::max(nd, (size_t)B * 11) * 4),
                 o_out1 = st.take(nd * 4), o_ok = st.take((size_t)B), o_vel = st.take((size_t)std::max(O, 1) * 8),
                 o_gxy = st.take((size_t)B * 8), o_via = st.take((size_t)B * std::max(V, 1) * D * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    std::vector<float> zeros;
    if (!start || !goal) zeros.assign((size_t)B * D, 0.f);
    HIP_TRY(hipMemcpyAsync(d + o_alpha, alpha, nd * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_s, start ? start : zeros.data(), (size_t)B * D * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_g, goal ? goal : zeros.data(), (size_t)B * D * 4, hipMemcpyHostToDevice, s));
    if (O > 0 && obs) HIP_TRY(hipMemcpyAsync(d + o_obs, obs, (size_t)O * 8, hipMemcpyHostToDevice, s));
    if (v.vel) HIP_TRY(hipMemcpyAsync(d + o_vel, v.vel, (size_t)O * 8, hipMemcpyHostToDevice, s));
    KParams kp = c->kp;
    kp.B = B;
    kp.O = (obs ? O : 0);
    kp.obs_stride = 0;
    if (v.gxy) HIP_TRY(hipMemcpyAsync(d + o_gxy, v.gxy, (size_t)B * 8, hipMemcpyHostToDevice, s));
    if (V > 0) HIP_TRY(hipMemcpyAsync(d + o_via, v.via->target, (size_t)B * V * D * 4, hipMemcpyHostToDevice, s));
    set_variant(kp, v.vel != nullptr, v.gxy != nullptr, {(const float*)(d + o_vel), (const float*)(d + o_gxy), v.via}, V,
                (const float*)(d + o_via));
    kp.alpha0 = (const float*)(d + o_alpha);
    kp.start = (const float*)(d + o_s);
    kp.goal = (const float*)(d + o_g);
    kp.obstacles = (const float*)(d + o_obs);
    kp.lam_sg = lsg;
    kp.lam_jl = ljl;
    kp.lam_max = lmax;
    kp.one_m_lmax = (float)(1.0 - (double)lmax);
    kp.which = which;
    kp.out0 = (float*)(d + o_out0);
    kp.out1 = (float*)(d + o_out1);
    kp.out_ok = (uint8_t*)(d + o_ok);
    if (choose_shape(c, B, false, kp, nullptr) <= 0)
        return fail_no_shape("irm_eval_cost(_grad)_moving", "irm_eval_cost(_grad)_via", c, kp, O, 0);
    HIP_TRY(irm::launch_forward(kp, mode, s));
    if (out0) {
        size_t bytes = (mode == 0) ? nd * 4 : (mode == 3 ? (size_t)B * 11 * 4 : (size_t)B * 4);
        HIP_TRY(hipMemcpyAsync(out0, d + o_out0, bytes, hipMemcpyDeviceToHost, s));
    }
    if (out1) HIP_TRY(hipMemcpyAsync(out1, d + o_out1, nd * 4, hipMemcpyDeviceToHost, s));
    // (mode 3 of a via call: the kernel wrote the via distances through out1, B×V ≤ B×N×D words)
    if (v.vdist && V > 0) HIP_TRY(hipMemcpyAsync(v.vdist, d + o_out1, (size_t)B * V * 4, hipMemcpyDeviceToHost, s));
    if (ok) HIP_TRY(hipMemcpyAsync(ok, d + o_ok, (size_t)B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

}  // namespace

int irm_evaluate(irm_ctx* c, const float* alpha, int32_t B, int32_t which, float* out) {
    if (!c || !out) return fail(IRM_EINVAL, "irm_evaluate: null argument");
    return run_forward(c, 0, alpha, nullptr, nullptr, nullptr, 0, B, 0.f, 0.f, 0.f, which ? 1 : 0, out, nullptr,
                       nullptr, {});
}

int irm_eval_cost(irm_ctx* c, const float* alpha, const float* start, const float* goal, const float* obstacles,
                  int32_t O, int32_t B, float lsg, float ljl, float lmax, float* cost_out) {
    if (!c || !cost_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost: null argument");
    return run_forward(c, 1, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, nullptr, nullptr, {});
}

int irm_eval_cost_grad(irm_ctx* c, const float* alpha, const float* start, const float* goal, const float* obstacles,
                       int32_t O, int32_t B, float lsg, float ljl, float lmax, float* grad_out, float* cost_out) {
    if (!c || !grad_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost_grad: null argument");
    return run_forward(c, 2, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, grad_out, nullptr, {});
}

int irm_eval_cost_moving(irm_ctx* c, const float* alpha, const float* start, const float* goal, const float* obstacles,
                         int32_t O, int32_t B, float lsg, float ljl, float lmax, float* cost_out,
                         const float* obstacle_velocity) {
    if (!c || !cost_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost_moving: null argument");
    return run_forward(c, 1, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, nullptr, nullptr,
                       {obstacle_velocity});
}

int irm_eval_cost_grad_moving(irm_ctx* c, const float* alpha, const float* start, const float* goal,
                              const float* obstacles, int32_t O, int32_t B, float lsg, float ljl, float lmax,
                              float* grad_out, float* cost_out, const float* obstacle_velocity) {
    if (!c || !grad_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost_grad_moving: null argument");
    return run_forward(c, 2, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, grad_out, nullptr,
                       {obstacle_velocity});
}

int irm_constraints(irm_ctx* c, const float* alpha, const float* start, const float* goal, int32_t B, uint8_t* ok_out,
                    float* report_out) {
    if (!c || !ok_out || !start || !goal) return fail(IRM_EINVAL, "irm_constraints: null argument");
    return run_forward(c, 3, alpha, start, goal, nullptr, 0, B, 0.f, 0.f, 0.f, 0, report_out, nullptr, ok_out, {});
}

int irm_eval_cost_task(irm_ctx* c, const float* alpha, const float* start, const float* goal, const float* obstacles,
                       int32_t O, int32_t B, float lsg, float ljl, float lmax, float* cost_out,
                       const float* obstacle_velocity, const float* goal_xy) {
    if (!c || !cost_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost_task: null argument");
    return run_forward(c, 1, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, nullptr, nullptr,
                       {obstacle_velocity, goal_xy});
}

int irm_eval_cost_grad_task(irm_ctx* c, const float* alpha, const float* start, const float* goal,
                            const float* obstacles, int32_t O, int32_t B, float lsg, float ljl, float lmax,
                            float* grad_out, float* cost_out, const float* obstacle_velocity, const float* goal_xy) {
    if (!c || !grad_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost_grad_task: null argument");
    return run_forward(c, 2, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, grad_out, nullptr,
                       {obstacle_velocity, goal_xy});
}

int irm_constraints_task(irm_ctx* c, const float* alpha, const float* start, const float* goal, int32_t B,
                         uint8_t* ok_out, float* report_out, const float* goal_xy) {
    if (!c || !ok_out || !start || !goal) return fail(IRM_EINVAL, "irm_constraints_task: null argument");
    return run_forward(c, 3, alpha, start, goal, nullptr, 0, B, 0.f, 0.f, 0.f, 0, report_out, nullptr, ok_out,
                       {nullptr, goal_xy});
}

int irm_eval_cost_via(irm_ctx* c, const float* alpha, const float* start, const float* goal, const float* obstacles,
                      int32_t O, int32_t B, float lsg, float ljl, float lmax, float* cost_out,
                      const float* obstacle_velocity, const float* goal_xy, const irm_via* via) {
    if (!c || !cost_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost_via: null argument");
    return run_forward(c, 1, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, nullptr, nullptr,
                       {obstacle_velocity, goal_xy, via});
}

int irm_eval_cost_grad_via(irm_ctx* c, const float* alpha, const float* start, const float* goal,
                           const float* obstacles, int32_t O, int32_t B, float lsg, float ljl, float lmax,
                           float* grad_out, float* cost_out, const float* obstacle_velocity, const float* goal_xy,
                           const irm_via* via) {
    if (!c || !grad_out || !start || !goal) return fail(IRM_EINVAL, "irm_eval_cost_grad_via: null argument");
    return run_forward(c, 2, alpha, start, goal, obstacles, O, B, lsg, ljl, lmax, 0, cost_out, grad_out, nullptr,
                       {obstacle_velocity, goal_xy, via});
}

int irm_constraints_via(irm_ctx* c, const float* alpha, const float* start, const float* goal, int32_t B,
                        uint8_t* ok_out, float* report_out, const float* goal_xy, const irm_via* via,
                        float* via_dist_out) {
    if (!c || !ok_out || !start || !goal) return fail(IRM_EINVAL, "irm_constraints_via: null argument");
    return run_forward(c, 3, alpha, start, goal, nullptr, 0, B, 0.f, 0.f, 0.f, 0, report_out, nullptr, ok_out,
                       {nullptr, goal_xy, via, via_dist_out});
}

int irm_ik_seed_dev(irm_ctx* c, const float* start_dev, const float* goal_xy_dev, int32_t B, float* q_dev,
                    float* residual_dev, void* stream) {
    if (!c || !start_dev || !goal_xy_dev || !q_dev) return fail(IRM_EINVAL, "irm_ik_seed_dev: null argument");
    if (B < 0) return fail(IRM_EINVAL, "irm_ik_seed_dev: negative batch");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    KParams kp = c->kp;
    kp.B = B;
    // the joint range the seed stays in: the safety fraction of the limits (the optimiser's penalty thresholds)
    const float lo = (float)((double)c->p.joint_safety_limit * (double)c->p.min_joint_position);
    const float hi = (float)((double)c->p.joint_safety_limit * (double)c->p.max_joint_position);
    HIP_TRY(irm::launch_ik_seed(kp, start_dev, goal_xy_dev, lo, hi, q_dev, residual_dev, (hipStream_t)stream));
    return IRM_OK;
}

int irm_ik_seed(irm_ctx* c, const float* start, const float* goal_xy, int32_t B, float* q_out, float* residual_out) {
    if (!c || !start || !goal_xy || !q_out) return fail(IRM_EINVAL, "irm_ik_seed: null argument");
    if (B < 0) return fail(IRM_EINVAL, "irm_ik_seed: negative batch");
    if (check_goal_xy("irm_ik_seed", goal_xy, (size_t)B)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int D = c->D;
    Stage st{c};
    const size_t o_s = st.take((size_t)B * D * 4), o_p = st.take((size_t)B * 8), o_q = st.take((size_t)B * D * 4),
                 o_r = st.take((size_t)B * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_s, start, (size_t)B * D * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_p, goal_xy, (size_t)B * 8, hipMemcpyHostToDevice, s));
    const int rc = irm_ik_seed_dev(c, (const float*)(d + o_s), (const float*)(d + o_p), B, (float*)(d + o_q),
                                   (float*)(d + o_r), s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(q_out, d + o_q, (size_t)B * D * 4, hipMemcpyDeviceToHost, s));
    if (residual_out) HIP_TRY(hipMemcpyAsync(residual_out, d + o_r, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

int irm_fk(irm_ctx* c, const float* traj, int32_t B, float* pos_out, float* jac_out) {
    if (!c || !traj || !pos_out) return fail(IRM_EINVAL, "irm_fk: null argument");
    if (set_device(c)) return IRM_EDEVICE;
    if (B <= 0) return B == 0 ? IRM_OK : fail(IRM_EINVAL, "negative batch");
    const int N = c->N, D = c->D;
    const size_t nd = (size_t)B * N * D;
    Stage st{c};
    const size_t o_q = st.take(nd * 4), o_p = st.take((size_t)B * 2 * N * 4), o_j = st.take(2 * nd * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    KParams kp = c->kp;
    kp.B = B;
    HIP_TRY(hipMemcpyAsync(d + o_q, traj, nd * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(irm::launch_fk(kp, (const float*)(d + o_q), (float*)(d + o_p), jac_out ? (float*)(d + o_j) : nullptr,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(pos_out, d + o_p, (size_t)B * 2 * N * 4, hipMemcpyDeviceToHost, c->stream));
    if (jac_out) HIP_TRY(hipMemcpyAsync(jac_out, d + o_j, 2 * nd * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return IRM_OK;
}

int irm_fk_joints(irm_ctx* c, const float* traj, int32_t B, float* pos_out) {
    if (!c || !traj || !pos_out) return fail(IRM_EINVAL, "irm_fk_joints: null argument");
    if (set_device(c)) return IRM_EDEVICE;
    if (B <= 0) return B == 0 ? IRM_OK : fail(IRM_EINVAL, "negative batch");
    const int N = c->N, D = c->D;
    const size_t nd = (size_t)B * N * D;
    Stage st{c};
    const size_t o_q = st.take(nd * 4), o_p = st.take(2 * nd * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    KParams kp = c->kp;
    kp.B = B;
    HIP_TRY(hipMemcpyAsync(d + o_q, traj, nd * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(irm::launch_fk_joints(kp, (const float*)(d + o_q), (float*)(d + o_p), c->stream));
    HIP_TRY(hipMemcpyAsync(pos_out, d + o_p, 2 * nd * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return IRM_OK;
}

int irm_compute_cost_vg(irm_ctx* c, const float* f, const float* obstacles, int32_t O, int32_t B, float* cost_v,
                        float* cost_g) {
    if (!c || !f || !cost_v || (O > 0 && !obstacles)) return fail(IRM_EINVAL, "irm_compute_cost_vg: null argument");
    if (check_obs(O)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B <= 0) return B == 0 ? IRM_OK : fail(IRM_EINVAL, "negative batch");
    const int N = c->N;
    Stage st{c};
    const size_t o_f = st.take((size_t)B * 2 * N * 4), o_o = st.take((size_t)std::max(O, 1) * 8),
                 o_v = st.take((size_t)B * N * 4), o_g = st.take((size_t)B * 2 * N * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    KParams kp = c->kp;
    kp.B = B;
    kp.O = O;
    kp.obstacles = (const float*)(d + o_o);
    HIP_TRY(hipMemcpyAsync(d + o_f, f, (size_t)B * 2 * N * 4, hipMemcpyHostToDevice, c->stream));
    if (O > 0) HIP_TRY(hipMemcpyAsync(d + o_o, obstacles, (size_t)O * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(irm::launch_cost_vg(kp, (const float*)(d + o_f), (float*)(d + o_v), cost_g ? (float*)(d + o_g) : nullptr,
                                c->stream));
    HIP_TRY(hipMemcpyAsync(cost_v, d + o_v, (size_t)B * N * 4, hipMemcpyDeviceToHost, c->stream));
    if (cost_g) HIP_TRY(hipMemcpyAsync(cost_g, d + o_g, (size_t)B * 2 * N * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return IRM_OK;
}

int irm_init_alpha(irm_ctx* c, const float* start, const float* goal, int32_t B, float* alpha_out) {
    if (!c || !start || !goal || !alpha_out) return fail(IRM_EINVAL, "irm_init_alpha: null argument");
    if (set_device(c)) return IRM_EDEVICE;
    if (B <= 0) return B == 0 ? IRM_OK : fail(IRM_EINVAL, "negative batch");
    const int N = c->N, D = c->D;
    const size_t nd = (size_t)B * N * D;
    Stage st{c};
    const size_t o_s = st.take((size_t)B * D * 4), o_g = st.take((size_t)B * D * 4), o_a = st.take(nd * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    KParams kp = c->kp;
    kp.B = B;
    kp.start = (const float*)(d + o_s);
    kp.goal = (const float*)(d + o_g);
    HIP_TRY(hipMemcpyAsync(d + o_s, start, (size_t)B * D * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d + o_g, goal, (size_t)B * D * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(irm::launch_init_alpha(kp, (float*)(d + o_a), c->stream));
    HIP_TRY(hipMemcpyAsync(alpha_out, d + o_a, nd * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return IRM_OK;
}

}  // extern "C"

namespace {

// irm_optimize_batch_dev and its _moving, _task and _via twins (v: device pointers, the via target too)
int optimize_dev(irm_ctx* c, const irm_batch_dev* a, const Variant& v, void* stream) {
    if (!c || !a) return fail(IRM_EINVAL, "irm_optimize_batch_dev: null argument");
    if (a->batch < 0 || !a->start || !a->goal) return fail(IRM_EINVAL, "bad batch arguments");
    int V = 0;
    if (check_via("irm_optimize_batch_via", c, v.via, (size_t)a->batch, false, a->batch > 0, &V)) return IRM_EINVAL;
    if (check_obs(a->n_obstacles) || check_stride(a->n_obstacles, a->obstacle_stride)) return IRM_EINVAL;
    if (a->n_obstacles > 0 && !a->obstacles) return fail(IRM_EINVAL, "obstacles pointer missing");
    if (set_device(c)) return IRM_EDEVICE;
    if (a->batch == 0) return IRM_OK;
    KParams kp = c->kp;
    kp.B = a->batch;
    kp.O = a->n_obstacles;
    kp.obs_stride = a->obstacle_stride;
    kp.alpha0 = a->alpha0;
    kp.start = a->start;
    kp.goal = a->goal;
    kp.obstacles = a->obstacles;
    kp.alpha_out = a->alpha_out;
    kp.traj_out = a->traj_out;
    kp.stats = a->stats_out;
    kp.series = a->series_out;
    kp.trace = c->d_trace;
    kp.trace_cap = c->trace_cap;
    set_variant(kp, v.vel && a->n_obstacles > 0, v.gxy != nullptr, v, V, V > 0 ? v.via->target : nullptr);
    if (choose_shape(c, a->batch, true, kp, nullptr) <= 0)
        return fail_no_shape("irm_optimize_batch_moving", "irm_optimize_batch_via", c, kp, a->n_obstacles, a->obstacle_stride);
#if defined(IRM_PHASE_PROFILE) || defined(IRM_DIV_CHECK)
    {  // (IRM_DIV_CHECK: per-block counters of the BLS division check, zeroed per launch)
        const int grid = (a->batch + kp.TB - 1) / kp.TB;
        if (grid > c->prof_cap) {
            if (c->d_prof) (void)hipFree(c->d_prof);
            c->d_prof = nullptr;
            HIP_TRY(hipMalloc(&c->d_prof, (size_t)grid * irm::kProfPhases * sizeof(unsigned long long)));
            c->prof_cap = grid;
        }
        c->prof_blocks = grid;
        kp.prof = c->d_prof;
#ifdef IRM_DIV_CHECK
        HIP_TRY(hipMemsetAsync(c->d_prof, 0, (size_t)grid * irm::kProfPhases * sizeof(unsigned long long), (hipStream_t)stream));
#endif
    }
#endif
    HIP_TRY(irm::launch_optimize(kp, (hipStream_t)stream));
    return IRM_OK;
}

// irm_optimize_plan and its twins: a moving / an end-effector-goal launch is named without its tables
int optimize_plan(const irm_ctx* c, int32_t batch, int32_t n_obstacles, int32_t record_series, bool moving, bool task,
                  const irm_via* via, irm_launch_plan* out) {
    if (!c || !out || batch <= 0) return fail(IRM_EINVAL, "irm_optimize_plan: bad argument");
    if (check_obs(n_obstacles)) return IRM_EINVAL;
    int V = 0;
    if (check_via("irm_optimize_plan_via", c, via, (size_t)batch, false, false, &V)) return IRM_EINVAL;
    memset(out, 0, sizeof(*out));
    KParams kp = c->kp;
    kp.B = batch;
    kp.O = n_obstacles;
    // the series flow runs when the context records it (irm_params.record_series) or the call asks
    // for the series (irm_optimize_batch with series_out) — as in irm_optimize_batch(_dev)
    kp.record_series = (c->kp.record_series || record_series) ? 1 : 0;
    set_variant(kp, moving && n_obstacles > 0, task, {nullptr, nullptr, via}, V, nullptr);
    if (choose_shape(c, batch, true, kp, nullptr) <= 0)
        return fail_no_shape("irm_optimize_plan_moving", "irm_optimize_plan_via", c, kp, n_obstacles, 0);
    irm::LaunchDesc d{};
    d.describe_only = true;
    HIP_TRY(irm::launch_optimize(kp, nullptr, &d));  // the dispatch fills d and launches nothing
    snprintf(out->kernel, sizeof(out->kernel), "%s", d.kernel);
    out->lean = d.lean;
    out->flow = d.flow;
    out->waypoints_per_lane = d.wpl;
    out->threads = d.threads;
    out->grid = d.grid;
    out->lds_bytes = d.lds_bytes;
    out->traj_per_block = d.traj_per_block;
    out->rank_z = d.rank_z;
    out->rank_dir = d.rank_dir;
    out->rank_g = d.rank_g;
    out->lam16 = c->lam16;
    out->lam24 = c->lam24;
    return IRM_OK;
}

}  // namespace

extern "C" {

int irm_optimize_batch_dev(irm_ctx* c, const irm_batch_dev* a, void* stream) { return optimize_dev(c, a, {}, stream); }

int irm_optimize_batch_moving_dev(irm_ctx* c, const irm_batch_dev* a, const float* obstacle_velocity_dev, void* stream) {
    return optimize_dev(c, a, {obstacle_velocity_dev}, stream);
}

int irm_optimize_plan(const irm_ctx* c, int32_t batch, int32_t n_obstacles, int32_t record_series,
                      irm_launch_plan* out) {
    return optimize_plan(c, batch, n_obstacles, record_series, false, false, nullptr, out);
}

int irm_optimize_plan_moving(const irm_ctx* c, int32_t batch, int32_t n_obstacles, int32_t record_series,
                             irm_launch_plan* out) {
    return optimize_plan(c, batch, n_obstacles, record_series, true, false, nullptr, out);
}

int irm_optimize_batch_task_dev(irm_ctx* c, const irm_batch_dev* a, const float* obstacle_velocity_dev,
                                const float* goal_xy_dev, void* stream) {
    return optimize_dev(c, a, {obstacle_velocity_dev, goal_xy_dev}, stream);
}

int irm_optimize_plan_task(const irm_ctx* c, int32_t batch, int32_t n_obstacles, int32_t record_series,
                           irm_launch_plan* out) {
    return optimize_plan(c, batch, n_obstacles, record_series, false, true, nullptr, out);
}

int irm_optimize_batch_via_dev(irm_ctx* c, const irm_batch_dev* a, const float* obstacle_velocity_dev,
                               const float* goal_xy_dev, void* stream, const irm_via* via) {
    return optimize_dev(c, a, {obstacle_velocity_dev, goal_xy_dev, via}, stream);
}

int irm_optimize_plan_via(const irm_ctx* c, int32_t batch, int32_t n_obstacles, int32_t record_series,
                          irm_launch_plan* out, const irm_via* via) {
    return optimize_plan(c, batch, n_obstacles, record_series, false, true, via, out);
}

int irm_set_work_queue(irm_ctx* c, int32_t groups) {
    if (!c) return fail(IRM_EINVAL, "irm_set_work_queue: null context");
    if (groups < -1) return fail(IRM_EINVAL, "irm_set_work_queue: groups=%d (0 off, > 0 workgroups, -1 auto)", groups);
    c->kp.queue_groups = groups;
    return IRM_OK;
}

int irm_work_queue_groups(const irm_ctx* c, int32_t batch, int32_t n_obstacles, int32_t record_series) {
    if (!c) return fail(IRM_EINVAL, "irm_work_queue_groups: null context");
    if (batch < 0) return fail(IRM_EINVAL, "irm_work_queue_groups: negative batch");
    if (check_obs(n_obstacles)) return IRM_EINVAL;
    if (batch == 0 || c->kp.queue_groups == 0) return 0;
    if (set_device(c)) return IRM_EDEVICE;
    KParams kp = c->kp;
    kp.B = batch;
    kp.O = n_obstacles;
    kp.record_series = (c->kp.record_series || record_series) ? 1 : 0;
    if (choose_shape(c, batch, true, kp, nullptr) <= 0) return fail(IRM_EINVAL, "no workgroup shape fits LDS");
    irm::LaunchDesc d{};
    d.describe_only = true;
    HIP_TRY(irm::launch_optimize(kp, nullptr, &d));  // the dispatch fills d and launches nothing
    return d.queue_groups;
}

// ------------------------------------------- evaluation at arbitrary times
}  // extern "C"

namespace {

int check_eval_times(const char* fn, const float* t_eval, int M) {
    if (!t_eval) return fail(IRM_EINVAL, "%s: null t_eval", fn);
    if (M < 1 || M > IRM_MAX_EVAL_TIMES) return fail(IRM_EINVAL, "%s: M=%d outside [1, %d]", fn, M, IRM_MAX_EVAL_TIMES);
    for (int i = 0; i < M; ++i)
        if (!std::isfinite(t_eval[i])) return fail(IRM_EINVAL, "%s: t_eval[%d] is not finite", fn, i);
    return 0;
}

}  // namespace

extern "C" {

int irm_query_matrices(int32_t N, float rbf_variance, const float* t_eval, int32_t M, float* kq, float* dkq) {
    if (N < 2 || N > IRM_MAX_TIMESTEPS)
        return fail(IRM_EINVAL, "irm_query_matrices: n_timesteps=%d outside [2, %d]", N, IRM_MAX_TIMESTEPS);
    if (!(rbf_variance > 0.f)) return fail(IRM_EINVAL, "irm_query_matrices: rbf_variance must be > 0");
    if (check_eval_times("irm_query_matrices", t_eval, M)) return IRM_EINVAL;
    std::vector<float> t(N);
    support_times(N, t.data());
    kernel_matrices(t.data(), N, rbf_variance, t_eval, M, kq, dkq);
    return IRM_OK;
}

int irm_set_eval_times(irm_ctx* c, const float* t_eval, int32_t M) {
    if (!c) return fail(IRM_EINVAL, "irm_set_eval_times: null context");
    if (check_eval_times("irm_set_eval_times", t_eval, M)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    const int N = c->N;
    std::vector<float> kq((size_t)M * N), dkq((size_t)M * N), kqT((size_t)N * M), dkqT((size_t)N * M);
    kernel_matrices(c->t.data(), N, c->p.rbf_variance, t_eval, M, kq.data(), dkq.data());
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j) {
            kqT[(size_t)j * M + i] = kq[(size_t)i * N + j];
            dkqT[(size_t)j * M + i] = dkq[(size_t)i * N + j];
        }
    // (hipFree waits for the device: no launch that reads the previous grid is left running)
    if (c->d_KqT) (void)hipFree(c->d_KqT);
    if (c->d_dKqT) (void)hipFree(c->d_dKqT);
    c->d_KqT = c->d_dKqT = nullptr;
    c->t_eval.clear();
    if (c->d_teval) (void)hipFree(c->d_teval);
    c->d_teval = nullptr;
    if (upload(&c->d_KqT, kqT) || upload(&c->d_dKqT, dkqT) ||
        upload(&c->d_teval, std::vector<float>(t_eval, t_eval + M)))
        return IRM_ENOMEM;
    c->t_eval.assign(t_eval, t_eval + M);
    return IRM_OK;
}

int32_t irm_eval_times(const irm_ctx* c, float* t_out) {
    if (!c) return fail(IRM_EINVAL, "irm_eval_times: null context");
    if (t_out && !c->t_eval.empty()) memcpy(t_out, c->t_eval.data(), sizeof(float) * c->t_eval.size());
    return (int32_t)c->t_eval.size();
}

int irm_eval_any(irm_ctx* c, const float* alpha, int32_t B, int32_t which, float* out) {
    if (!c || !alpha || !out) return fail(IRM_EINVAL, "irm_eval_any: null argument");
    if (c->t_eval.empty()) return fail(IRM_EINVAL, "irm_eval_any: no evaluation times set (irm_set_eval_times)");
    if (B < 0) return fail(IRM_EINVAL, "irm_eval_any: negative batch");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int N = c->N, D = c->D, M = (int)c->t_eval.size();
    const size_t nd = (size_t)B * N * D, md = (size_t)B * M * D;
    Stage st{c};
    const size_t o_a = st.take(nd * 4), o_o = st.take(md * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    KParams kp = c->kp;
    kp.B = B;
    kp.alpha0 = (const float*)(d + o_a);
    HIP_TRY(hipMemcpyAsync(d + o_a, alpha, nd * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(irm::launch_eval_any(kp, which ? c->d_dKqT : c->d_KqT, M, (float*)(d + o_o), s));
    HIP_TRY(hipMemcpyAsync(out, d + o_o, md * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

}  // extern "C"

namespace {

// the velocity table (a device pointer, nullable) of a launch on the evaluation times, after kp.O is set
void set_moving_eval(KParams& kp, const irm_ctx* c, const float* vel) {
    if (!vel || kp.O <= 0) return;
    kp.moving = 1;  // sample i sees the table at t_eval[i]
    kp.obs_vel = vel;
    kp.tsup = c->d_teval;
}

// irm_dense_check(_moving)_dev: vel a device pointer, NULL for the static check
int dense_check_dev(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O, int32_t obstacle_stride,
                    int32_t B, irm_dense_report* report, float* cost, const float* vel, void* stream) {
    if (!c || !alpha || !report) return fail(IRM_EINVAL, "irm_dense_check_dev: null argument");
    if (c->t_eval.empty()) return fail(IRM_EINVAL, "irm_dense_check_dev: no evaluation times set (irm_set_eval_times)");
    if (B < 0) return fail(IRM_EINVAL, "irm_dense_check_dev: negative batch");
    if (check_obs(O) || check_stride(O, obstacle_stride)) return IRM_EINVAL;
    if (O > 0 && !obstacles) return fail(IRM_EINVAL, "irm_dense_check_dev: obstacles pointer missing");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    KParams kp = c->kp;
    kp.B = B;
    kp.O = O;
    kp.obs_stride = obstacle_stride;
    kp.alpha0 = alpha;
    kp.obstacles = obstacles;
    set_moving_eval(kp, c, vel);
    HIP_TRY(irm::launch_dense_check(kp, c->d_KqT, c->d_dKqT, (int)c->t_eval.size(), report, cost, (hipStream_t)stream));
    return IRM_OK;
}

int dense_check_host(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O, int32_t obstacle_stride,
                     int32_t B, irm_dense_report* report_out, float* cost_out, const float* vel) {
    if (!c || !alpha || !report_out) return fail(IRM_EINVAL, "irm_dense_check: null argument");
    if (c->t_eval.empty()) return fail(IRM_EINVAL, "irm_dense_check: no evaluation times set (irm_set_eval_times)");
    if (B < 0) return fail(IRM_EINVAL, "irm_dense_check: negative batch");
    if (check_obs(O) || check_stride(O, obstacle_stride)) return IRM_EINVAL;
    if (O > 0 && !obstacles) return fail(IRM_EINVAL, "irm_dense_check: obstacles pointer missing");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int N = c->N, D = c->D, M = (int)c->t_eval.size();
    const size_t nd = (size_t)B * N * D;
    const size_t nobs = obstacle_stride ? (size_t)B * obstacle_stride : (size_t)O * 2;
    Stage st{c};
    if (O == 0) vel = nullptr;
    if (vel && check_vel("irm_dense_check_moving", vel, nobs)) return IRM_EINVAL;
    const size_t o_a = st.take(nd * 4), o_o = st.take(std::max<size_t>(nobs, 1) * 4),
                 o_r = st.take((size_t)B * sizeof(irm_dense_report)), o_c = st.take((size_t)B * M * 4),
                 o_w = st.take(std::max<size_t>(nobs, 1) * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_a, alpha, nd * 4, hipMemcpyHostToDevice, s));
    if (nobs && O > 0) HIP_TRY(hipMemcpyAsync(d + o_o, obstacles, nobs * 4, hipMemcpyHostToDevice, s));
    if (vel) HIP_TRY(hipMemcpyAsync(d + o_w, vel, nobs * 4, hipMemcpyHostToDevice, s));
    const int rc = dense_check_dev(c, (const float*)(d + o_a), (const float*)(d + o_o), O, obstacle_stride, B,
                                   (irm_dense_report*)(d + o_r), cost_out ? (float*)(d + o_c) : nullptr,
                                   vel ? (const float*)(d + o_w) : nullptr, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(report_out, d + o_r, (size_t)B * sizeof(irm_dense_report), hipMemcpyDeviceToHost, s));
    if (cost_out) HIP_TRY(hipMemcpyAsync(cost_out, d + o_c, (size_t)B * M * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

}  // namespace

extern "C" {

int irm_dense_check_dev(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O, int32_t obstacle_stride,
                        int32_t B, irm_dense_report* report, float* cost, void* stream) {
    return dense_check_dev(c, alpha, obstacles, O, obstacle_stride, B, report, cost, nullptr, stream);
}

int irm_dense_check(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O, int32_t obstacle_stride,
                    int32_t B, irm_dense_report* report_out, float* cost_out) {
    return dense_check_host(c, alpha, obstacles, O, obstacle_stride, B, report_out, cost_out, nullptr);
}

int irm_dense_check_moving_dev(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O,
                               int32_t obstacle_stride, int32_t B, irm_dense_report* report, float* cost,
                               const float* obstacle_velocity_dev, void* stream) {
    return dense_check_dev(c, alpha, obstacles, O, obstacle_stride, B, report, cost, obstacle_velocity_dev, stream);
}

int irm_dense_check_moving(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O, int32_t obstacle_stride,
                           int32_t B, irm_dense_report* report_out, float* cost_out, const float* obstacle_velocity) {
    return dense_check_host(c, alpha, obstacles, O, obstacle_stride, B, report_out, cost_out, obstacle_velocity);
}

// ------------------------------------------------- clearance of the links against disc obstacles
}  // extern "C"

namespace {

// what irm_clearance and irm_clearance_dev both refuse (fn: the entry point's name)
int clearance_check(const char* fn, const irm_ctx* c, const float* alpha, const float* obstacles, int32_t O,
                    int32_t obstacle_stride, const float* radius, float link_radius, int32_t B, const void* report) {
    if (!c || !alpha || !report) return fail(IRM_EINVAL, "%s: null argument", fn);
    if (c->t_eval.empty()) return fail(IRM_EINVAL, "%s: no evaluation times set (irm_set_eval_times)", fn);
    if (B < 0) return fail(IRM_EINVAL, "%s: negative batch", fn);
    if (O < 0 || O > IRM_MAX_OBSTACLES)
        return fail(IRM_EINVAL, "%s: n_obstacles=%d outside [0, %d]", fn, O, IRM_MAX_OBSTACLES);
    if (obstacle_stride != 0 && (obstacle_stride < 2 * O || obstacle_stride < 0))
        return fail(IRM_EINVAL, "%s: obstacle_stride=%d must be 0 (shared) or >= 2*n_obstacles=%d", fn, obstacle_stride,
                    2 * O);
    if (O > 0 && !obstacles) return fail(IRM_EINVAL, "%s: obstacles pointer missing", fn);
    if (radius && (obstacle_stride & 1))
        return fail(IRM_EINVAL, "%s: obstacle_stride=%d is odd: the radius tables lie obstacle_stride/2 floats apart", fn,
                    obstacle_stride);
    if (!(link_radius >= 0.f) || !std::isfinite(link_radius))
        return fail(IRM_EINVAL, "%s: link_radius must be finite and >= 0", fn);
    return 0;
}

}  // namespace

extern "C" {

int irm_clearance_dev(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O, int32_t obstacle_stride,
                      const float* vel, const float* radius, float link_radius, int32_t B, irm_clearance_report* report,
                      float* clear, float* link, float* joints, void* stream) {
    if (clearance_check("irm_clearance_dev", c, alpha, obstacles, O, obstacle_stride, radius, link_radius, B, report))
        return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    KParams kp = c->kp;
    kp.B = B;
    kp.O = O;
    kp.obs_stride = obstacle_stride;
    kp.alpha0 = alpha;
    kp.obstacles = obstacles;
    set_moving_eval(kp, c, vel);
    HIP_TRY(irm::launch_clearance(kp, c->d_KqT, (int)c->t_eval.size(), O > 0 ? radius : nullptr, obstacle_stride / 2,
                                  link_radius, report, clear, link, joints, (hipStream_t)stream));
    return IRM_OK;
}

int irm_clearance(irm_ctx* c, const float* alpha, const float* obstacles, int32_t O, int32_t obstacle_stride,
                  const float* vel, const float* radius, float link_radius, int32_t B, irm_clearance_report* report_out,
                  float* clear_out, float* link_out, float* joints_out) {
    if (clearance_check("irm_clearance", c, alpha, obstacles, O, obstacle_stride, radius, link_radius, B, report_out))
        return IRM_EINVAL;
    if (O == 0) vel = radius = nullptr;
    const size_t nobs = obstacle_stride ? (size_t)B * obstacle_stride : (size_t)O * 2;
    const size_t nrad = obstacle_stride ? (size_t)B * (obstacle_stride / 2) : (size_t)O;
    if (vel && check_vel("irm_clearance", vel, nobs)) return IRM_EINVAL;
    if (radius)  // (per-problem tables: the floats between a table's O radii and the next table are not read)
        for (size_t b = 0; b < (obstacle_stride ? (size_t)B : 1); ++b)
            for (int o = 0; o < O; ++o) {
                const float r = radius[b * (size_t)(obstacle_stride / 2) + o];
                if (!(r >= 0.f) || !std::isfinite(r))
                    return fail(IRM_EINVAL, "irm_clearance: obstacle_radius[%zu] must be finite and >= 0",
                                b * (size_t)(obstacle_stride / 2) + o);
            }
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int N = c->N, D = c->D, M = (int)c->t_eval.size();
    const size_t nd = (size_t)B * N * D, bm = (size_t)B * M;
    Stage st{c};
    const size_t o_a = st.take(nd * 4), o_o = st.take(std::max<size_t>(nobs, 1) * 4),
                 o_w = st.take(std::max<size_t>(nobs, 1) * 4), o_rad = st.take(std::max<size_t>(nrad, 1) * 4),
                 o_r = st.take((size_t)B * sizeof(irm_clearance_report)), o_c = st.take(bm * 4),
                 o_l = st.take((size_t)B * D * 4), o_j = st.take(joints_out ? bm * D * 2 * 4 : 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_a, alpha, nd * 4, hipMemcpyHostToDevice, s));
    if (nobs && O > 0) HIP_TRY(hipMemcpyAsync(d + o_o, obstacles, nobs * 4, hipMemcpyHostToDevice, s));
    if (vel) HIP_TRY(hipMemcpyAsync(d + o_w, vel, nobs * 4, hipMemcpyHostToDevice, s));
    if (radius) HIP_TRY(hipMemcpyAsync(d + o_rad, radius, nrad * 4, hipMemcpyHostToDevice, s));
    const int rc = irm_clearance_dev(c, (const float*)(d + o_a), (const float*)(d + o_o), O, obstacle_stride,
                                     vel ? (const float*)(d + o_w) : nullptr, radius ? (const float*)(d + o_rad) : nullptr,
                                     link_radius, B, (irm_clearance_report*)(d + o_r), clear_out ? (float*)(d + o_c) : nullptr,
                                     link_out ? (float*)(d + o_l) : nullptr, joints_out ? (float*)(d + o_j) : nullptr, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(report_out, d + o_r, (size_t)B * sizeof(irm_clearance_report), hipMemcpyDeviceToHost, s));
    if (clear_out) HIP_TRY(hipMemcpyAsync(clear_out, d + o_c, bm * 4, hipMemcpyDeviceToHost, s));
    if (link_out) HIP_TRY(hipMemcpyAsync(link_out, d + o_l, (size_t)B * D * 4, hipMemcpyDeviceToHost, s));
    if (joints_out) HIP_TRY(hipMemcpyAsync(joints_out, d + o_j, bm * D * 2 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

// ------------------------------------------------- clearance of the links against each other
}  // extern "C"

namespace {

// what irm_self_clearance and irm_self_clearance_dev both refuse (fn: the entry point's name)
int self_clearance_check(const char* fn, const irm_ctx* c, const float* alpha, float link_radius, int32_t B,
                         const void* report) {
    if (!c) return fail(IRM_EINVAL, "%s: null argument: ctx", fn);
    if (c->t_eval.empty()) return fail(IRM_EINVAL, "%s: no evaluation times set (irm_set_eval_times)", fn);
    if (B < 0) return fail(IRM_EINVAL, "%s: negative batch", fn);
    if (!(link_radius >= 0.f) || !std::isfinite(link_radius))
        return fail(IRM_EINVAL, "%s: link_radius must be finite and >= 0", fn);
    if (B > 0 && !alpha) return fail(IRM_EINVAL, "%s: null argument: alpha", fn);
    if (B > 0 && !report) return fail(IRM_EINVAL, "%s: null argument: report", fn);
    return 0;
}

}  // namespace

extern "C" {

int irm_self_clearance_dev(irm_ctx* c, const float* alpha, float link_radius, int32_t B,
                           irm_self_clearance_report* report, float* clear, float* pair, float* joints, void* stream) {
    if (self_clearance_check("irm_self_clearance_dev", c, alpha, link_radius, B, report)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    KParams kp = c->kp;
    kp.B = B;
    kp.alpha0 = alpha;
    HIP_TRY(irm::launch_self_clearance(kp, c->d_KqT, (int)c->t_eval.size(), link_radius, report, clear, pair, joints,
                                       (hipStream_t)stream));
    return IRM_OK;
}

int irm_self_clearance(irm_ctx* c, const float* alpha, float link_radius, int32_t B,
                       irm_self_clearance_report* report_out, float* clear_out, float* pair_out, float* joints_out) {
    if (self_clearance_check("irm_self_clearance", c, alpha, link_radius, B, report_out)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int N = c->N, D = c->D, M = (int)c->t_eval.size();
    const size_t np = D > 2 ? (size_t)(D - 1) * (D - 2) / 2 : 0;
    const size_t nd = (size_t)B * N * D, bm = (size_t)B * M, bp = (size_t)B * np;
    Stage st{c};
    const size_t o_a = st.take(nd * 4), o_r = st.take((size_t)B * sizeof(irm_self_clearance_report)),
                 o_c = st.take(bm * 4), o_p = st.take(std::max<size_t>(bp, 1) * 4),
                 o_j = st.take(joints_out ? bm * D * 2 * 4 : 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_a, alpha, nd * 4, hipMemcpyHostToDevice, s));
    const int rc = irm_self_clearance_dev(c, (const float*)(d + o_a), link_radius, B,
                                          (irm_self_clearance_report*)(d + o_r), clear_out ? (float*)(d + o_c) : nullptr,
                                          pair_out ? (float*)(d + o_p) : nullptr,
                                          joints_out ? (float*)(d + o_j) : nullptr, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(report_out, d + o_r, (size_t)B * sizeof(irm_self_clearance_report), hipMemcpyDeviceToHost, s));
    if (clear_out) HIP_TRY(hipMemcpyAsync(clear_out, d + o_c, bm * 4, hipMemcpyDeviceToHost, s));
    if (pair_out && bp) HIP_TRY(hipMemcpyAsync(pair_out, d + o_p, bp * 4, hipMemcpyDeviceToHost, s));
    if (joints_out) HIP_TRY(hipMemcpyAsync(joints_out, d + o_j, bm * D * 2 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

// ------------------------------------------------- fitting and re-timing
}  // extern "C"

namespace {

// The factorisation runs in extended precision (x87 long double, 64-bit significand) and its results are
// rounded to fp64 once.  K + ρI has condition ≈ ‖K‖/ρ ≈ 1e8, and an fp64 factorisation leaves W with a forward
// error of 1e-8·‖W‖: a W that is symmetric by construction (L⁻ᵀ·L⁻¹) then misses (K + ρI)·W = I by 150-250
// times what an unsymmetric column-by-column solve leaves, and that solve's W is unsymmetric by 2e-4 to 5e-2
// (N = 50 … 512).  With the factor 2048 of the wider significand both residuals are the final rounding's.
typedef long double fit_real;

// Cholesky factor L (lower triangle, row-major n×n) of K + ρI, from the fp32 entries of K widened.
// K is numerically singular, so ρ is what makes the matrix definite: a non-positive pivot is IRM_EINVAL.
int fit_factor(const char* fn, const float* K, int n, float ridge, std::vector<fit_real>& L) {
    const fit_real rho = (fit_real)ridge;
    L.assign((size_t)n * n, (fit_real)0);
    for (int j = 0; j < n; ++j) {
        const fit_real* lj = &L[(size_t)j * n];
        for (int i = j; i < n; ++i) {
            const fit_real* li = &L[(size_t)i * n];
            fit_real s = (fit_real)K[(size_t)i * n + j] + (i == j ? rho : (fit_real)0);
            for (int k = 0; k < j; ++k) s -= li[k] * lj[k];
            if (i == j) {
                if (!(s > 0))
                    return fail(IRM_EINVAL, "%s: K + rho*I is not positive definite for the ridge rho=%g (pivot %d of %d is %g): "
                                "use a larger ridge (default %g)", fn, (double)rho, j, n, (double)s, (double)IRM_FIT_RIDGE_DEFAULT);
                L[(size_t)j * n + j] = sqrtl(s);
            } else {
                L[(size_t)i * n + j] = s / lj[j];
            }
        }
    }
    return 0;
}

// X ← L⁻¹·X for X n×r row-major (forward substitution on every column at once).
void fit_forward(const std::vector<fit_real>& L, int n, fit_real* X, int r) {
    for (int i = 0; i < n; ++i) {
        fit_real* xi = X + (size_t)i * r;
        for (int k = 0; k < i; ++k) {
            const fit_real l = L[(size_t)i * n + k];
            const fit_real* xk = X + (size_t)k * r;
            for (int j = 0; j < r; ++j) xi[j] -= l * xk[j];
        }
        const fit_real d = L[(size_t)i * n + i];
        for (int j = 0; j < r; ++j) xi[j] /= d;
    }
}

// X ← L⁻ᵀ·X.
void fit_backward(const std::vector<fit_real>& L, int n, fit_real* X, int r) {
    for (int i = n - 1; i >= 0; --i) {
        fit_real* xi = X + (size_t)i * r;
        for (int k = i + 1; k < n; ++k) {
            const fit_real l = L[(size_t)k * n + i];
            const fit_real* xk = X + (size_t)k * r;
            for (int j = 0; j < r; ++j) xi[j] -= l * xk[j];
        }
        const fit_real d = L[(size_t)i * n + i];
        for (int j = 0; j < r; ++j) xi[j] /= d;
    }
}

// W = (K + ρI)⁻¹ = L⁻ᵀ·L⁻¹ (n×n): the lower triangle is summed (k ascending), rounded to fp64 and mirrored,
// so W is symmetric to the bit.
void fit_W(const std::vector<fit_real>& L, int n, std::vector<double>& W) {
    std::vector<fit_real> Li((size_t)n * n, (fit_real)0), S((size_t)n * n, (fit_real)0);
    for (int i = 0; i < n; ++i) {  // L⁻¹ (lower triangular): column j of the identity only reaches rows ≥ j
        fit_real* xi = &Li[(size_t)i * n];
        xi[i] = 1;
        for (int k = 0; k < i; ++k) {
            const fit_real l = L[(size_t)i * n + k];
            const fit_real* xk = &Li[(size_t)k * n];
            for (int j = 0; j <= k; ++j) xi[j] -= l * xk[j];
        }
        const fit_real d = L[(size_t)i * n + i];
        for (int j = 0; j <= i; ++j) xi[j] /= d;
    }
    for (int k = 0; k < n; ++k) {
        const fit_real* lk = &Li[(size_t)k * n];
        for (int i = 0; i <= k; ++i) {
            const fit_real a = lk[i];
            fit_real* si = &S[(size_t)i * n];
            for (int j = 0; j <= i; ++j) si[j] += a * lk[j];
        }
    }
    W.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) W[(size_t)i * n + j] = W[(size_t)j * n + i] = (double)S[(size_t)i * n + j];
}

// T = (K + ρI)⁻¹·Kx (n×n_src) by the two triangular solves, with Kx[i][j] = rbf_kernel(t_src[j], s_i),
// s_i = t0 + (t1 − t0)·t[i] in fp32, in kernel_matrices' fp32 arithmetic.  kq0 (nullable, n_src): Kx's row 0,
// the source grid's query row at s_0 = t0.
void fit_T(const std::vector<fit_real>& L, const float* t, int n, int n_src, float var_src, float t0, float t1,
           std::vector<double>& T, float* kq0) {
    std::vector<float> ts(n_src), s(n), kx((size_t)n * n_src);
    support_times(n_src, ts.data());
    const float dt = t1 - t0;
    for (int i = 0; i < n; ++i) {
        const float step = dt * t[i];
        s[i] = t0 + step;
    }
    kernel_matrices(ts.data(), n_src, var_src, s.data(), n, kx.data(), nullptr);
    if (kq0) memcpy(kq0, kx.data(), sizeof(float) * n_src);
    std::vector<fit_real> X(kx.begin(), kx.end());
    fit_forward(L, n, X.data(), n_src);
    fit_backward(L, n, X.data(), n_src);
    T.resize(X.size());
    for (size_t e = 0; e < T.size(); ++e) T[e] = (double)X[e];
}

int check_ridge(const char* fn, float ridge) {
    if (!std::isfinite(ridge) || !(ridge > 0.f)) return fail(IRM_EINVAL, "%s: the ridge rho=%g must be finite and > 0", fn, (double)ridge);
    return 0;
}

int check_transfer(const char* fn, int n_src, float t0, float t1) {
    if (n_src < 2 || n_src > IRM_MAX_TIMESTEPS) return fail(IRM_EINVAL, "%s: n_src=%d outside [2, %d]", fn, n_src, IRM_MAX_TIMESTEPS);
    if (!std::isfinite(t0) || !std::isfinite(t1)) return fail(IRM_EINVAL, "%s: t0=%g, t1=%g must be finite", fn, (double)t0, (double)t1);
    if (!(t0 < t1)) return fail(IRM_EINVAL, "%s: t0=%g must be < t1=%g", fn, (double)t0, (double)t1);
    return 0;
}

// a (rows × cols, row-major) transposed onto the device (cols × rows).
int upload_transposed(double** dst, const std::vector<double>& a, int rows, int cols) {
    std::vector<double> tr((size_t)rows * cols);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) tr[(size_t)j * rows + i] = a[(size_t)i * cols + j];
    HIP_TRY(hipMalloc(dst, tr.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(*dst, tr.data(), tr.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

// The context's factor and Wᵀ for `ridge`, into L / d_WT (the caller owns them until it commits).
int fit_build(const char* fn, const irm_ctx* c, float ridge, std::vector<fit_real>& L, double** d_WT) {
    if (fit_factor(fn, c->K.data(), c->N, ridge, L)) return IRM_EINVAL;
    std::vector<double> W;
    fit_W(L, c->N, W);
    *d_WT = nullptr;
    if (upload_transposed(d_WT, W, c->N, c->N)) {
        if (*d_WT) (void)hipFree(*d_WT);
        *d_WT = nullptr;
        return IRM_ENOMEM;
    }
    return 0;
}

// W at first use, with the context's ridge.
int ensure_fit(const char* fn, irm_ctx* c) {
    if (c->d_WT) return 0;
    std::vector<fit_real> L;
    double* w = nullptr;
    const int rc = fit_build(fn, c, c->fit_ridge, L, &w);
    if (rc) return rc;
    c->fit_L.swap(L);
    c->d_WT = w;
    return 0;
}

void drop_transfer(irm_ctx* c) {
    // (hipFree waits for the device: no launch that reads the previous operator is left running)
    if (c->d_TT) (void)hipFree(c->d_TT);
    if (c->d_kq0) (void)hipFree(c->d_kq0);
    c->d_TT = nullptr;
    c->d_kq0 = nullptr;
    c->xfer_src = 0;
}

}  // namespace

extern "C" {

int irm_fit_operator(int32_t n, float rbf_variance, float ridge, int32_t n_src, float rbf_variance_src, float t0,
                     float t1, double* out) {
    if (n < 2 || n > IRM_MAX_TIMESTEPS) return fail(IRM_EINVAL, "irm_fit_operator: n=%d outside [2, %d]", n, IRM_MAX_TIMESTEPS);
    if (!(rbf_variance > 0.f)) return fail(IRM_EINVAL, "irm_fit_operator: rbf_variance must be > 0");
    if (!out) return fail(IRM_EINVAL, "irm_fit_operator: null output");
    if (check_ridge("irm_fit_operator", ridge)) return IRM_EINVAL;
    if (n_src != 0 && check_transfer("irm_fit_operator", n_src, t0, t1)) return IRM_EINVAL;
    std::vector<float> t(n), K((size_t)n * n);
    support_times(n, t.data());
    kernel_matrices(t.data(), n, rbf_variance, t.data(), n, K.data(), nullptr);
    std::vector<fit_real> L;
    std::vector<double> A;
    if (fit_factor("irm_fit_operator", K.data(), n, ridge, L)) return IRM_EINVAL;
    if (n_src == 0) fit_W(L, n, A);
    else fit_T(L, t.data(), n, n_src, rbf_variance_src > 0.f ? rbf_variance_src : rbf_variance, t0, t1, A, nullptr);
    memcpy(out, A.data(), A.size() * sizeof(double));
    return IRM_OK;
}

int irm_set_fit_ridge(irm_ctx* c, float ridge) {
    if (!c) return fail(IRM_EINVAL, "irm_set_fit_ridge: null context");
    if (check_ridge("irm_set_fit_ridge", ridge)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    std::vector<fit_real> L;
    double* w = nullptr;
    const int rc = fit_build("irm_set_fit_ridge", c, ridge, L, &w);
    if (rc) return rc;  // the previous ridge, W and transfer stay
    drop_transfer(c);
    if (c->d_WT) (void)hipFree(c->d_WT);
    c->d_WT = w;
    c->fit_L.swap(L);
    c->fit_ridge = ridge;
    return IRM_OK;
}

int irm_set_transfer(irm_ctx* c, int32_t n_src, float rbf_variance_src, float t0, float t1) {
    if (!c) return fail(IRM_EINVAL, "irm_set_transfer: null context");
    if (check_transfer("irm_set_transfer", n_src, t0, t1)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    const int rc = ensure_fit("irm_set_transfer", c);
    if (rc) return rc;
    std::vector<double> T;
    std::vector<float> kq0(n_src);
    fit_T(c->fit_L, c->t.data(), c->N, n_src, rbf_variance_src > 0.f ? rbf_variance_src : c->p.rbf_variance, t0, t1, T,
          kq0.data());
    drop_transfer(c);
    if (upload_transposed(&c->d_TT, T, c->N, n_src) || upload(&c->d_kq0, kq0)) {
        drop_transfer(c);
        return IRM_ENOMEM;
    }
    c->xfer_src = n_src;
    return IRM_OK;
}

int irm_fit_alpha_dev(irm_ctx* c, const float* traj, int32_t B, float* alpha, void* stream) {
    if (!c || !traj || !alpha) return fail(IRM_EINVAL, "irm_fit_alpha_dev: null argument");
    if (B < 0) return fail(IRM_EINVAL, "irm_fit_alpha_dev: negative batch");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int rc = ensure_fit("irm_fit_alpha_dev", c);
    if (rc) return rc;
    KParams kp = c->kp;
    kp.B = B;
    HIP_TRY(irm::launch_fit_alpha(kp, c->d_WT, traj, alpha, (hipStream_t)stream));
    return IRM_OK;
}

int irm_transfer_alpha_dev(irm_ctx* c, const float* alpha_src, int32_t B, float* alpha, float* start, void* stream) {
    if (!c || !alpha_src || !alpha) return fail(IRM_EINVAL, "irm_transfer_alpha_dev: null argument");
    if (c->xfer_src == 0) return fail(IRM_EINVAL, "irm_transfer_alpha_dev: no transfer set (irm_set_transfer)");
    if (B < 0) return fail(IRM_EINVAL, "irm_transfer_alpha_dev: negative batch");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    KParams kp = c->kp;
    kp.B = B;
    HIP_TRY(irm::launch_transfer_alpha(kp, c->d_TT, c->xfer_src, c->d_kq0, alpha_src, alpha, start, (hipStream_t)stream));
    return IRM_OK;
}

int irm_fit_alpha(irm_ctx* c, const float* traj, int32_t B, float* alpha_out) {
    if (!c || !traj || !alpha_out) return fail(IRM_EINVAL, "irm_fit_alpha: null argument");
    if (B < 0) return fail(IRM_EINVAL, "irm_fit_alpha: negative batch");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const size_t nd = (size_t)B * c->N * c->D;
    Stage st{c};
    const size_t o_q = st.take(nd * 4), o_a = st.take(nd * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_q, traj, nd * 4, hipMemcpyHostToDevice, s));
    const int rc = irm_fit_alpha_dev(c, (const float*)(d + o_q), B, (float*)(d + o_a), s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(alpha_out, d + o_a, nd * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

int irm_transfer_alpha(irm_ctx* c, const float* alpha_src, int32_t B, float* alpha_out, float* start_out) {
    if (!c || !alpha_src || !alpha_out) return fail(IRM_EINVAL, "irm_transfer_alpha: null argument");
    if (c->xfer_src == 0) return fail(IRM_EINVAL, "irm_transfer_alpha: no transfer set (irm_set_transfer)");
    if (B < 0) return fail(IRM_EINVAL, "irm_transfer_alpha: negative batch");
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const size_t ns = (size_t)B * c->xfer_src * c->D, nd = (size_t)B * c->N * c->D, sd = (size_t)B * c->D;
    Stage st{c};
    const size_t o_s = st.take(ns * 4), o_a = st.take(nd * 4), o_q = st.take(sd * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_s, alpha_src, ns * 4, hipMemcpyHostToDevice, s));
    const int rc = irm_transfer_alpha_dev(c, (const float*)(d + o_s), B, (float*)(d + o_a),
                                          start_out ? (float*)(d + o_q) : nullptr, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(alpha_out, d + o_a, nd * 4, hipMemcpyDeviceToHost, s));
    if (start_out) HIP_TRY(hipMemcpyAsync(start_out, d + o_q, sd * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

const char* irm_build_id(void) {
#ifdef IRM_SOURCE_HASH
    return IRM_SOURCE_HASH;
#else
    return "unknown";
#endif
}

}  // extern "C"

namespace {

int optimize_host(irm_ctx* c, const float* alpha0, const float* start, const float* goal, const float* obstacles,
                  int32_t O, int32_t obstacle_stride, int32_t B, float* alpha_out, float* traj_out,
                  irm_stats* stats_out, float* series_out, Variant v) {
    if (!c || !start || !goal) return fail(IRM_EINVAL, "irm_optimize_batch: null argument");
    if (check_obs(O) || check_stride(O, obstacle_stride)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    int V = 0;
    if (check_via("irm_optimize_batch_via", c, v.via, (size_t)std::max(B, 0), true, B > 0, &V)) return IRM_EINVAL;
    if (B <= 0) return B == 0 ? IRM_OK : fail(IRM_EINVAL, "negative batch");
    const int N = c->N, D = c->D;
    const size_t nd = (size_t)B * N * D;
    const size_t nobs = obstacle_stride ? (size_t)B * obstacle_stride : (size_t)O * 2;
    const size_t nser = series_out ? (size_t)B * c->max_series * N * D : 0;
    if (!obstacles || O == 0) v.vel = nullptr;
    if (v.vel && check_vel("irm_optimize_batch_moving", v.vel, nobs)) return IRM_EINVAL;
    if (v.gxy && check_goal_xy("irm_optimize_batch_task", v.gxy, (size_t)B)) return IRM_EINVAL;
    Stage st{c};
    const size_t o_a0 = st.take(nd * 4), o_s = st.take((size_t)B * D * 4), o_g = st.take((size_t)B * D * 4),
                 o_o = st.take(std::max<size_t>(nobs, 1) * 4), o_ao = st.take(nd * 4), o_to = st.take(nd * 4),
                 o_st = st.take((size_t)B * sizeof(irm_stats)), o_se = st.take(std::max<size_t>(nser, 1) * 4),
                 o_w = st.take(std::max<size_t>(nobs, 1) * 4), o_p = st.take((size_t)B * 8),
                 o_via = st.take((size_t)B * std::max(V, 1) * D * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    if (v.gxy) HIP_TRY(hipMemcpyAsync(d + o_p, v.gxy, (size_t)B * 8, hipMemcpyHostToDevice, s));
    irm_via vdev{};
    if (V > 0) {
        HIP_TRY(hipMemcpyAsync(d + o_via, v.via->target, (size_t)B * V * D * 4, hipMemcpyHostToDevice, s));
        vdev = *v.via;
        vdev.target = (const float*)(d + o_via);
    }
    if (alpha0) HIP_TRY(hipMemcpyAsync(d + o_a0, alpha0, nd * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_s, start, (size_t)B * D * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_g, goal, (size_t)B * D * 4, hipMemcpyHostToDevice, s));
    if (nobs && obstacles) HIP_TRY(hipMemcpyAsync(d + o_o, obstacles, nobs * 4, hipMemcpyHostToDevice, s));
    if (v.vel) HIP_TRY(hipMemcpyAsync(d + o_w, v.vel, nobs * 4, hipMemcpyHostToDevice, s));
    irm_batch_dev a{};
    a.alpha0 = alpha0 ? (const float*)(d + o_a0) : nullptr;
    a.start = (const float*)(d + o_s);
    a.goal = (const float*)(d + o_g);
    a.obstacles = (const float*)(d + o_o);
    a.n_obstacles = O;
    a.obstacle_stride = obstacle_stride;
    a.batch = B;
    a.alpha_out = (float*)(d + o_ao);
    a.traj_out = (float*)(d + o_to);
    a.stats_out = (irm_stats*)(d + o_st);
    a.series_out = series_out ? (float*)(d + o_se) : nullptr;
    KParams save = c->kp;
    if (series_out) c->kp.record_series = 1;
    int rc = optimize_dev(c, &a, {v.vel ? (const float*)(d + o_w) : nullptr, v.gxy ? (const float*)(d + o_p) : nullptr,
                                  V > 0 ? &vdev : nullptr}, s);
    c->kp = save;
    if (rc) return rc;
    if (alpha_out) HIP_TRY(hipMemcpyAsync(alpha_out, d + o_ao, nd * 4, hipMemcpyDeviceToHost, s));
    if (traj_out) HIP_TRY(hipMemcpyAsync(traj_out, d + o_to, nd * 4, hipMemcpyDeviceToHost, s));
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d + o_st, (size_t)B * sizeof(irm_stats), hipMemcpyDeviceToHost, s));
    if (series_out) HIP_TRY(hipMemcpyAsync(series_out, d + o_se, nser * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

}  // namespace

extern "C" {

int irm_optimize_batch(irm_ctx* c, const float* alpha0, const float* start, const float* goal, const float* obstacles,
                       int32_t O, int32_t obstacle_stride, int32_t B, float* alpha_out, float* traj_out,
                       irm_stats* stats_out, float* series_out) {
    return optimize_host(c, alpha0, start, goal, obstacles, O, obstacle_stride, B, alpha_out, traj_out, stats_out,
                         series_out, {});
}

int irm_optimize_batch_moving(irm_ctx* c, const float* alpha0, const float* start, const float* goal,
                              const float* obstacles, int32_t O, int32_t obstacle_stride, int32_t B, float* alpha_out,
                              float* traj_out, irm_stats* stats_out, float* series_out,
                              const float* obstacle_velocity) {
    return optimize_host(c, alpha0, start, goal, obstacles, O, obstacle_stride, B, alpha_out, traj_out, stats_out,
                         series_out, {obstacle_velocity});
}

int irm_optimize_batch_task(irm_ctx* c, const float* alpha0, const float* start, const float* goal,
                            const float* obstacles, int32_t O, int32_t obstacle_stride, int32_t B, float* alpha_out,
                            float* traj_out, irm_stats* stats_out, float* series_out, const float* obstacle_velocity,
                            const float* goal_xy) {
    return optimize_host(c, alpha0, start, goal, obstacles, O, obstacle_stride, B, alpha_out, traj_out, stats_out,
                         series_out, {obstacle_velocity, goal_xy});
}

int irm_optimize_batch_via(irm_ctx* c, const float* alpha0, const float* start, const float* goal,
                           const float* obstacles, int32_t O, int32_t obstacle_stride, int32_t B, float* alpha_out,
                           float* traj_out, irm_stats* stats_out, float* series_out, const float* obstacle_velocity,
                           const float* goal_xy, const irm_via* via) {
    return optimize_host(c, alpha0, start, goal, obstacles, O, obstacle_stride, B, alpha_out, traj_out, stats_out,
                         series_out, {obstacle_velocity, goal_xy, via});
}

}  // extern "C"

// ------------------------------------------------- multi-start planning
namespace {

// c (N) then φ (N) on the device, at first use: φ_n = 16·(p·p), p = t_n·(1 − t_n) in fp32
int ensure_seed_tables(irm_ctx* c) {
    if (c->d_cphi) return 0;
    const int N = c->N;
    std::vector<float> cphi(2 * (size_t)N);
    for (int n = 0; n < N; ++n) {
        const float t = c->t[n];
        const float om = 1.f - t;
        const float p = t * om;
        const float pp = p * p;
        cphi[n] = c->cvec[n];
        cphi[(size_t)N + n] = 16.f * pp;
    }
    if (upload(&c->d_cphi, cphi)) {
        if (c->d_cphi) (void)hipFree(c->d_cphi);
        c->d_cphi = nullptr;
        return IRM_ENOMEM;
    }
    return 0;
}

// what every seed / multi-start entry point refuses about the ensemble itself
int check_ensemble(const char* fn, int32_t B, int32_t S, float amplitude, int32_t problem_offset) {
    if (B < 0) return fail(IRM_EINVAL, "%s: negative batch", fn);
    if (S < 1 || S > IRM_MAX_SEEDS) return fail(IRM_EINVAL, "%s: n_seeds=%d outside [1, %d]", fn, S, IRM_MAX_SEEDS);
    if (!(amplitude >= 0.f) || !std::isfinite(amplitude))
        return fail(IRM_EINVAL, "%s: amplitude=%g must be finite and >= 0", fn, (double)amplitude);
    if (problem_offset < 0) return fail(IRM_EINVAL, "%s: problem_offset=%d must be >= 0", fn, problem_offset);
    if ((int64_t)B * S > (int64_t)1 << 24) return fail(IRM_EINVAL, "%s: batch*n_seeds=%lld candidates exceed 2^24", fn, (long long)B * S);
    return 0;
}

size_t al256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// The device workspace of irm_optimize_multistart_dev: offsets of its slices (every optional one reserved).
struct MsLayout {
    size_t seeds, start, goal, ik, gxy, obs, vel, rad, c_alpha, c_traj, c_stats, c_rep, rank, total;
};

MsLayout ms_layout(const irm_ctx* c, size_t B, size_t S, size_t stride) {
    const size_t BS = B * S, nd = (size_t)c->N * c->D, D = (size_t)c->D;
    MsLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += al256(std::max<size_t>(bytes, 4));
        return o;
    };
    l.seeds = take(BS * nd * 4);
    l.start = take(BS * D * 4);
    l.goal = take(BS * D * 4);
    l.ik = take(B * D * 4);
    l.gxy = take(BS * 8);
    l.obs = take(BS * stride * 4);
    l.vel = take(BS * stride * 4);
    l.rad = take(BS * (stride / 2) * 4);
    l.c_alpha = take(BS * nd * 4);
    l.c_traj = take(BS * nd * 4);
    l.c_stats = take(BS * sizeof(irm_stats));
    l.c_rep = take(BS * sizeof(irm_clearance_report));
    l.rank = take(BS * 4);
    l.total = off;
    return l;
}

// what irm_optimize_multistart and its _dev form both refuse (the host form before it stages anything)
int check_multistart(const char* fn, const irm_ctx* c, const irm_multistart* ms, int32_t B, int32_t O, int32_t stride,
                     const void* alpha0, const void* series_out, const void* start, const void* goal,
                     const void* obstacles, const void* goal_xy, const irm_multistart_out* out) {
    if (!c || !ms || !out || !out->winner || !start) return fail(IRM_EINVAL, "%s: null argument", fn);
    if (check_ensemble(fn, B, ms->n_seeds, ms->amplitude, ms->problem_offset)) return IRM_EINVAL;
    if (alpha0) return fail(IRM_EINVAL, "%s: alpha0 must be NULL (the seeds are the call's own)", fn);
    if (series_out || c->kp.record_series)
        return fail(IRM_EINVAL, "%s: series_out / record_series: a multi-start call records no series", fn);
    if (!goal && !goal_xy) return fail(IRM_EINVAL, "%s: goal is NULL without goal_xy", fn);
    if (check_obs(O) || check_stride(O, stride)) return IRM_EINVAL;
    if (O > 0 && !obstacles) return fail(IRM_EINVAL, "%s: obstacles pointer missing", fn);
    if (ms->rank_clearance && c->t_eval.empty())
        return fail(IRM_EINVAL, "%s: rank_clearance needs an evaluation grid (irm_set_eval_times)", fn);
    if (!ms->rank_clearance && ms->obstacle_radius)
        return fail(IRM_EINVAL, "%s: obstacle_radius without rank_clearance", fn);
    if (!ms->rank_clearance && ms->link_radius != 0.f)
        return fail(IRM_EINVAL, "%s: link_radius=%g without rank_clearance", fn, (double)ms->link_radius);
    if (ms->rank_clearance && (!(ms->link_radius >= 0.f) || !std::isfinite(ms->link_radius)))
        return fail(IRM_EINVAL, "%s: link_radius must be finite and >= 0", fn);
    if (ms->rank_clearance && ms->obstacle_radius && (stride & 1))
        return fail(IRM_EINVAL, "%s: obstacle_stride=%d is odd: the radius tables lie obstacle_stride/2 floats apart", fn, stride);
    return 0;
}

}  // namespace

extern "C" {

int irm_seed_ensemble_dev(irm_ctx* c, const float* start, const float* goal, int32_t B, int32_t S, uint32_t seed,
                          float amplitude, int32_t problem_offset, float* alpha, float* waypoints, void* stream) {
    if (!c || !start || !goal || !alpha) return fail(IRM_EINVAL, "irm_seed_ensemble_dev: null argument");
    if (check_ensemble("irm_seed_ensemble_dev", B, S, amplitude, problem_offset)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    int rc = ensure_fit("irm_seed_ensemble_dev", c);
    if (rc) return rc;
    if ((rc = ensure_seed_tables(c))) return rc;
    KParams kp = c->kp;
    kp.B = B;
    // the joint range of the clamp: irm_ik_seed's
    const float lo = (float)((double)c->p.joint_safety_limit * (double)c->p.min_joint_position);
    const float hi = (float)((double)c->p.joint_safety_limit * (double)c->p.max_joint_position);
    HIP_TRY(irm::launch_seed_ensemble(kp, c->d_WT, c->d_cphi, start, goal, S, seed, amplitude, (uint32_t)problem_offset,
                                      lo, hi, alpha, waypoints, (hipStream_t)stream));
    return IRM_OK;
}

int irm_seed_ensemble(irm_ctx* c, const float* start, const float* goal, int32_t B, int32_t S, uint32_t seed,
                      float amplitude, int32_t problem_offset, float* alpha_out, float* waypoints_out) {
    if (!c || !start || !goal || !alpha_out) return fail(IRM_EINVAL, "irm_seed_ensemble: null argument");
    if (check_ensemble("irm_seed_ensemble", B, S, amplitude, problem_offset)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const size_t sd = (size_t)B * c->D, nd = (size_t)B * S * c->N * c->D;
    Stage st{c};
    const size_t o_s = st.take(sd * 4), o_g = st.take(sd * 4), o_a = st.take(nd * 4), o_w = st.take(nd * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_s, start, sd * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_g, goal, sd * 4, hipMemcpyHostToDevice, s));
    const int rc = irm_seed_ensemble_dev(c, (const float*)(d + o_s), (const float*)(d + o_g), B, S, seed, amplitude,
                                         problem_offset, (float*)(d + o_a), waypoints_out ? (float*)(d + o_w) : nullptr, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(alpha_out, d + o_a, nd * 4, hipMemcpyDeviceToHost, s));
    if (waypoints_out) HIP_TRY(hipMemcpyAsync(waypoints_out, d + o_w, nd * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

int irm_rank_candidates_dev(irm_ctx* c, const irm_stats* stats, const irm_clearance_report* reports, int32_t B,
                            int32_t S, int32_t* winner, int32_t* rank, void* stream) {
    if (!c || !stats || !winner) return fail(IRM_EINVAL, "irm_rank_candidates_dev: null argument");
    if (check_ensemble("irm_rank_candidates_dev", B, S, 0.f, 0)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    HIP_TRY(irm::launch_rank_candidates(stats, reports, B, S, winner, rank, (hipStream_t)stream));
    return IRM_OK;
}

int irm_rank_candidates(irm_ctx* c, const irm_stats* stats, const irm_clearance_report* reports, int32_t B, int32_t S,
                        int32_t* winner_out, int32_t* rank_out) {
    if (!c || !stats || !winner_out) return fail(IRM_EINVAL, "irm_rank_candidates: null argument");
    if (check_ensemble("irm_rank_candidates", B, S, 0.f, 0)) return IRM_EINVAL;
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const size_t BS = (size_t)B * S;
    Stage st{c};
    const size_t o_st = st.take(BS * sizeof(irm_stats)), o_rp = st.take(BS * sizeof(irm_clearance_report)),
                 o_w = st.take((size_t)B * 4), o_r = st.take(BS * 4);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_st, stats, BS * sizeof(irm_stats), hipMemcpyHostToDevice, s));
    if (reports) HIP_TRY(hipMemcpyAsync(d + o_rp, reports, BS * sizeof(irm_clearance_report), hipMemcpyHostToDevice, s));
    const int rc = irm_rank_candidates_dev(c, (const irm_stats*)(d + o_st),
                                           reports ? (const irm_clearance_report*)(d + o_rp) : nullptr, B, S,
                                           (int32_t*)(d + o_w), rank_out ? (int32_t*)(d + o_r) : nullptr, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(winner_out, d + o_w, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    if (rank_out) HIP_TRY(hipMemcpyAsync(rank_out, d + o_r, BS * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

int64_t irm_multistart_workspace(const irm_ctx* c, int32_t B, int32_t S, int32_t O, int32_t obstacle_stride) {
    if (!c) return fail(IRM_EINVAL, "irm_multistart_workspace: null context");
    if (check_ensemble("irm_multistart_workspace", B, S, 0.f, 0)) return IRM_EINVAL;
    if (check_obs(O) || check_stride(O, obstacle_stride)) return IRM_EINVAL;
    return (int64_t)ms_layout(c, (size_t)B, (size_t)S, (size_t)obstacle_stride).total;
}

int irm_optimize_multistart_dev(irm_ctx* c, const irm_multistart* ms, const irm_batch_dev* a, const float* vel,
                                const float* gxy, const irm_multistart_out* out, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    const char* fn = "irm_optimize_multistart_dev";
    if (!a) return fail(IRM_EINVAL, "%s: null argument", fn);
    if (check_multistart(fn, c, ms, a->batch, a->n_obstacles, a->obstacle_stride, a->alpha0, a->series_out, a->start,
                         a->goal, a->obstacles, gxy, out))
        return IRM_EINVAL;
    const int B = a->batch, S = ms->n_seeds, O = a->n_obstacles, stride = a->obstacle_stride;
    const MsLayout l = ms_layout(c, (size_t)B, (size_t)S, (size_t)stride);
    if (B > 0 && (!workspace || workspace_bytes < (int64_t)l.total))
        return fail(IRM_EINVAL, "%s: workspace of %lld bytes, irm_multistart_workspace asks for %lld", fn,
                    (long long)(workspace ? workspace_bytes : 0), (long long)l.total);
    if (B > 0 && ((uintptr_t)workspace & 255)) return fail(IRM_EINVAL, "%s: workspace is not 256-byte aligned", fn);
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int D = c->D, nd = c->N * c->D, BS = B * S;
    char* w = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    float* seeds = (float*)(w + l.seeds);
    float* start_r = (float*)(w + l.start);
    float* goal_r = (float*)(w + l.goal);
    if (O == 0) vel = nullptr;  // no obstacle, nothing moves
    // the goal configuration: given, or the IK seed's for (start, goal_xy)
    const float* goal = a->goal;
    if (!goal) {
        const int rc = irm_ik_seed_dev(c, a->start, gxy, B, (float*)(w + l.ik), nullptr, s);
        if (rc) return rc;
        goal = (const float*)(w + l.ik);
    }
    int rc = irm_seed_ensemble_dev(c, a->start, goal, B, S, ms->seed, ms->amplitude, ms->problem_offset, seeds, nullptr, s);
    if (rc) return rc;
    HIP_TRY(irm::launch_replicate(a->start, start_r, B, S, D, D, s));
    HIP_TRY(irm::launch_replicate(goal, goal_r, B, S, D, D, s));
    const float* gxy_r = nullptr;
    if (gxy) {
        HIP_TRY(irm::launch_replicate(gxy, (float*)(w + l.gxy), B, S, 2, 2, s));
        gxy_r = (const float*)(w + l.gxy);
    }
    // shared tables (obstacle_stride 0) serve the B·S problems as they are; per-problem ones are replicated
    const float *obs_r = a->obstacles, *vel_r = vel, *rad_r = ms->rank_clearance && O > 0 ? ms->obstacle_radius : nullptr;
    if (stride && O > 0) {
        HIP_TRY(irm::launch_replicate(a->obstacles, (float*)(w + l.obs), B, S, stride, stride, s));
        obs_r = (const float*)(w + l.obs);
        if (vel) {
            HIP_TRY(irm::launch_replicate(vel, (float*)(w + l.vel), B, S, stride, stride, s));
            vel_r = (const float*)(w + l.vel);
        }
        if (rad_r) {
            HIP_TRY(irm::launch_replicate(rad_r, (float*)(w + l.rad), B, S, stride / 2, stride / 2, s));
            rad_r = (const float*)(w + l.rad);
        }
    }
    float* c_alpha = out->cand_alpha ? out->cand_alpha : (float*)(w + l.c_alpha);
    float* c_traj = out->cand_traj ? out->cand_traj : (a->traj_out ? (float*)(w + l.c_traj) : nullptr);
    irm_stats* c_stats = out->cand_stats ? out->cand_stats : (irm_stats*)(w + l.c_stats);
    irm_clearance_report* c_rep = out->cand_reports ? out->cand_reports : (irm_clearance_report*)(w + l.c_rep);
    irm_batch_dev in{};
    in.alpha0 = seeds;
    in.start = start_r;
    in.goal = goal_r;
    in.obstacles = obs_r;
    in.n_obstacles = O;
    in.obstacle_stride = stride;
    in.batch = BS;
    in.alpha_out = c_alpha;
    in.traj_out = c_traj;
    in.stats_out = c_stats;
    if ((rc = optimize_dev(c, &in, {vel_r, gxy_r}, stream))) return rc;
    if (ms->rank_clearance) {
        rc = irm_clearance_dev(c, c_alpha, obs_r, O, stride, vel_r, rad_r, ms->link_radius, BS, c_rep, nullptr, nullptr,
                               nullptr, stream);
        if (rc) return rc;
    }
    HIP_TRY(irm::launch_rank_candidates(c_stats, ms->rank_clearance ? c_rep : nullptr, B, S, out->winner, out->rank, s));
    HIP_TRY(irm::launch_gather_winner(out->winner, B, S, nd, c_alpha, c_traj, c_stats, a->alpha_out, a->traj_out,
                                      a->stats_out, s));
    return IRM_OK;
}

int irm_optimize_multistart(irm_ctx* c, const irm_multistart* ms, const float* alpha0, const float* start,
                            const float* goal, const float* obstacles, int32_t O, int32_t obstacle_stride, int32_t B,
                            float* alpha_out, float* traj_out, irm_stats* stats_out, float* series_out,
                            const float* vel, const float* gxy, const irm_multistart_out* out) {
    const char* fn = "irm_optimize_multistart";
    if (check_multistart(fn, c, ms, B, O, obstacle_stride, alpha0, series_out, start, goal, obstacles, gxy, out))
        return IRM_EINVAL;
    const size_t nobs = obstacle_stride ? (size_t)B * obstacle_stride : (size_t)O * 2;
    const size_t nrad = obstacle_stride ? (size_t)B * (obstacle_stride / 2) : (size_t)O;
    if (O == 0) vel = nullptr;
    const float* radius = ms->rank_clearance && O > 0 ? ms->obstacle_radius : nullptr;
    if (vel && check_vel(fn, vel, nobs)) return IRM_EINVAL;
    if (gxy && check_goal_xy(fn, gxy, (size_t)B)) return IRM_EINVAL;
    if (radius)
        for (size_t b = 0; b < (obstacle_stride ? (size_t)B : 1); ++b)
            for (int o = 0; o < O; ++o) {
                const float r = radius[b * (size_t)(obstacle_stride / 2) + o];
                if (!(r >= 0.f) || !std::isfinite(r))
                    return fail(IRM_EINVAL, "%s: obstacle_radius[%zu] must be finite and >= 0", fn,
                                b * (size_t)(obstacle_stride / 2) + o);
            }
    if (set_device(c)) return IRM_EDEVICE;
    if (B == 0) return IRM_OK;
    const int S = ms->n_seeds;
    const size_t BS = (size_t)B * S, sd = (size_t)B * c->D, nd1 = (size_t)c->N * c->D;
    const MsLayout l = ms_layout(c, (size_t)B, (size_t)S, (size_t)obstacle_stride);
    Stage st{c};
    const size_t o_s = st.take(sd * 4), o_g = st.take(sd * 4), o_o = st.take(std::max<size_t>(nobs, 1) * 4),
                 o_v = st.take(std::max<size_t>(nobs, 1) * 4), o_p = st.take((size_t)B * 8),
                 o_rad = st.take(std::max<size_t>(nrad, 1) * 4), o_ao = st.take(B * nd1 * 4), o_to = st.take(B * nd1 * 4),
                 o_st = st.take((size_t)B * sizeof(irm_stats)), o_win = st.take((size_t)B * 4), o_ws = st.take(l.total);
    if (ensure_io(c, st.off)) return IRM_ENOMEM;
    char* d = st.base();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d + o_s, start, sd * 4, hipMemcpyHostToDevice, s));
    if (goal) HIP_TRY(hipMemcpyAsync(d + o_g, goal, sd * 4, hipMemcpyHostToDevice, s));
    if (nobs && O > 0) HIP_TRY(hipMemcpyAsync(d + o_o, obstacles, nobs * 4, hipMemcpyHostToDevice, s));
    if (vel) HIP_TRY(hipMemcpyAsync(d + o_v, vel, nobs * 4, hipMemcpyHostToDevice, s));
    if (gxy) HIP_TRY(hipMemcpyAsync(d + o_p, gxy, (size_t)B * 8, hipMemcpyHostToDevice, s));
    if (radius) HIP_TRY(hipMemcpyAsync(d + o_rad, radius, nrad * 4, hipMemcpyHostToDevice, s));
    irm_multistart msd = *ms;
    msd.obstacle_radius = radius ? (const float*)(d + o_rad) : nullptr;
    irm_batch_dev a{};
    a.start = (const float*)(d + o_s);
    a.goal = goal ? (const float*)(d + o_g) : nullptr;
    a.obstacles = (const float*)(d + o_o);
    a.n_obstacles = O;
    a.obstacle_stride = obstacle_stride;
    a.batch = B;
    a.alpha_out = (float*)(d + o_ao);
    a.traj_out = (float*)(d + o_to);
    a.stats_out = (irm_stats*)(d + o_st);
    // the candidates' rows stay in the workspace (its own slices) and are copied out from there
    char* w = d + o_ws;
    irm_multistart_out od{};
    od.winner = (int32_t*)(d + o_win);
    od.cand_traj = out->cand_traj ? (float*)(w + l.c_traj) : nullptr;
    od.rank = out->rank ? (int32_t*)(w + l.rank) : nullptr;
    const int rc = irm_optimize_multistart_dev(c, &msd, &a, vel ? (const float*)(d + o_v) : nullptr,
                                               gxy ? (const float*)(d + o_p) : nullptr, &od, w, (int64_t)l.total, s);
    if (rc) return rc;
    if (alpha_out) HIP_TRY(hipMemcpyAsync(alpha_out, d + o_ao, B * nd1 * 4, hipMemcpyDeviceToHost, s));
    if (traj_out) HIP_TRY(hipMemcpyAsync(traj_out, d + o_to, B * nd1 * 4, hipMemcpyDeviceToHost, s));
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d + o_st, (size_t)B * sizeof(irm_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out->winner, d + o_win, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    if (out->cand_alpha) HIP_TRY(hipMemcpyAsync(out->cand_alpha, w + l.c_alpha, BS * nd1 * 4, hipMemcpyDeviceToHost, s));
    if (out->cand_traj) HIP_TRY(hipMemcpyAsync(out->cand_traj, w + l.c_traj, BS * nd1 * 4, hipMemcpyDeviceToHost, s));
    if (out->cand_stats)
        HIP_TRY(hipMemcpyAsync(out->cand_stats, w + l.c_stats, BS * sizeof(irm_stats), hipMemcpyDeviceToHost, s));
    if (out->cand_reports && ms->rank_clearance)
        HIP_TRY(hipMemcpyAsync(out->cand_reports, w + l.c_rep, BS * sizeof(irm_clearance_report), hipMemcpyDeviceToHost, s));
    if (out->rank) HIP_TRY(hipMemcpyAsync(out->rank, w + l.rank, BS * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IRM_OK;
}

}  // extern "C"
