// irm_operator.hpp — the device-free part of context creation (irm_operator.cpp): the host linear
// algebra, the kernel matrices, the operator factorisation with its fragment packing, the fp32
// constants of the kernel-parameter block and the workgroup shape.  No HIP header and no hip* symbol:
// it compiles with any C++17 host compiler, so tests/test_operator_host.py checks on a CPU what
// irm_ctx_create (irm_host.cpp) uploads.
#pragma once

#include <stdint.h>

#include <vector>

#include "irm_layout.hpp"

namespace irm {

// ------------------------------------------------------------- host linalg
// fp32 LU (LAPACK's recursive order) and A·X = B, A n×n, B / X n×nrhs, row-major; lu_solve_f32 returns
// false if a pivot is exactly 0.
void getrf2_f32(int m, int n, float* A, int lda, int* ipiv);
bool lu_solve_f32(int n, const float* A_in, const float* B_in, int nrhs, float* X);
// Cyclic Jacobi eigen-decomposition of a symmetric n×n matrix (fp64); the memo keeps the last few.
void jacobi_eigen(std::vector<double>& a_io, int n, std::vector<double>& v_out);
void jacobi_eigen_memo(std::vector<double>& a, int n, std::vector<double>& v);
// legacy threefry and erf⁻¹ (irm_default_jac)
void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1);
double erfinv_f64(double y);

// ------------------------------------------------- kernel-matrix helpers
double decimal_double(float f);
void support_times(int N, float* t);
void kernel_matrices(const float* support, int N, float rbf_variance, const float* eval, int M, float* km, float* dkm);
void fill_frag(std::vector<float>& out, int M, int K, const std::vector<double>& A /*row-major M×K*/, bool kperm = false);
int round_up(int x, int m);

// --------------------------------------------------------------- operators
// Everything build_operators derives from the parameters, on the host: the shapes, the spectrum
// ratios that gate the lean kernel, Trajectory.__init__'s vectors and one fp32 vector per device
// buffer of kOperatorBuffers.
struct HostOperators {
    int R = 0, RP = 0, NK = 0, MP = 0;
    float trunc = 0.f;
    // λ_16/λ_0, λ_24/λ_0 of the operator actually built (0 where the component is not in it): the
    // lean kernel's per-stage rank cuts (direction / residual at rank 16, G at rank 24) are exact to
    // fp32 only while these are at fp32 noise, so they gate it (lean_rank_cut_ok)
    float lam16 = 0.f, lam24 = 0.f;
    std::vector<float> t, cvec, J;
    std::vector<float> K, dK, Kt, dKt, F1, F1p, F2, F2p, Fbot, Vr, VTp, VTs, VNp, VNs, HV, H, u, w;
};

// The operator buffers of a context, once: the name (dumps, diagnostics), the host vector that
// build_operators fills and the KParams pointer that the kernels read it through.  irm_ctx holds one
// device pointer per row; upload, wiring and destroy are loops over this table.
struct OperatorBuffer {
    const char* name;
    std::vector<float> HostOperators::*host;
    const float* KParams::*dev;
};
constexpr OperatorBuffer kOperatorBuffers[] = {
    {"K", &HostOperators::K, &KParams::Km},        {"dK", &HostOperators::dK, &KParams::dKm},
    {"Kt", &HostOperators::Kt, &KParams::Kt},      {"dKt", &HostOperators::dKt, &KParams::dKt},
    {"F1", &HostOperators::F1, &KParams::F1frag},  {"F1p", &HostOperators::F1p, &KParams::F1p},
    {"F2", &HostOperators::F2, &KParams::F2frag},  {"F2p", &HostOperators::F2p, &KParams::F2p},
    {"Fbot", &HostOperators::Fbot, &KParams::Fbot}, {"Vr", &HostOperators::Vr, &KParams::Vr},
    {"VTp", &HostOperators::VTp, &KParams::VTp},   {"VTs", &HostOperators::VTs, &KParams::VTs},
    {"VNp", &HostOperators::VNp, &KParams::VNp},   {"VNs", &HostOperators::VNs, &KParams::VNs},
    {"HV", &HostOperators::HV, &KParams::HV},      {"H", &HostOperators::H, &KParams::Hend},
    {"u", &HostOperators::u, &KParams::uvec},      {"w", &HostOperators::w, &KParams::wvec},
};
constexpr int kNumOperatorBuffers = (int)(sizeof(kOperatorBuffers) / sizeof(kOperatorBuffers[0]));

// Trajectory.__init__ (K, dK, c), the factorisation F = L·V_R, its fragments, Hend / HV / Fbot and
// the initTrajectory basis.  Returns nullptr, or the message of the failure (IRM_EINVAL).
const char* build_operators(const irm_params& p, HostOperators& ops);

// Every scalar and small matrix of the kernel-parameter template (the pointers and num_cus are the
// context's).  Returns nullptr, or the message of the failure (IRM_EINVAL).
const char* fill_kparams(const irm_params& p, const HostOperators& ops, KParams& kp);

// The environment's diagnostics switches IRM_GENERAL_KERNEL, IRM_LEAN_WPL, IRM_LEAN_NOHELP,
// IRM_TRACE_PROBLEM and IRM_WORK_QUEUE, into lean_ok, lean_wpl, lean_nohelp, trace_b, queue_groups.
void read_env_switches(KParams& kp);

// Thresholds of the lean kernel's rank cuts on λ_r/λ_0 (see build_operators): the direction keeps its
// terms to ≤ 1e-6 relative (fp32 rounding of the direction itself is 6e-8), G to σ_24/σ_0 ≤ 1e-7.
constexpr float kLam16Max = 1e-6f, kLam24Max = 1e-14f;
inline bool lean_rank_cut_ok(float lam16, float lam24) { return lam16 <= kLam16Max && lam24 <= kLam24Max; }

// Workgroup shape for a launch of B trajectories; sets the shape fields of kp (N … MP, NW, TB, BT,
// nsplit, regops, ops_in_lds; kp.O and kp.obs_stride are read) and returns TB, 0 if nothing fits.
int choose_shape(int N, int D, int NK, int RP, int MP, int traj_per_block, int num_cus, int B, bool optimizer,
                 KParams& kp, int* lds_bytes_out);

}  // namespace irm
