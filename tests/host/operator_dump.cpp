// operator_dump — stand-alone driver of the device-free operator build (csrc/irm_operator.cpp) for
// tests/test_operator_host.py.  Built by the test with a plain host compiler from this file and
// irm_operator.cpp only: no HIP, no library.
//
//   operator_dump ops OUT N D RANK SIGMA CVDL
//       builds the operators of one configuration (every other parameter at irm_params_default's
//       value, J = irm_default_jac(D, 0.15, seed 0)) and writes to OUT, as records
//       "<name> <bytes>\n<raw bytes>\n": the parameters it used, every buffer of kOperatorBuffers,
//       t and cvec, the KParams scalars, and R, RP, NK, MP, trunc, lam16, lam24.
//   operator_dump shape N D RP B O TRAJ_PER_BLOCK NUM_CUS
//       prints choose_shape's result for an optimiser launch, without building operators:
//       "TB BT nsplit regops ops_in_lds lds_bytes".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../irm_motion_planning_amd/csrc/irm_operator.hpp"

using irm::KParams;

namespace {

// irm_default_jac (irm_host.cpp) on the operator unit's threefry / erf⁻¹
void default_jac(int D, float jgm, uint32_t seed, float* jac_out) {
    const int n = D * D, odd = n & 1, half = (n + odd) / 2;
    std::vector<uint32_t> bits(2 * half, 0u);
    for (int i = 0; i < half; ++i) {
        uint32_t x0 = (uint32_t)i, x1 = half + i < n ? (uint32_t)(half + i) : 0u;
        irm::threefry2x32(0u, seed, x0, x1);
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
        float z = (float)sqrt(2.0) * (float)irm::erfinv_f64((double)u);
        jac_out[i] = ((i / D) == (i % D) ? 1.f : 0.f) + jgm * z;
    }
}

// irm_params_default (irm_host.cpp), GD, with the configuration of the command line
irm_params make_params(int N, int D, int rank, float sigma, int cvdl) {
    irm_params p;
    memset(&p, 0, sizeof p);
    p.n_timesteps = N;
    p.n_joints = D;
    p.optimizer = IRM_OPT_GD;
    p.max_inner_iteration = 200;
    p.max_outer_iteration = 10;
    p.max_bls_iteration = 20;
    p.constraint_violating_dependant_loss = cvdl;
    const float lr[10] = {2e-3f, 1e-4f, 1e-5f, 1e-6f, 1e-7f, 1e-8f, 1e-8f, 1e-8f, 1e-8f, 1e-8f};
    p.n_gd_lr = 10;
    for (int i = 0; i < 10; ++i) p.gd_lr[i] = lr[i];
    p.rbf_variance = sigma;
    p.loop_loss_reduction = 1e-3f;
    p.lambda_constraint_increase = 10.f;
    p.lambda_sg_constraint = 0.5f;
    p.lambda_jl_constraint = 0.1f;
    p.eps_position = 0.01f;
    p.eps_velocity = 0.01f;
    p.lambda_max_cost = 0.5f;
    p.lambda_reg = 1e-4f;
    p.joint_safety_limit = 0.98f;
    p.bls_lr_start = 0.2f;
    p.bls_alpha = 0.01f;
    p.bls_beta_plus = 1.2f;
    p.bls_beta_minus = 0.5f;
    p.max_joint_velocity = 7.f;
    p.max_joint_position = 2.f;
    p.min_joint_position = -1.f;
    if (D == 3) {
        p.link_length[0] = 1.5f;
        p.link_length[1] = 1.0f;
        p.link_length[2] = 0.5f;
    } else {
        for (int i = 0; i < D; ++i) p.link_length[i] = 0.4f;
    }
    default_jac(D, 0.15f, 0u, p.jac);
    p.operator_rank = rank;
    p.operator_tol = 1e-12f;
    return p;
}

void record(FILE* f, const char* name, const void* data, size_t bytes) {
    fprintf(f, "%s %zu\n", name, bytes);
    fwrite(data, 1, bytes, f);
    fputc('\n', f);
}

int dump_ops(int argc, char** argv) {
    if (argc != 8) return 2;
    const irm_params p = make_params(atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), (float)atof(argv[6]), atoi(argv[7]));
    irm::HostOperators ops;
    if (const char* err = irm::build_operators(p, ops)) {
        fprintf(stderr, "build_operators: %s\n", err);
        return 1;
    }
    KParams kp{};
    if (const char* err = irm::fill_kparams(p, ops, kp)) {
        fprintf(stderr, "fill_kparams: %s\n", err);
        return 1;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 1;
#define P_(m) record(f, "p." #m, &p.m, sizeof p.m)
    P_(lambda_reg); P_(gd_lr); P_(lambda_max_cost); P_(joint_safety_limit); P_(max_joint_velocity);
    P_(max_joint_position); P_(min_joint_position); P_(jac); P_(link_length); P_(max_inner_iteration);
    P_(max_outer_iteration);
#undef P_
    for (const irm::OperatorBuffer& b : irm::kOperatorBuffers) {
        const std::vector<float>& v = ops.*b.host;
        record(f, b.name, v.data(), v.size() * sizeof(float));
    }
    record(f, "t", ops.t.data(), ops.t.size() * sizeof(float));
    record(f, "cvec", ops.cvec.data(), ops.cvec.size() * sizeof(float));
#define O_(m) record(f, #m, &ops.m, sizeof ops.m)
    O_(R); O_(RP); O_(NK); O_(MP); O_(trunc); O_(lam16); O_(lam24);
#undef O_
#define K_(m) record(f, "kp." #m, &kp.m, sizeof kp.m)
    K_(N); K_(D); K_(R); K_(NK); K_(MP); K_(RP); K_(v_ident); K_(O); K_(optimizer); K_(max_inner); K_(max_outer);
    K_(max_bls); K_(cvdl); K_(record_series); K_(max_series); K_(lean_ok); K_(lean_wpl); K_(lean_nohelp); K_(trace_b);
    K_(llr); K_(lci); K_(lsg0); K_(ljl0); K_(eps_p); K_(eps_v); K_(lmax); K_(lreg); K_(bls_lr0); K_(bls_a); K_(bls_bp);
    K_(bls_bm); K_(vmax); K_(pmax); K_(pmin); K_(mean_pos); K_(std_pos); K_(std2); K_(vmax2); K_(thr_hi); K_(thr_lo);
    K_(thr_v); K_(invN); K_(inv_std_pos); K_(inv_vmax); K_(inv_std2); K_(inv_vmax2); K_(Nmagic); K_(NDmagic); K_(gd_lr);
    K_(gd_c); K_(link); K_(J); K_(JtJ); K_(Jinv); K_(Minv); K_(wal); K_(lam_max); K_(one_m_lmax); K_(whole_robot);
    K_(queue_groups);
#undef K_
    return fclose(f) ? 1 : 0;
}

int print_shape(int argc, char** argv) {
    if (argc != 9) return 2;
    const int N = atoi(argv[2]), D = atoi(argv[3]), RP = atoi(argv[4]), B = atoi(argv[5]);
    const int NK = irm::round_up(N, 16), MP = 2 * NK;
    KParams kp{};
    kp.O = atoi(argv[6]);
    int lds = 0;
    const int tb = irm::choose_shape(N, D, NK, RP, MP, atoi(argv[7]), atoi(argv[8]), B, true, kp, &lds);
    printf("%d %d %d %d %d %d\n", tb, kp.BT, kp.nsplit, kp.regops, kp.ops_in_lds, lds);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "ops")) return dump_ops(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "shape")) return print_shape(argc, argv);
    fprintf(stderr, "usage: operator_dump ops OUT N D RANK SIGMA CVDL | shape N D RP B O TRAJ_PER_BLOCK NUM_CUS\n");
    return 2;
}
