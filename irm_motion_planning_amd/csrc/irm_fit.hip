// irm_fit.hip — gfx950 kernels that fit and re-time trajectories (irm_fit_alpha, irm_transfer_alpha;
// DESIGN.md §2 "Fitting and re-timing").
//
// Both apply a host-built fp64 operator to source rows X (n_src × D per problem):
//   fit       X[m][k] = Σ_d Q[m][d]·Jinv[d][k]  (fp64 FMA chain over d)     α  = fp32(W·X),  W = (K + ρI)⁻¹
//   transfer  X[m][k] = α_src[m][k]                                          α' = fp32(T·X),  T = W·Kx
// One lane per output waypoint n (chunks of the workgroup's threads where N is larger), kFitP problems per
// workgroup: the source rows of all of them are staged once into LDS as fp64 ([m][problem·D + k], one
// 16-byte-aligned row per m), every lane of a wave reads the same row (broadcast reads), and an operator
// value — consecutive doubles of the transposed operator's row m across the lanes, streamed from L2 and
// prefetched kFitU rows ahead — serves kFitP·D FMAs.  Each output element is one fp64 FMA chain in the
// order m = 0, 1, …, n_src − 1 and is rounded to fp32 once; the chains of different problems never mix, so
// a problem's result does not depend on its batch.  Slots of the last workgroup beyond the batch stage
// zeros and store nothing.
#include "irm_dispatch.hpp"
#include "irm_fit_apply.hpp"  // kFitT, fit_problems, fit_threads, fit_apply, fit_lds
#include "irm_kernels.hpp"

namespace irm {

// Waypoints n = wave·64 + lane, + threads, … of the workgroup's problems b0 … b0 + PB − 1: apply and store.
template <int D, int PB>
__device__ __forceinline__ void fit_outputs(const double* __restrict__ opT, int N, int M, int B, int b0,
                                            const double* __restrict__ X, float* __restrict__ alpha_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int base = wave * 64; base < N; base += blockDim.x) {  // wave-uniform
        const int n = base + lane;
        const bool live = n < N;
        double acc[PB * D];
        fit_apply<PB * D>(opT, (unsigned)N, M, (unsigned)(live ? n : N - 1), X, acc);
        if (!live) continue;
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            if (b0 + p >= B) break;
            float* o = alpha_out + ((size_t)(b0 + p) * N + n) * D;
#pragma unroll
            for (int k = 0; k < D; ++k) o[k] = (float)acc[p * D + k];
        }
    }
}

// α (B×N×D) = fp32(W·(Q·Jinv)): wT is Wᵀ ([m][n]), traj the waypoints Q (B×N×D).
template <int D>
__global__ __launch_bounds__(kFitT) void k_fit_alpha(KParams P, const double* wT, const float* traj, float* alpha_out) {
    extern __shared__ __attribute__((aligned(16))) double fit_smem[];
    constexpr int PB = fit_problems<D>(), C = PB * D;
    const int N = P.N, B = P.B, b0 = blockIdx.x * PB;
    double* X = fit_smem;  // [N][C]
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const bool valid = b0 + p < B;
        const float* q = traj + (size_t)(valid ? b0 + p : 0) * N * D;
        for (int m = threadIdx.x; m < N; m += blockDim.x) {  // one waypoint row per lane
            double qd[D];
#pragma unroll
            for (int d = 0; d < D; ++d) qd[d] = (double)q[m * D + d];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double s = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) s = fma(qd[d], (double)P.Jinv[d * D + k], s);
                X[m * C + p * D + k] = valid ? s : 0.0;
            }
        }
    }
    __syncthreads();
    fit_outputs<D, PB>(wT, N, N, B, b0, X, alpha_out);
}

// α' (B×N×D) = fp32(T·α_src): tT is Tᵀ ([m][n], M × N), alpha_src B×M×D.  start_out (B×D, nullable): the
// source trajectory at t0, fp32(fp32(kq0·α_src)·J) — irm_eval_any's arithmetic for that one time.
template <int D>
__global__ __launch_bounds__(kFitT) void k_transfer_alpha(KParams P, const double* tT, int M, const float* kq0,
                                                          const float* alpha_src, float* alpha_out, float* start_out) {
    extern __shared__ __attribute__((aligned(16))) double fit_smem[];
    constexpr int PB = fit_problems<D>(), C = PB * D;
    const int N = P.N, B = P.B, b0 = blockIdx.x * PB;
    double* X = fit_smem;                // [M][C]
    float* sq = (float*)(X + M * C);     // [C]: fp32(kq0·α_src) per problem and column
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const bool valid = b0 + p < B;
        const float* a = alpha_src + (size_t)(valid ? b0 + p : 0) * M * D;
        for (int r = threadIdx.x; r < M * D; r += blockDim.x) {
            const int m = r / D, k = r - m * D;
            X[m * C + p * D + k] = valid ? (double)a[r] : 0.0;
        }
    }
    __syncthreads();
    fit_outputs<D, PB>(tT, N, M, B, b0, X, alpha_out);
    if (!start_out) return;  // (uniform: a kernel argument)
    const int c = threadIdx.x;
    if (c < C) {  // X holds α_src exactly, so this is the exact fp32×fp32 product chain of eval_any
        double s = 0.0;
        for (int m = 0; m < M; ++m) s = fma((double)kq0[m], X[m * C + c], s);
        sq[c] = (float)s;
    }
    __syncthreads();
    if (c < PB && b0 + c < B) {  // one problem per lane: ·J
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < D; ++d) s = fma((double)sq[c * D + d], (double)P.J[d * D + k], s);
            start_out[(size_t)(b0 + c) * D + k] = (float)s;
        }
    }
}

hipError_t launch_fit_alpha(const KParams& p, const double* wT, const float* traj, float* alpha_out, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        constexpr int PB = fit_problems<DD>();
        return launch_lds(k_fit_alpha<DD>, (p.B + PB - 1) / PB, fit_threads(p.N), fit_lds<DD>(p.N), s, p, wT, traj,
                          alpha_out);
    });
}

hipError_t launch_transfer_alpha(const KParams& p, const double* tT, int n_src, const float* kq0, const float* alpha_src,
                                 float* alpha_out, float* start_out, hipStream_t s) {
    if (p.B <= 0 || n_src <= 0) return hipSuccess;
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        constexpr int PB = fit_problems<DD>();
        return launch_lds(k_transfer_alpha<DD>, (p.B + PB - 1) / PB, fit_threads(p.N), fit_lds<DD>(n_src), s, p, tT,
                          n_src, kq0, alpha_src, alpha_out, start_out);
    });
}

}  // namespace irm
