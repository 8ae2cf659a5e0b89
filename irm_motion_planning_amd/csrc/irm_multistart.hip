// irm_multistart.hip — gfx950 kernels of multi-start planning (irm_seed_ensemble, irm_rank_candidates,
// irm_optimize_multistart; include/irm.h states the contract, this file follows it operation for operation).
//
// Candidates are rows, problem-major: candidate s of problem b is row b·S + s.
//   k_seed_ensemble    the S seeds of every problem: waypoints formed in the staging loop (the smooth-step line
//                      plus a hashed smooth bump, clamped), then fit_alpha's FMA chain on them (irm_fit_apply.hpp,
//                      the workgroup shape of k_fit_alpha: fit_problems rows per workgroup, one lane per waypoint);
//                      candidate 0 is k_init_alpha's expression instead
//   k_replicate        per-problem rows of w floats, S times each (start, goal, goal_xy, obstacle / velocity /
//                      radius tables)
//   k_rank_candidates  one wave per problem, one lane per candidate: the position of the lane's key
//                      (class, loss, s) among the problem's keys, by counting the smaller ones
//   k_gather_winner    the winner's α, trajectory and stats rows into the B-sized outputs
#include <algorithm>

#include "irm_dispatch.hpp"
#include "irm_fit_apply.hpp"  // kFitT, fit_problems, fit_threads, fit_apply, fit_lds
#include "irm_kernels.hpp"

namespace irm {

// MurmurHash3's finaliser
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

struct SeedArgs {
    const double* wT;    // Wᵀ of the fit ([m][n], N×N fp64)
    const float* cphi;   // c (N: the smooth step) then φ (N: the bump)
    const float* start;  // B×D
    const float* goal;   // B×D
    int32_t S;
    uint32_t seed, problem_offset;
    float amplitude, lo, hi;
    float* alpha;  // B·S×N×D
    float* way;    // B·S×N×D, nullable
};

template <int D>
__global__ __launch_bounds__(kFitT) void k_seed_ensemble(KParams P, SeedArgs A) {
    extern __shared__ __attribute__((aligned(16))) double fit_smem[];
    constexpr int PB = fit_problems<D>(), C = PB * D;
    const int N = P.N, S = A.S, R = P.B * S, r0 = blockIdx.x * PB;
    double* X = fit_smem;  // [N][C]
    const float twoA = 2.f * A.amplitude;
    const uint32_t h0 = fmix32(A.seed ^ 0x243F6A88u);
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        const int r = r0 + p;
        const bool valid = r < R;
        const int b = valid ? r / S : 0, s = valid ? r - b * S : 0;
        float sd[D], gd[D], amp[D];
        const uint32_t hs = fmix32(fmix32(h0 + (A.problem_offset + (uint32_t)b)) + (uint32_t)s);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            sd[d] = A.start[(size_t)b * D + d];
            gd[d] = A.goal[(size_t)b * D + d] - sd[d];
            const float u = (float)(fmix32(hs + (uint32_t)d) >> 8) * 0x1p-24f;
            amp[d] = fmaf(twoA, u, -A.amplitude);
        }
        for (int m = threadIdx.x; m < N; m += blockDim.x) {  // one waypoint row per lane
            const float cm = A.cphi[m], ph = A.cphi[N + m];
            double qd[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                float q = fmaf(cm, gd[d], sd[d]);
                if (s > 0) q = fminf(fmaxf(fmaf(ph, amp[d], q), A.lo), A.hi);
                if (A.way && valid) A.way[((size_t)r * N + m) * D + d] = q;
                qd[d] = (double)q;
            }
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double acc = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) acc = fma(qd[d], (double)P.Jinv[d * D + k], acc);
                X[m * C + p * D + k] = valid ? acc : 0.0;
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int base = wave * 64; base < N; base += blockDim.x) {  // wave-uniform
        const int n = base + lane;
        const bool live = n < N;
        double acc[C];
        if (S > 1) fit_apply<C>(A.wT, (unsigned)N, N, (unsigned)(live ? n : N - 1), X, acc);  // (S = 1: candidate 0 only)
        if (!live) continue;
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            const int r = r0 + p;
            if (r >= R) break;
            const int b = r / S, s = r - b * S;
            float* o = A.alpha + ((size_t)r * N + n) * D;
            if (s > 0) {
#pragma unroll
                for (int k = 0; k < D; ++k) o[k] = (float)acc[p * D + k];
            } else {  // k_init_alpha's expression: α0 = u⊗(s·J⁻¹) + w⊗(g·J⁻¹)
                const float un = P.uvec[n], wn = P.wvec[n];
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    float sj = 0.f, gj = 0.f;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        sj += A.start[(size_t)b * D + d] * P.Jinv[d * D + k];
                        gj += A.goal[(size_t)b * D + d] * P.Jinv[d * D + k];
                    }
                    o[k] = un * sj + wn * gj;
                }
            }
        }
    }
}

// out[(b·S + s)·w + j] = in[b·in_stride + j]
__global__ __launch_bounds__(256) void k_replicate(const float* __restrict__ in, float* __restrict__ out, int B, int S,
                                                   int w, int in_stride) {
    const size_t total = (size_t)B * S * w;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / (unsigned)w;
        const int j = (int)(e - r * (unsigned)w);
        const size_t b = r / (unsigned)S;
        out[e] = in[b * (size_t)in_stride + j];
    }
}

constexpr int kRankT = 256;  // four problems per workgroup, one wave each

__global__ __launch_bounds__(kRankT) void k_rank_candidates(const irm_stats* __restrict__ st,
                                                            const irm_clearance_report* __restrict__ rep, int B, int S,
                                                            int32_t* __restrict__ winner, int32_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * (kRankT / 64) + wave;
    if (b >= B) return;  // wave-uniform
    const bool live = lane < S;
    int cls = 0x7fffffff;
    float loss = INFINITY;
    if (live) {
        const size_t r = (size_t)b * S + lane;
        loss = st[r].final_loss;
        cls = 2 * (st[r].constraints_ok ? 0 : 1) + ((rep && rep[r].n_colliding > 0) ? 1 : 0);
        if (loss != loss) {  // NaN: behind every class, compared as +inf
            cls = 4;
            loss = INFINITY;
        }
    }
    int before = 0;
    for (int j = 0; j < S; ++j) {  // (uniform trip count: every lane takes part in the shuffles)
        const int cj = __shfl(cls, j);
        const float lj = __shfl(loss, j);
        const bool less = cj < cls || (cj == cls && (lj < loss || (lj == loss && j < lane)));
        before += less ? 1 : 0;
    }
    if (!live) return;
    if (rank) rank[(size_t)b * S + lane] = before;
    if (before == 0) winner[b] = lane;
}

// row b·S + winner[b] of the candidates' α, trajectories (nd floats each) and stats into row b of the outputs
__global__ __launch_bounds__(256) void k_gather_winner(const int32_t* __restrict__ winner, int S, int nd,
                                                       const float* __restrict__ cand_alpha,
                                                       const float* __restrict__ cand_traj,
                                                       const irm_stats* __restrict__ cand_stats,
                                                       float* __restrict__ alpha, float* __restrict__ traj,
                                                       irm_stats* __restrict__ stats) {
    const int b = blockIdx.x;
    const int w = min(max(winner[b], 0), S - 1);
    const size_t src = ((size_t)b * S + w) * nd, dst = (size_t)b * nd;
    for (int e = threadIdx.x; e < nd; e += blockDim.x) {
        if (alpha) alpha[dst + e] = cand_alpha[src + e];
        if (traj) traj[dst + e] = cand_traj[src + e];
    }
    constexpr int kWords = (int)(sizeof(irm_stats) / sizeof(int32_t));
    if (stats && threadIdx.x < kWords)
        reinterpret_cast<int32_t*>(stats + b)[threadIdx.x] =
            reinterpret_cast<const int32_t*>(cand_stats + (size_t)b * S + w)[threadIdx.x];
}

hipError_t launch_seed_ensemble(const KParams& p, const double* wT, const float* cphi, const float* start,
                                const float* goal, int S, uint32_t seed, float amplitude, uint32_t problem_offset,
                                float lo, float hi, float* alpha_out, float* way_out, hipStream_t s) {
    if (p.B <= 0 || S <= 0) return hipSuccess;
    const SeedArgs a = {wT, cphi, start, goal, S, seed, problem_offset, amplitude, lo, hi, alpha_out, way_out};
    return dispatch_d(p.D, [&](auto dc) {
        constexpr int DD = decltype(dc)::value;
        constexpr int PB = fit_problems<DD>();
        return launch_lds(k_seed_ensemble<DD>, (p.B * S + PB - 1) / PB, fit_threads(p.N), fit_lds<DD>(p.N), s, p, a);
    });
}

hipError_t launch_replicate(const float* in, float* out, int B, int S, int w, int in_stride, hipStream_t s) {
    const size_t total = (size_t)std::max(B, 0) * std::max(S, 0) * std::max(w, 0);
    if (total == 0) return hipSuccess;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 65535);
    hipLaunchKernelGGL(k_replicate, dim3(grid), dim3(256), 0, s, in, out, B, S, w, in_stride);
    return hipGetLastError();
}

hipError_t launch_rank_candidates(const irm_stats* stats, const irm_clearance_report* rep, int B, int S,
                                  int32_t* winner, int32_t* rank, hipStream_t s) {
    if (B <= 0 || S <= 0) return hipSuccess;
    constexpr int per = kRankT / 64;
    hipLaunchKernelGGL(k_rank_candidates, dim3((B + per - 1) / per), dim3(kRankT), 0, s, stats, rep, B, S, winner, rank);
    return hipGetLastError();
}

hipError_t launch_gather_winner(const int32_t* winner, int B, int S, int nd, const float* cand_alpha,
                                const float* cand_traj, const irm_stats* cand_stats, float* alpha, float* traj,
                                irm_stats* stats, hipStream_t s) {
    if (B <= 0 || S <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_winner, dim3(B), dim3(256), 0, s, winner, S, nd, cand_alpha, cand_traj, cand_stats,
                       alpha, traj, stats);
    return hipGetLastError();
}

}  // namespace irm
