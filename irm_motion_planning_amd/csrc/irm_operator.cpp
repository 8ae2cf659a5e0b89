// irm_operator.cpp — the device-free operator build behind irm_ctx_create (irm_host.cpp).
//
// build_operators builds, once per configuration, everything
// Trajectory.__init__ builds (trajectory.py:23-42) plus the host images of the device-side
// operators of the trajectory-space formulation:
//   L = [K; dK]                (2N × N, fp32 exactly as the reference)
//   F = L·V_R                  (V_R: top-R eigenvectors of LᵀL, fp64 Jacobi)
// packed into the 16x16x4 MFMA A-fragment layouts; fill_kparams derives the fp32 constants of the
// kernel-parameter block and choose_shape the workgroup shape.  Nothing here touches the GPU: the
// unit includes no HIP header and builds with any C++17 compiler (with -ffp-contract=off: the
// roundings below are the reference's only without contraction).
#include "irm_operator.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

namespace irm {

/* A hyper-parameter the reference holds as a Python double (argparse) reaches this library as a
   float: recover the double the decimal argument denotes — the shortest decimal that round-trips the
   float (0.1f → "0.1" → 0.1) — so derived constants such as fp32(2·σ²) round as the reference's do
   (trajectory.py:14-19: 2*rbf_var**2 is a double, weakly typed to fp32 in the division). */
double decimal_double(float f) {
    char buf[32];
    for (int prec = 6; prec <= 9; ++prec) {
        snprintf(buf, sizeof buf, "%.*g", prec, (double)f);
        if (strtof(buf, nullptr) == f) return strtod(buf, nullptr);
    }
    return (double)f;
}

// ------------------------------------------------------------- host linalg
// Cyclic Jacobi eigen-decomposition of a symmetric n×n matrix (fp64).
// On return a's diagonal holds the eigenvalues and v the eigenvectors (columns).
// The rotations work on copies with a padded row stride (a power-of-two stride put every element of a
// column rotation into one cache set) and accumulate the eigenvectors as rows (vᵀ: each rotation updates
// two contiguous rows): the same operations in the same order as the plain n-stride form, so the result
// is bit-identical, 4.6× faster at n = 512 (108 → 23 s on one core; the context of an N = 512 trajectory).
void jacobi_eigen(std::vector<double>& a_io, int n, std::vector<double>& v_out) {
    const int ld = n + 8;
    std::vector<double> a((size_t)n * ld), vt((size_t)n * ld, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) a[(size_t)i * ld + j] = a_io[(size_t)i * n + j];
    for (int i = 0; i < n; ++i) vt[(size_t)i * ld + i] = 1.0;
    double fro = 0.0;
    for (double x : a_io) fro += x * x;
    fro = sqrt(fro);
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += a[(size_t)p * ld + q] * a[(size_t)p * ld + q];
        if (sqrt(off) <= 1e-17 * fro) break;
        for (int p = 0; p < n; ++p) {
            for (int q = p + 1; q < n; ++q) {
                double apq = a[(size_t)p * ld + q];
                if (fabs(apq) <= 1e-300) continue;
                double app = a[(size_t)p * ld + p], aqq = a[(size_t)q * ld + q];
                double theta = (aqq - app) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {  // rotate columns p, q
                    double akp = a[(size_t)k * ld + p], akq = a[(size_t)k * ld + q];
                    a[(size_t)k * ld + p] = c * akp - s * akq;
                    a[(size_t)k * ld + q] = s * akp + c * akq;
                }
                double* ap = &a[(size_t)p * ld];
                double* aq = &a[(size_t)q * ld];
                for (int k = 0; k < n; ++k) {  // rotate rows p, q
                    double apk = ap[k], aqk = aq[k];
                    ap[k] = c * apk - s * aqk;
                    aq[k] = s * apk + c * aqk;
                }
                double* vp = &vt[(size_t)p * ld];
                double* vq = &vt[(size_t)q * ld];
                for (int k = 0; k < n; ++k) {  // eigenvector columns p, q (rows of vᵀ)
                    double vkp = vp[k], vkq = vq[k];
                    vp[k] = c * vkp - s * vkq;
                    vq[k] = s * vkp + c * vkq;
                }
            }
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) a_io[(size_t)i * n + j] = a[(size_t)i * ld + j];
    v_out.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) v_out[(size_t)i * n + j] = vt[(size_t)j * ld + i];
}

namespace {
// Eigen-decompositions of the operator Gram matrices already computed in this process, keyed by the
// matrix itself (a context of the same N, σ and time grid reuses it: N = 512 takes ≈ 20 s to factorise).
struct EigenMemo {
    int n;
    std::vector<double> g, a, v;  // input, decomposed a (eigenvalues on the diagonal), eigenvectors
};
std::mutex g_eigen_mu;
std::vector<EigenMemo> g_eigen_memo;
}  // namespace

void jacobi_eigen_memo(std::vector<double>& a, int n, std::vector<double>& v) {
    {
        std::lock_guard<std::mutex> lk(g_eigen_mu);
        for (const EigenMemo& m : g_eigen_memo)
            if (m.n == n && m.g == a) {
                a = m.a;
                v = m.v;
                return;
            }
    }
    EigenMemo m{n, a, {}, {}};
    jacobi_eigen(a, n, v);
    m.a = a;
    m.v = v;
    std::lock_guard<std::mutex> lk(g_eigen_mu);
    if (g_eigen_memo.size() >= 8) g_eigen_memo.erase(g_eigen_memo.begin());
    g_eigen_memo.push_back(std::move(m));
}

/* fp32 LU with partial pivoting in LAPACK's recursive order (sgetrf2: factor the left half of the
   columns, swap, triangular solve, Schur update, factor the right half) followed by sgetrs's
   substitutions.  numpy.linalg.solve — what trajectory.py:77 runs — is LAPACK sgesv; K is
   numerically singular (cond ≈ 1e19), so α0's null-space part is rounding noise whose size depends
   on the elimination order: the recursive order keeps |α0| at the reference's ~1e3 where the
   right-looking textbook loop reached 4e4 (N=50), with K·α0·J within 3e-4 of the reference's. */
void getrf2_f32(int m, int n, float* A, int lda, int* ipiv) {
    if (n == 1) {
        int p = 0;
        for (int i = 1; i < m; ++i)
            if (fabsf(A[(size_t)i * lda]) > fabsf(A[(size_t)p * lda])) p = i;
        ipiv[0] = p;
        if (p != 0) {
            float t = A[0];
            A[0] = A[(size_t)p * lda];
            A[(size_t)p * lda] = t;
        }
        if (A[0] != 0.f) {
            const float r = 1.f / A[0]; /* LAPACK scales by the reciprocal */
            for (int i = 1; i < m; ++i) A[(size_t)i * lda] *= r;
        }
        return;
    }
    const int n1 = (m < n ? m : n) / 2, n2 = n - n1;
    getrf2_f32(m, n1, A, lda, ipiv);
    for (int i = 0; i < n1; ++i) /* row swaps of the left panel on the right columns */
        if (ipiv[i] != i)
            for (int j = n1; j < n; ++j) {
                float t = A[(size_t)i * lda + j];
                A[(size_t)i * lda + j] = A[(size_t)ipiv[i] * lda + j];
                A[(size_t)ipiv[i] * lda + j] = t;
            }
    for (int i = 1; i < n1; ++i) /* A12 = L11⁻¹·A12 (unit lower) */
        for (int k = 0; k < i; ++k) {
            const float l = A[(size_t)i * lda + k];
            for (int j = n1; j < n; ++j) A[(size_t)i * lda + j] -= l * A[(size_t)k * lda + j];
        }
    for (int i = n1; i < m; ++i) /* A22 −= A21·A12 */
        for (int j = n1; j < n; ++j) {
            float s = 0.f;
            for (int k = 0; k < n1; ++k) s += A[(size_t)i * lda + k] * A[(size_t)k * lda + j];
            A[(size_t)i * lda + j] -= s;
        }
    getrf2_f32(m - n1, n2, A + (size_t)n1 * lda + n1, lda, ipiv + n1);
    for (int i = n1; i < (m < n ? m : n); ++i) {
        ipiv[i] += n1;
        if (ipiv[i] != i) /* the right factorisation's swaps on the left columns */
            for (int j = 0; j < n1; ++j) {
                float t = A[(size_t)i * lda + j];
                A[(size_t)i * lda + j] = A[(size_t)ipiv[i] * lda + j];
                A[(size_t)ipiv[i] * lda + j] = t;
            }
    }
}

/* A·X = B, A n×n, B / X n×nrhs, row-major; returns false if a pivot is exactly 0. */
bool lu_solve_f32(int n, const float* A_in, const float* B_in, int nrhs, float* X) {
    float* A = (float*)malloc(sizeof(float) * (size_t)n * n);
    int* ipiv = (int*)malloc(sizeof(int) * (size_t)n);
    bool ok = true;
    memcpy(A, A_in, sizeof(float) * (size_t)n * n);
    memcpy(X, B_in, sizeof(float) * (size_t)n * nrhs);
    getrf2_f32(n, n, A, n, ipiv);
    for (int i = 0; i < n; ++i) {
        if (A[(size_t)i * n + i] == 0.f) ok = false;
        if (ipiv[i] != i)
            for (int j = 0; j < nrhs; ++j) {
                float t = X[(size_t)i * nrhs + j];
                X[(size_t)i * nrhs + j] = X[(size_t)ipiv[i] * nrhs + j];
                X[(size_t)ipiv[i] * nrhs + j] = t;
            }
    }
    if (ok) {
        for (int j = 0; j < nrhs; ++j) {
            for (int i = 1; i < n; ++i) {
                float s = X[(size_t)i * nrhs + j];
                for (int k = 0; k < i; ++k) s -= A[(size_t)i * n + k] * X[(size_t)k * nrhs + j];
                X[(size_t)i * nrhs + j] = s;
            }
            for (int i = n - 1; i >= 0; --i) {
                float s = X[(size_t)i * nrhs + j];
                for (int k = i + 1; k < n; ++k) s -= A[(size_t)i * n + k] * X[(size_t)k * nrhs + j];
                X[(size_t)i * nrhs + j] = s / A[(size_t)i * n + i];
            }
        }
    }
    free(A);
    free(ipiv);
    return ok;
}

// ------------------------------------------------ legacy threefry (J)
static uint32_t rotl32(uint32_t v, int r) { return (v << r) | (v >> (32 - r)); }

void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
    static const int rot[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
    static const int inj[5][2] = {{1, 2}, {2, 0}, {0, 1}, {1, 2}, {2, 0}};
    const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
    uint32_t a = x0 + ks[0], b = x1 + ks[1];
    for (int i = 0; i < 5; ++i) {
        for (int r = 0; r < 4; ++r) {
            a += b;
            b = rotl32(b, rot[i % 2][r]);
            b ^= a;
        }
        a += ks[inj[i][0]];
        b += ks[inj[i][1]] + (uint32_t)(i + 1);
    }
    x0 = a;
    x1 = b;
}

double erfinv_f64(double y) {
    if (y <= -1.0) return -INFINITY;
    if (y >= 1.0) return INFINITY;
    const double a = 0.147, ln = log(1.0 - y * y);
    const double t1 = 2.0 / (M_PI * a) + ln / 2.0;
    double x = copysign(sqrt(sqrt(t1 * t1 - ln / a) - t1), y);
    for (int it = 0; it < 60; ++it) {  // Newton on erf(x) = y
        const double step = (erf(x) - y) / (2.0 / sqrt(M_PI) * exp(-x * x));
        x -= step;
        if (fabs(step) < 1e-17 * (1.0 + fabs(x))) break;
    }
    return x;
}

void fill_frag(std::vector<float>& out, int M, int K, const std::vector<double>& A /*row-major M×K*/, bool kperm) {
    out.assign((size_t)irm::frag_floats(M, K), 0.f);
    for (int r = 0; r < M; ++r)
        for (int k = 0; k < K; ++k)
            out[(size_t)(kperm ? irm::frag_index_kp(r, k, K) : irm::frag_index(r, k, K))] = (float)A[(size_t)r * K + k];
}

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// t = jnp.linspace(0, 1, N) in fp32 (trajectory.py:35)
void support_times(int N, float* t) {
    const float div = (float)(N - 1);
    for (int i = 0; i < N - 1; ++i) {
        const float st = (float)i / div;
        t[i] = 0.f * (1.f - st) + 1.f * st;
    }
    t[N - 1] = 1.f;
}

// Kernel matrices of M evaluation times against N support times (M×N, row = evaluation time; outputs
// nullable): entry (i, j) = kernel_f(support[j], eval[i]) in fp32 as the reference evaluates km / dkm
// (trajectory.py:14-19, 40-48) — K and dK themselves for eval = support (the context's), the query
// matrices of eval_any for any other grid, the same arithmetic by construction.
void kernel_matrices(const float* support, int N, float rbf_variance, const float* eval, int M, float* km, float* dkm) {
    const double sig = decimal_double(rbf_variance);
    const float two_s2 = (float)(2.0 * sig * sig), s2 = (float)(sig * sig);
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j) {
            const float d = support[j] - eval[i];
            const float e = expf(-(d * d) / two_s2);
            if (km) km[(size_t)i * N + j] = e;
            if (dkm) dkm[(size_t)i * N + j] = d / s2 * e;
        }
}

// =============================================================== operators
const char* build_operators(const irm_params& p, HostOperators& ops) {
    const int N = p.n_timesteps, D = p.n_joints;

    // ---- Trajectory.__init__ (trajectory.py:31-42), fp32 as the reference
    ops.t.resize(N);
    ops.cvec.resize(N);
    support_times(N, ops.t.data());
    for (int i = 0; i < N; ++i) {
        const float tt = ops.t[i], t3 = tt * tt * tt, t4 = t3 * tt, t5 = t4 * tt;
        ops.cvec[i] = 6.f * t5 - 15.f * t4 + 10.f * t3;
    }
    ops.K.resize((size_t)N * N);
    ops.dK.resize((size_t)N * N);
    kernel_matrices(ops.t.data(), N, p.rbf_variance, ops.t.data(), N, ops.K.data(), ops.dK.data());
    ops.J.assign(p.jac, p.jac + (size_t)D * D);

    // ---- operator factorisation F = L·V_R
    // optimiser row layout: position half rows 0..N-1, velocity half from row NK
    const int NK = round_up(N, 16), MP = 2 * NK;
    std::vector<double> Ld((size_t)2 * N * N);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            Ld[(size_t)i * N + j] = ops.K[(size_t)i * N + j];
            Ld[(size_t)(N + i) * N + j] = ops.dK[(size_t)i * N + j];
        }
    int R = 0, RP = 0;
    std::vector<double> Vd;  // N × RP
    if (p.operator_rank < 0) {  // dense: F = L, V = I
        R = N;
        RP = NK;
        Vd.assign((size_t)N * RP, 0.0);
        for (int i = 0; i < N; ++i) Vd[(size_t)i * RP + i] = 1.0;
        ops.trunc = 0.f;
    } else {
        std::vector<double> G((size_t)N * N, 0.0), Vfull, LdT((size_t)N * 2 * N);
        for (int m = 0; m < 2 * N; ++m)  // Lᵀ rows: the Gram sums read contiguously (same sums, same order)
            for (int i = 0; i < N; ++i) LdT[(size_t)i * 2 * N + m] = Ld[(size_t)m * N + i];
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) {
                double s = 0.0;
                const double* li = &LdT[(size_t)i * 2 * N];
                const double* lj = &LdT[(size_t)j * 2 * N];
                for (int m = 0; m < 2 * N; ++m) s += li[m] * lj[m];
                G[(size_t)i * N + j] = G[(size_t)j * N + i] = s;
            }
        jacobi_eigen_memo(G, N, Vfull);
        std::vector<int> order(N);
        for (int i = 0; i < N; ++i) order[i] = i;
        std::sort(order.begin(), order.end(),
                  [&](int a, int b) { return G[(size_t)a * N + a] > G[(size_t)b * N + b]; });
        const double l0 = G[(size_t)order[0] * N + order[0]];
        if (p.operator_rank > 0) {
            R = std::min(p.operator_rank, N);
        } else {
            const double tol = p.operator_tol > 0.f ? p.operator_tol : 1e-12;
            R = N;
            for (int r = 16; r < N; r += 16) {
                const double lr = std::max(0.0, G[(size_t)order[r] * N + order[r]]);
                if (lr / l0 < tol) { R = r; break; }
            }
        }
        RP = round_up(R, 16);
        ops.trunc = (R < N) ? (float)(std::max(0.0, G[(size_t)order[R] * N + order[R]]) / l0) : 0.f;
        auto lam = [&](int r) { return (r < R) ? (float)(std::max(0.0, G[(size_t)order[r] * N + order[r]]) / l0) : 0.f; };
        ops.lam16 = lam(16);
        ops.lam24 = lam(24);
        Vd.assign((size_t)N * RP, 0.0);
        // Rank slot of component r.  At RP = 32 the second k-quad interleaves components 16-23 and
        // 24-31 so that the lean kernel's MFMAs 2 and 3 of that quad (k-permuted fragments: MFMA j
        // covers rows j, 4+j, 8+j, 12+j of a quad) see only components 24-31, whose singular values
        // are at fp32 noise (σ_24/σ_0 ≈ 3e-8 at N = 128) — k_lean skips those two MFMAs (rank 24 in
        // stage 2).  Every other use is a sum over all slots, so the order does not matter there.
        auto slot = [&](int r) {
            if (RP != 32 || r < 16) return r;
            const int j = r - 16, hi = j >= 8, q = j & 7;  // q-th of the 8 components of its half
            return 16 + 4 * (q >> 1) + (q & 1) + (hi ? 2 : 0);
        };
        for (int i = 0; i < N; ++i)
            for (int r = 0; r < R; ++r) Vd[(size_t)i * RP + slot(r)] = Vfull[(size_t)i * N + order[r]];
    }
    ops.R = R;
    ops.RP = RP;
    ops.NK = NK;
    ops.MP = MP;
    std::vector<double> F((size_t)2 * N * RP, 0.0);  // F = L·V
    for (int m = 0; m < 2 * N; ++m)
        for (int r = 0; r < RP; ++r) {
            double s = 0.0;
            for (int j = 0; j < N; ++j) s += Ld[(size_t)m * N + j] * Vd[(size_t)j * RP + r];
            F[(size_t)m * RP + r] = s;
        }

    // fragments
    std::vector<double> A;
    {  // K, dK and their transposes, row-major fp32: the correctly rounded α-space
       // contractions (eval_exact / grad_exact) read one coalesced row per k-step
        ops.Kt.resize((size_t)N * N);
        ops.dKt.resize((size_t)N * N);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                ops.Kt[(size_t)j * N + i] = ops.K[(size_t)i * N + j];
                ops.dKt[(size_t)j * N + i] = ops.dK[(size_t)i * N + j];
            }
    }
    // F rows m < N (K part) → row m, m = N + j (dK part) → row NK + j
    auto frow = [&](int m) { return m < N ? m : NK + (m - N); };
    // Fᵀ (RP × MP): stage 1 contracts y = Fᵀ·[a; b].  The endpoint velocity rows (m = N, 2N−1)
    // are left out: the optimiser adds b'[0], b'[N−1] through their own operator columns (Hend,
    // Fbot) in every round, so a round whose stage 1 is dense because of a neighbour adds exact
    // zeros for them and a problem's arithmetic never depends on its workgroup neighbours.
    A.assign((size_t)RP * MP, 0.0);
    for (int m = 0; m < 2 * N; ++m) {
        if (m == N || m == 2 * N - 1) continue;
        for (int r = 0; r < RP; ++r) A[(size_t)r * MP + frow(m)] = F[(size_t)m * RP + r];
    }
    fill_frag(ops.F1, RP, MP, A);
    fill_frag(ops.F1p, RP, MP, A, true);
    A.assign((size_t)MP * RP, 0.0);  // F (MP × RP)
    for (int m = 0; m < 2 * N; ++m)
        for (int r = 0; r < RP; ++r) A[(size_t)frow(m) * RP + r] = F[(size_t)m * RP + r];
    fill_frag(ops.F2, MP, RP, A);
    fill_frag(ops.F2p, MP, RP, A, true);
    ops.Fbot.resize((size_t)N * RP);
    ops.Vr.resize((size_t)N * RP);
    for (int n = 0; n < N; ++n)
        for (int r = 0; r < RP; ++r) {
            ops.Fbot[(size_t)n * RP + r] = (float)F[(size_t)(N + n) * RP + r];
            ops.Vr[(size_t)n * RP + r] = (float)Vd[(size_t)n * RP + r];
        }
    {  // the lean kernel's α-space terms: V_Rᵀ (RP × NK) and V_R (NK × RP), k-permuted fragments,
       // and G's endpoint velocity columns hv_e = V_R·F[N+e]ᵀ (e ∈ {0, N−1}), NK each
        A.assign((size_t)RP * NK, 0.0);
        for (int n = 0; n < N; ++n)
            for (int r = 0; r < RP; ++r) A[(size_t)r * NK + n] = Vd[(size_t)n * RP + r];
        fill_frag(ops.VTp, RP, NK, A, true);
        fill_frag(ops.VTs, RP, NK, A);
        A.assign((size_t)NK * RP, 0.0);
        for (int n = 0; n < N; ++n)
            for (int r = 0; r < RP; ++r) A[(size_t)n * RP + r] = Vd[(size_t)n * RP + r];
        fill_frag(ops.VNp, NK, RP, A, true);
        fill_frag(ops.VNs, NK, RP, A);
        ops.HV.assign((size_t)2 * NK, 0.f);
        for (int e = 0; e < 2; ++e) {
            const int me = N + (e ? N - 1 : 0);
            for (int n = 0; n < N; ++n) {
                double acc = 0.0;
                for (int r = 0; r < RP; ++r) acc += Vd[(size_t)n * RP + r] * F[(size_t)me * RP + r];
                ops.HV[(size_t)e * NK + n] = (float)acc;
            }
        }
    }
    {  // h_e = F·F[N+e]ᵀ for the endpoint velocity rows e ∈ {0, N−1}, kernel row layout
        ops.H.assign((size_t)2 * MP, 0.f);
        for (int e = 0; e < 2; ++e) {
            const int me = N + (e ? N - 1 : 0);
            for (int m = 0; m < 2 * N; ++m) {
                double acc = 0.0;
                for (int r = 0; r < RP; ++r) acc += F[(size_t)m * RP + r] * F[(size_t)me * RP + r];
                ops.H[(size_t)e * MP + frow(m)] = (float)acc;
            }
        }
    }
    // initTrajectory basis: u = K⁻¹(1−c), w = K⁻¹c (fp32 LU, trajectory.py:77)
    {
        std::vector<float> rhs((size_t)N * 2), X((size_t)N * 2);
        for (int n = 0; n < N; ++n) {
            rhs[(size_t)n * 2] = 1.f - ops.cvec[n];
            rhs[(size_t)n * 2 + 1] = ops.cvec[n];
        }
        if (!lu_solve_f32(N, ops.K.data(), rhs.data(), 2, X.data())) return "kernel matrix K is exactly singular in fp32 LU";
        ops.u.resize(N);
        ops.w.resize(N);
        for (int n = 0; n < N; ++n) {
            ops.u[n] = X[(size_t)n * 2];
            ops.w[n] = X[(size_t)n * 2 + 1];
        }
    }
    return nullptr;
}

void read_env_switches(KParams& kp) {
    const char* g = getenv("IRM_GENERAL_KERNEL");  // diagnostics: force the general optimiser
    kp.lean_ok = (g && g[0] == '1') ? 0 : 1;
    const char* w = getenv("IRM_LEAN_WPL");
    kp.lean_wpl = w ? atoi(w) : 0;
    const char* nh = getenv("IRM_LEAN_NOHELP");
    kp.lean_nohelp = (nh && nh[0] == '1') ? 1 : 0;
    const char* tp = getenv("IRM_TRACE_PROBLEM");
    kp.trace_b = tp ? atoi(tp) : 0;
    // IRM_WORK_QUEUE=off|auto|<n>: the context's work-queue request until irm_set_work_queue is called
    const char* wq = getenv("IRM_WORK_QUEUE");
    kp.queue_groups = 0;
    if (wq && !strcmp(wq, "auto")) kp.queue_groups = -1;
    else if (wq && strcmp(wq, "off")) kp.queue_groups = std::max(0, atoi(wq));
}

// ---- kernel parameter template
const char* fill_kparams(const irm_params& p, const HostOperators& ops, KParams& kp) {
    const int N = p.n_timesteps, D = p.n_joints;
    kp.N = N;
    kp.D = D;
    kp.R = ops.R;
    kp.NK = ops.NK;
    kp.MP = ops.MP;
    kp.RP = ops.RP;
    kp.v_ident = p.operator_rank < 0 ? 1 : 0;
    kp.O = 0;
    kp.optimizer = p.optimizer;
    kp.max_inner = p.max_inner_iteration;
    kp.max_outer = p.max_outer_iteration;
    kp.max_bls = p.max_bls_iteration;
    kp.cvdl = p.constraint_violating_dependant_loss ? 1 : 0;
    kp.llr = p.loop_loss_reduction;
    kp.lci = p.lambda_constraint_increase;
    kp.lsg0 = p.lambda_sg_constraint;
    kp.ljl0 = p.lambda_jl_constraint;
    kp.eps_p = p.eps_position;
    kp.eps_v = p.eps_velocity;
    kp.lmax = p.lambda_max_cost;
    kp.lreg = p.lambda_reg;
    // GD weight decay (1 − λ_reg·lr) per outer iteration, in fp32 as the reference evaluates it:
    // lr = dual_lr[k] is an fp32 array element (optimizer_GD.py:38-39, :209) and the Python float
    // λ_reg enters weakly typed, so both the product and the difference round to fp32
    // (optimizer_GD.py:81, :185).  The product is rounded through a volatile: clang contracts across
    // statements under -ffp-contract=fast, so only the missing FMA of the default host target kept the
    // two roundings apart before (a -march with FMA would have fused them into one)
    for (int i = 0; i < IRM_MAX_LR; ++i) {
        volatile float prod = p.lambda_reg * p.gd_lr[i];
        kp.gd_c[i] = 1.f - prod;
    }
    kp.bls_lr0 = p.bls_lr_start;
    kp.bls_a = p.bls_alpha;
    kp.bls_bp = p.bls_beta_plus;
    kp.bls_bm = p.bls_beta_minus;
    kp.vmax = p.max_joint_velocity;
    kp.pmax = p.max_joint_position;
    kp.pmin = p.min_joint_position;
    {  // trajectory.py:31-32, 221-222, 251 (Python doubles → fp32)
        const double mean = 0.5 * ((double)p.max_joint_position + (double)p.min_joint_position);
        const double stdp = 0.5 * ((double)p.max_joint_position - mean);
        kp.mean_pos = (float)mean;
        kp.std_pos = (float)stdp;
        kp.std2 = kp.std_pos * kp.std_pos;
        kp.vmax2 = kp.vmax * kp.vmax;
        kp.thr_hi = (float)((double)p.joint_safety_limit * (double)p.max_joint_position);
        kp.thr_lo = (float)((double)p.joint_safety_limit * (double)p.min_joint_position);
        kp.thr_v = (float)((double)p.joint_safety_limit * (double)p.max_joint_velocity);
        // --constraint-violating-dependant-loss false (trajectory.py:221-222, 251: the penalties apply to
        // every element): thresholds that every finite joint position / velocity passes, so the kernels
        // form the masks without the flag (one scalar op fewer per mask element and round).  Deliberate
        // deviation: a NaN joint value fails every compare, so its penalty term is masked
        // off (0) where the reference's unmasked penalty would carry the NaN into the loss — only a diverged
        // trajectory (non-finite state) can see the difference, and its loss is non-finite either way
        if (!p.constraint_violating_dependant_loss) {
            kp.thr_hi = -INFINITY;
            kp.thr_lo = INFINITY;
            kp.thr_v = -1.f;
        }
        kp.invN = 1.f / (float)N;
        kp.inv_std_pos = 1.f / kp.std_pos;
        kp.inv_vmax = 1.f / kp.vmax;
        kp.inv_std2 = 1.f / kp.std2;
        kp.inv_vmax2 = 1.f / kp.vmax2;
        kp.Nmagic = (uint32_t)((((uint64_t)1 << 32) + (uint64_t)N - 1) / (uint64_t)N);
        kp.NDmagic = (uint32_t)((((uint64_t)1 << 32) + (uint64_t)(N * D) - 1) / (uint64_t)(N * D));
    }
    for (int i = 0; i < IRM_MAX_LR; ++i) kp.gd_lr[i] = p.gd_lr[i];
    for (int i = 0; i < IRM_MAX_JOINTS; ++i) kp.link[i] = p.link_length[i];
    {
        std::vector<double> Jd((size_t)D * D), JtJ((size_t)D * D, 0.0);
        for (int i = 0; i < D * D; ++i) Jd[i] = p.jac[i];
        for (int a = 0; a < D; ++a)
            for (int b = 0; b < D; ++b) {
                double s = 0.0;
                for (int k = 0; k < D; ++k) s += Jd[(size_t)k * D + a] * Jd[(size_t)k * D + b];
                JtJ[(size_t)a * D + b] = s;
            }
        std::vector<float> eye((size_t)D * D, 0.f), Jinv((size_t)D * D);
        for (int i = 0; i < D; ++i) eye[(size_t)i * D + i] = 1.f;
        if (!lu_solve_f32(D, p.jac, eye.data(), D, Jinv.data())) return "J is singular";
        // (JᵀJ)⁻¹ by Gauss-Jordan in fp64, and w = (JᵀJ)⁻¹·Jᵀ1 (BLS norms from y' = y·JᵀJ)
        std::vector<double> Mi((size_t)D * D, 0.0), Mw(JtJ);
        for (int i = 0; i < D; ++i) Mi[(size_t)i * D + i] = 1.0;
        for (int col = 0; col < D; ++col) {
            int piv = col;
            for (int r = col + 1; r < D; ++r)
                if (std::fabs(Mw[(size_t)r * D + col]) > std::fabs(Mw[(size_t)piv * D + col])) piv = r;
            for (int k = 0; k < D; ++k) {
                std::swap(Mw[(size_t)col * D + k], Mw[(size_t)piv * D + k]);
                std::swap(Mi[(size_t)col * D + k], Mi[(size_t)piv * D + k]);
            }
            const double d = Mw[(size_t)col * D + col];
            for (int k = 0; k < D; ++k) {
                Mw[(size_t)col * D + k] /= d;
                Mi[(size_t)col * D + k] /= d;
            }
            for (int r = 0; r < D; ++r) {
                if (r == col) continue;
                const double f = Mw[(size_t)r * D + col];
                for (int k = 0; k < D; ++k) {
                    Mw[(size_t)r * D + k] -= f * Mw[(size_t)col * D + k];
                    Mi[(size_t)r * D + k] -= f * Mi[(size_t)col * D + k];
                }
            }
        }
        for (int a = 0; a < D; ++a) {
            double w = 0.0;
            for (int b = 0; b < D; ++b) {
                double u = 0.0;
                for (int i = 0; i < D; ++i) u += (double)p.jac[(size_t)i * D + b];
                w += Mi[(size_t)a * D + b] * u;
            }
            kp.wal[a] = (float)w;
        }
        for (int i = 0; i < D * D; ++i) kp.Minv[i] = (float)Mi[i];
        for (int i = 0; i < D * D; ++i) {
            kp.J[i] = p.jac[i];
            kp.JtJ[i] = (float)JtJ[i];
            kp.Jinv[i] = Jinv[i];
        }
    }
    kp.lam_max = p.lambda_max_cost;
    kp.one_m_lmax = (float)(1.0 - (double)p.lambda_max_cost);
    kp.record_series = p.record_series ? 1 : 0;
    kp.whole_robot = p.whole_robot_cost ? 1 : 0;
    read_env_switches(kp);
    // k_lean drops the components 16-31 from the waypoint direction (terms ∝ λ_r) and the residual
    // projection, and 24-31 from G (∝ σ_r): only where those are at fp32 noise (σ = 0.1: λ16/λ0 ≈
    // 1.5e-7, λ24/λ0 ≈ 6e-16).  A flatter spectrum (smaller --rbf-variance, e.g. 0.07: 4e-4 / 7e-9)
    // still selects R = 32; it runs the general kernel at the full rank instead.
    if (!lean_rank_cut_ok(ops.lam16, ops.lam24)) kp.lean_ok = 0;
    kp.max_series = p.max_series > 0 ? p.max_series : 1 + p.max_outer_iteration * p.max_inner_iteration;
    return nullptr;
}

// Workgroup shape for a launch of B trajectories: one lane per (trajectory,
// waypoint), NW = N rounded up to 64 lanes per trajectory, TB trajectories
// per workgroup with TB·D ≤ 16 MFMA columns and TB·NW ≤ 1024 threads.  For
// the optimiser TB defaults to ⌈B / #CU⌉ (one workgroup per CU when B is
// small) and the operator fragments are staged into LDS when they fit.
int choose_shape(int N, int D, int NK, int RP, int MP, int traj_per_block, int num_cus, int B, bool optimizer,
                 KParams& kp, int* lds_bytes_out) {
    kp.N = N;
    kp.D = D;
    kp.NK = NK;
    kp.RP = RP;
    kp.MP = MP;
    kp.NW = round_up(N, 64);
    // D ≥ 5 needs > 128 VGPRs per lane: keep those workgroups at ≤ 512 threads
    const int maxthreads = (D >= 5) ? 512 : irm::kMaxThreads;
    // Optimiser workgroups of N ≤ 128 stay at ≤ 512 threads: the 1024-thread variants are capped at
    // 128 VGPRs and spill (C3 with five trajectories per workgroup: 1.47 ms vs 0.79 ms for four), so a
    // large batch is better served by more 4-trajectory workgroups (bench.py --tb 5 vs default).
    const int cap = (optimizer && kp.NW <= 128) ? std::min(maxthreads, 512) : maxthreads;
    const int tbmax = std::max(1, std::min(irm::kCols / D, cap / kp.NW));
    int tb = tbmax;
    if (optimizer && traj_per_block > 0) tb = std::min(traj_per_block, tbmax);
    else if (optimizer) tb = std::min(tbmax, std::max(1, (B + num_cus - 1) / std::max(1, num_cus)));
    tb = std::max(1, std::min(tb, std::max(1, B)));
    const size_t lds_cap = 160 * 1024;
    // Under-filled GPU (fewer workgroups than half the CUs: small batches, C2's single
    // trajectory): pad the optimiser's workgroup with waves that take no trajectory
    // (tvalid = false in the kernels) up to 512 threads.  They share the MFMA stages (stage-2
    // tiles and stage-1 units are distributed over all waves), which shortens every round's
    // latency chain; the per-tile arithmetic is unchanged, so results are bit-identical.
    const char* pw = getenv("IRM_PAD_WAVES");
    const bool pad_ok = optimizer && !(pw && pw[0] == '0');
    for (; tb >= 1; --tb) {
        kp.TB = tb;
        kp.BT = tb * kp.NW;
        if (pad_ok && 2 * ((B + tb - 1) / tb) <= num_cus && kp.BT < 512) kp.BT = 512;
        kp.nsplit = irm::stage1_splits(kp.NK);
        // the lean kernel (k_lean) runs one stage-1 unit per wave and is instantiated for 256- and
        // 512-thread workgroups: smaller optimiser workgroups get idle waves up to that size (e.g.
        // one N = 128 trajectory per workgroup: 2 → 4 waves), so that the lean kernel — and its
        // fp32-α rounding — serves them; the general kernel runs padded workgroups bit-identically
        if (optimizer && kp.BT < 512) {
            kp.BT = std::max(kp.BT, std::min(512, 64 * (kp.RP / 16) * kp.nsplit));
            kp.BT = kp.BT <= 256 ? 256 : 512;
        }
        if (optimizer) {
            kp.regops = irm::regops_fit(kp) ? 1 : 0;
            irm::Plan a = irm::plan_lds(kp, true, true, false, kp.moving != 0, kp.via != 0);
            if ((size_t)a.total * 4 <= lds_cap) {
                kp.ops_in_lds = 1;
                if (lds_bytes_out) *lds_bytes_out = a.total * 4;
                return tb;
            }
            irm::Plan b = irm::plan_lds(kp, false, true, false, kp.moving != 0, kp.via != 0);
            if ((size_t)b.total * 4 <= lds_cap) {
                kp.ops_in_lds = 0;
                kp.regops = 0;
                if (lds_bytes_out) *lds_bytes_out = b.total * 4;
                return tb;
            }
        } else {
            irm::Plan a = irm::plan_lds(kp, false, false, false, kp.moving != 0, kp.via != 0);
            if ((size_t)a.total * 4 <= lds_cap) {
                if (lds_bytes_out) *lds_bytes_out = a.total * 4;
                return tb;
            }
        }
    }
    return 0;
}

}  // namespace irm
