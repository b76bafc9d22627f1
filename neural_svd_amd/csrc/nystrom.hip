// The small dense work of a block eigensolver on a tall-skinny basis: what the Nystrom baseline (reference
// methods/nystrom.py:8-47 - Nystrom, Nystrom.evd, run_nystrom - which forms the n x n Gram matrix and calls a host
// eigh on it) needs beside the matrix-free product of rbf_apply.hip to find the top L <= 64 eigenpairs of
// G = k(xs, xs) / n by block subspace iteration with Rayleigh-Ritz (neural_svd_amd/nystrom.py):
//   nsvd_tsgram_f64     XtX = X^T X, XtY = X^T Y of two (n, m) float32 blocks, products and sums in float64 (the
//                       kernels and the body of the entry point are ts_dense.h's, shared with nystrom_svd.hip)
//   nsvd_ritz_step_f64  the m x m solve of one iteration in ONE workgroup, float64, matrices in LDS:
//                       eigh(sym(A)) = Q diag(theta) Q^T (cyclic Jacobi, round-robin parallel ordering),
//                       M = Q^T S Q, residuals sqrt(max(M_kk - theta_k^2 (2 - q_k^T C q_k), 0)), R = chol(M),
//                       T = Q R^-1
//   nsvd_ts_rotate      out = X T[:, :k] in float64, rounded once to float32
//   nsvd_ts_rotate2     out = X T1[:, :k] + Y T2[:, :k], the sum in float64, rounded once (SpINx's cotangents)
// m <= 80 throughout (64 pairs + 16 columns of oversampling). Every device loop has a trip count bounded by an argument
// or a constant; nothing waits on a data-dependent flag. No atomics: the row slices of the Gram are reduced in slice
// order by a second launch, so every result is bit-reproducible.
#include "ts_dense.h"

namespace {

constexpr int RZ_SWEEPS = 30;   // Jacobi sweep cap (float64, m <= 80: 6-10 sweeps in practice)
constexpr int RO_ROWS = 32;     // rows of X per workgroup of the rotation kernel

// out[rows of this workgroup][c < k] = sum_kk X[row][kk] T[kk][c]. T's first k columns wait in LDS as float64 (rows of
// NY_MAXM, zero beyond k); thread (tr, tc) = (t / 16, t % 16) owns rows tr, tr + 16 and columns tc + 16 b.
__global__ void __launch_bounds__(NY_THREADS) ts_rotate_kernel(const float* __restrict__ X, size_t ldx, int n, int m,
                                                               const double* __restrict__ T, int ldt, int k,
                                                               float* __restrict__ out, size_t ldo) {
    __shared__ double Ts[NY_MAXM][NY_MAXM];
    __shared__ float xs[RO_ROWS][NY_MAXM + 1];
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const long rb = (long)blockIdx.x * RO_ROWS;
    for (int e = t; e < m * NY_MAXM; e += NY_THREADS) {
        const int kk = e / NY_MAXM, c = e - kk * NY_MAXM;
        Ts[kk][c] = c < k ? T[(size_t)kk * ldt + c] : 0.0;
    }
    for (int e = t; e < RO_ROWS * m; e += NY_THREADS) {
        const int r = e / m, c = e - r * m;
        xs[r][c] = rb + r < n ? X[(size_t)(rb + r) * ldx + c] : 0.f;
    }
    __syncthreads();
    double acc[2][NY_CB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) acc[a][b] = 0.0;
    for (int kk = 0; kk < m; ++kk) {
        const double x0 = (double)xs[tr][kk], x1 = (double)xs[tr + 16][kk];
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) {
            const double tv = Ts[kk][tc + 16 * b];
            acc[0][b] = fma(x0, tv, acc[0][b]);
            acc[1][b] = fma(x1, tv, acc[1][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const long row = rb + tr + 16 * a;
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) {
            const int c = tc + 16 * b;
            if (row < n && c < k) out[(size_t)row * ldo + c] = (float)acc[a][b];
        }
    }
}

// out = X T1[:, :k] + Y T2[:, :k]: the same tile and thread map; the two terms pass through the same LDS one after the
// other and share the float64 accumulators, so the sum is rounded once.
__global__ void __launch_bounds__(NY_THREADS) ts_rotate2_kernel(const float* __restrict__ X, size_t ldx,
                                                                const float* __restrict__ Y, size_t ldy, int n, int m,
                                                                const double* __restrict__ T1, int ldt1,
                                                                const double* __restrict__ T2, int ldt2, int k,
                                                                float* __restrict__ out, size_t ldo) {
    __shared__ double Ts[NY_MAXM][NY_MAXM];
    __shared__ float xs[RO_ROWS][NY_MAXM + 1];
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const long rb = (long)blockIdx.x * RO_ROWS;
    double acc[2][NY_CB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) acc[a][b] = 0.0;
    for (int term = 0; term < 2; ++term) {
        const float* Z = term ? Y : X;
        const size_t ldz = term ? ldy : ldx;
        const double* T = term ? T2 : T1;
        const int ldt = term ? ldt2 : ldt1;
        __syncthreads();
        for (int e = t; e < m * NY_MAXM; e += NY_THREADS) {
            const int kk = e / NY_MAXM, c = e - kk * NY_MAXM;
            Ts[kk][c] = c < k ? T[(size_t)kk * ldt + c] : 0.0;
        }
        for (int e = t; e < RO_ROWS * m; e += NY_THREADS) {
            const int r = e / m, c = e - r * m;
            xs[r][c] = rb + r < n ? Z[(size_t)(rb + r) * ldz + c] : 0.f;
        }
        __syncthreads();
        for (int kk = 0; kk < m; ++kk) {
            const double x0 = (double)xs[tr][kk], x1 = (double)xs[tr + 16][kk];
#pragma unroll
            for (int b = 0; b < NY_CB; ++b) {
                const double tv = Ts[kk][tc + 16 * b];
                acc[0][b] = fma(x0, tv, acc[0][b]);
                acc[1][b] = fma(x1, tv, acc[1][b]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const long row = rb + tr + 16 * a;
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) {
            const int c = tc + 16 * b;
            if (row < n && c < k) out[(size_t)row * ldo + c] = (float)acc[a][b];
        }
    }
}

// ---- the m x m solve ------------------------------------------------------------------------------------------------
struct RitzLds {
    double *B0, *B1, *B2;  // three (m, ld) matrices, ld = m | 1 (odd: a column walk touches every bank pair once)
    double *th, *ths;      // (m) eigenvalues as found / sorted; th is reused for the Cholesky diagonal
    double *cc, *ss;       // (mp / 2) rotations of a round
    double* red;           // (8) block reductions
    int *pp, *qq, *perm;   // (mp / 2) pairs of a round, (m) sorted position -> column
};

__host__ __device__ inline size_t ritz_lds_doubles(int m) {
    const int ld = m | 1, mp = (m + 1) & ~1;
    return (size_t)3 * m * ld + 2 * m + mp + 8;
}
__host__ __device__ inline size_t ritz_lds_bytes(int m) {
    const int mp = (m + 1) & ~1;
    return ritz_lds_doubles(m) * sizeof(double) + (size_t)(mp + m) * sizeof(int);
}

// sums of two values over the workgroup, the same result in every thread, in a fixed order
__device__ __forceinline__ void ritz_block_sum2(double& a, double& b, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = a;
        red[4 + (threadIdx.x >> 6)] = b;
    }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[4] + red[5]) + (red[6] + red[7]);
}

__global__ void __launch_bounds__(NY_THREADS) ritz_step_kernel(const double* __restrict__ S, const double* __restrict__ A,
                                                               const double* __restrict__ C, int m,
                                                               double* __restrict__ theta,
                                                               double* __restrict__ resid, double* __restrict__ Q,
                                                               double* __restrict__ T, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, ld = m | 1, mp = (m + 1) & ~1, np = mp >> 1, mm = m * m;
    RitzLds w;
    w.B0 = sm;
    w.B1 = w.B0 + m * ld;
    w.B2 = w.B1 + m * ld;
    w.th = w.B2 + m * ld;
    w.ths = w.th + m;
    w.cc = w.ths + m;
    w.ss = w.cc + np;
    w.red = w.ss + np;
    w.pp = (int*)(w.red + 8);
    w.qq = w.pp + np;
    w.perm = w.qq + np;
    int bits = 0;

    if (A) {
        // B0 = sym(A), B1 = I
        for (int e = t; e < mm; e += NY_THREADS) {
            const int i = e / m, j = e - i * m;
            w.B0[i * ld + j] = 0.5 * (A[i * m + j] + A[j * m + i]);
            w.B1[i * ld + j] = i == j ? 1.0 : 0.0;
        }
        bool converged = false;
        for (int sweep = 0; sweep <= RZ_SWEEPS; ++sweep) {
            __syncthreads();
            double off = 0.0, fro = 0.0;
            for (int e = t; e < mm; e += NY_THREADS) {
                const int i = e / m, j = e - i * m;
                const double v = w.B0[i * ld + j];
                fro = fma(v, v, fro);
                if (i != j) off = fma(v, v, off);
            }
            ritz_block_sum2(off, fro, w.red);
            if (off <= 1e-30 * fro) {  // |off-diagonal|_F <= 1e-15 |A|_F (false for NaN: runs to the cap)
                converged = true;
                break;
            }
            if (sweep == RZ_SWEEPS) break;
            // one sweep: mp - 1 rounds of the round-robin tournament, np disjoint pairs each (index m is the bye of an odd m)
            for (int r = 0; r < mp - 1; ++r) {
                if (t < np) {
                    const int a = t == 0 ? mp - 1 : (r + t) % (mp - 1);
                    const int b = t == 0 ? r : (r - t + mp - 1) % (mp - 1);
                    const int p = min(a, b), q = max(a, b);
                    double c = 1.0, s = 0.0;
                    if (q < m) {
                        const double apq = w.B0[p * ld + q];
                        if (apq != 0.0) {
                            const double zeta = (w.B0[q * ld + q] - w.B0[p * ld + p]) / (2.0 * apq);
                            const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                            c = 1.0 / sqrt(1.0 + tt * tt);
                            s = tt * c;
                        }
                    }
                    w.pp[t] = q < m ? p : -1;
                    w.qq[t] = q;
                    w.cc[t] = c;
                    w.ss[t] = s;
                }
                __syncthreads();
                // columns p, q of A and of the eigenvector matrix: A <- A J, Q <- Q J
                for (int e = t; e < np * m; e += NY_THREADS) {
                    const int pr = e / m, i = e - pr * m, p = w.pp[pr], q = w.qq[pr];
                    if (p < 0) continue;
                    const double c = w.cc[pr], s = w.ss[pr];
                    const double ap = w.B0[i * ld + p], aq = w.B0[i * ld + q];
                    w.B0[i * ld + p] = c * ap - s * aq;
                    w.B0[i * ld + q] = s * ap + c * aq;
                    const double vp = w.B1[i * ld + p], vq = w.B1[i * ld + q];
                    w.B1[i * ld + p] = c * vp - s * vq;
                    w.B1[i * ld + q] = s * vp + c * vq;
                }
                __syncthreads();
                // rows p, q of A: A <- J^T A; the annihilated pair is set to zero exactly
                for (int e = t; e < np * m; e += NY_THREADS) {
                    const int pr = e / m, j = e - pr * m, p = w.pp[pr], q = w.qq[pr];
                    if (p < 0) continue;
                    const double c = w.cc[pr], s = w.ss[pr];
                    const double ap = w.B0[p * ld + j], aq = w.B0[q * ld + j];
                    w.B0[p * ld + j] = j == q ? 0.0 : c * ap - s * aq;
                    w.B0[q * ld + j] = j == p ? 0.0 : s * ap + c * aq;
                }
                __syncthreads();
            }
        }
        if (!converged) bits |= NSVD_RITZ_SWEEP_CAP;
        __syncthreads();
        if (t < m) {
            w.th[t] = w.B0[t * ld + t];
            w.perm[t] = t;
        }
        __syncthreads();
        // descending, ties by ascending index
        if (t < m) {
            const double v = w.th[t];
            int rank = 0;
            for (int j = 0; j < m; ++j) {
                const double u = w.th[j];
                rank += (u > v || (u == v && j < t)) ? 1 : 0;
            }
            if (!(v != v)) w.perm[rank] = t;  // (a NaN leaves the identity entry: indices stay in range)
        }
        __syncthreads();
        if (t < m) {
            const int src = min(max(w.perm[t], 0), m - 1);
            w.perm[t] = src;
            w.ths[t] = w.th[src];
            if (theta) theta[t] = w.ths[t];
        }
        __syncthreads();
        // B0 = the eigenvectors in sorted order (A itself is no longer needed)
        for (int e = t; e < mm; e += NY_THREADS) {
            const int i = e / m, j = e - i * m;
            const double v = w.B1[i * ld + w.perm[j]];
            w.B0[i * ld + j] = v;
            if (Q) Q[e] = v;
        }
    } else {
        for (int e = t; e < mm; e += NY_THREADS) {
            const int i = e / m, j = e - i * m;
            w.B0[i * ld + j] = i == j ? 1.0 : 0.0;
            if (Q) Q[e] = i == j ? 1.0 : 0.0;
        }
        if (t < m) {
            w.ths[t] = 0.0;
            if (theta) theta[t] = 0.0;
        }
    }
    // dk = q_k^T (C - I) q_k, C = V^T V of the basis as it is STORED (float32: orthonormal to ~1e-8 only). The residual
    // |W q - theta V q|^2 = M_kk - theta^2 (1 - dk); without dk the difference M_kk - theta^2 carries theta^2 dk, and
    // its square root a floor of theta sqrt(|dk|) ~ 1e-4 theta under every residual. Thread k keeps dk.
    double dk = 0.0;
    if (A && C) {
        __syncthreads();
        for (int e = t; e < mm; e += NY_THREADS) {
            const int i = e / m, j = e - i * m;
            w.B2[i * ld + j] = C[e] - (i == j ? 1.0 : 0.0);
        }
        __syncthreads();
        for (int e = t; e < mm; e += NY_THREADS) {
            const int i = e / m, j = e - i * m;
            double s = 0.0;
            for (int k = 0; k < m; ++k) s = fma(w.B2[i * ld + k], w.B0[k * ld + j], s);
            w.B1[i * ld + j] = s;
        }
        __syncthreads();
        if (t < m)
            for (int i = 0; i < m; ++i) dk = fma(w.B0[i * ld + t], w.B1[i * ld + t], dk);
        __syncthreads();
    }
    // B2 = S; with a rotation: B1 = S Q, then B2 = M = Q^T (S Q)
    for (int e = t; e < mm; e += NY_THREADS) {
        const int i = e / m, j = e - i * m;
        w.B2[i * ld + j] = S[e];
    }
    __syncthreads();
    if (A) {
        for (int e = t; e < mm; e += NY_THREADS) {
            const int i = e / m, j = e - i * m;
            double s = 0.0;
            for (int k = 0; k < m; ++k) s = fma(w.B2[i * ld + k], w.B0[k * ld + j], s);
            w.B1[i * ld + j] = s;
        }
        __syncthreads();
        for (int e = t; e < mm; e += NY_THREADS) {
            const int i = e / m, j = e - i * m;
            double s = 0.0;
            for (int k = 0; k < m; ++k) s = fma(w.B0[k * ld + i], w.B1[k * ld + j], s);
            w.B2[i * ld + j] = s;
        }
        __syncthreads();
    }
    if (resid && t < m) {
        const double d = w.B2[t * ld + t] - w.ths[t] * w.ths[t] * (1.0 - dk);
        resid[t] = A && d > 0.0 ? sqrt(d) : 0.0;
    }
    // R = chol(M), upper, in the upper triangle of B2 (its diagonal stays M's; R_jj goes to th)
    int bad = m;
    for (int j = 0; j < m; ++j) {
        const double d = w.B2[j * ld + j];  // the same LDS word in every thread: the branch is uniform
        if (!(d > 0.0) || !(d < 1.7e308)) {
            bad = j;
            break;
        }
        const double rj = sqrt(d), inv = 1.0 / rj;
        if (t == 0) w.th[j] = rj;
        for (int c = j + 1 + t; c < m; c += NY_THREADS) w.B2[j * ld + c] *= inv;
        __syncthreads();
        const int rem = m - j - 1;
        for (int e = t; e < rem * rem; e += NY_THREADS) {
            const int i = j + 1 + e / rem, c = j + 1 + e % rem;
            if (c >= i) w.B2[i * ld + c] = fma(-w.B2[j * ld + i], w.B2[j * ld + c], w.B2[i * ld + c]);
        }
        __syncthreads();
    }
    if (bad < m) bits |= NSVD_RITZ_BAD_PIVOT;
    __syncthreads();
    // T = Q R^-1 by forward substitution along each row of Q, in place in B0 (one thread per row)
    if (t < m) {
        double* row = w.B0 + t * ld;
        for (int j = 0; j < m; ++j) {
            if (j >= bad) {
                row[j] = 0.0;
                continue;
            }
            double s = row[j];
            for (int k = 0; k < j; ++k) s = fma(-row[k], w.B2[k * ld + j], s);
            row[j] = s / w.th[j];
        }
    }
    __syncthreads();
    int nonfinite = 0;
    for (int e = t; e < mm; e += NY_THREADS) {
        const int i = e / m, j = e - i * m;
        double v = w.B0[i * ld + j];
        if (!(fabs(v) < 1.7e308)) {  // (overflow behind a tiny positive pivot, or NaN)
            v = 0.0;
            nonfinite = 1;
        }
        T[e] = v;
    }
    if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
    if (t == 0 && bits) *status = *status | bits;
}

}  // namespace

extern "C" size_t nsvd_tsgram_f64_workspace_bytes(int n, int m) { return ts_gram_workspace_bytes(n, m, 2); }

extern "C" int nsvd_tsgram_f64(const float* X, long ldx, const float* Y, long ldy, int n, int m, double* XtX,
                               double* XtY, void* ws, size_t ws_bytes, void* stream) {
    if (!XtX && !XtY) return NSVD_EINVAL;
    return ts_gram<false>(X, ldx, Y, ldy, n, m, XtX, XtY, nullptr, ws, ws_bytes, stream);
}

extern "C" int nsvd_ritz_step_f64(const double* S, const double* A, const double* C, int m, double* theta,
                                  double* resid, double* Q, double* T, int* status, void* stream) {
    if (!S || !T || !status || m <= 0) return NSVD_EINVAL;
    if (m > NY_MAXM) return NSVD_EUNSUPPORTED;
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)ritz_step_kernel}, ritz_lds_bytes(NY_MAXM))) return rc;
    ritz_step_kernel<<<1, NY_THREADS, ritz_lds_bytes(m), (hipStream_t)stream>>>(S, A, C, m, theta, resid, Q,
                                                                                T, status);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_ts_rotate(const float* X, long ldx, int n, int m, const double* T, int ldt, int k, float* out,
                              long ldo, void* stream) {
    if (!X || !T || !out || n <= 0 || m <= 0 || k <= 0 || k > m || ldx < m || ldt < k || ldo < k) return NSVD_EINVAL;
    if (m > NY_MAXM) return NSVD_EUNSUPPORTED;
    ts_rotate_kernel<<<nsvd_cdiv(n, RO_ROWS), NY_THREADS, 0, (hipStream_t)stream>>>(X, (size_t)ldx, n, m, T, ldt, k, out,
                                                                                  (size_t)ldo);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_ts_rotate2(const float* X, long ldx, const float* Y, long ldy, int n, int m, const double* T1,
                               int ldt1, const double* T2, int ldt2, int k, float* out, long ldo, void* stream) {
    if (!X || !Y || !T1 || !T2 || !out || n <= 0 || m <= 0 || k <= 0 || k > m || ldx < m || ldy < m || ldt1 < k ||
        ldt2 < k || ldo < k)
        return NSVD_EINVAL;
    if (out == X || out == Y) return NSVD_EINVAL;
    if (m > NY_MAXM) return NSVD_EUNSUPPORTED;
    ts_rotate2_kernel<<<nsvd_cdiv(n, RO_ROWS), NY_THREADS, 0, (hipStream_t)stream>>>(
        X, (size_t)ldx, Y, (size_t)ldy, n, m, T1, ldt1, T2, ldt2, k, out, (size_t)ldo);
    NSVD_CHECK_LAUNCH();
    return 0;
}
