// The small dense work of a TWO-SIDED block iteration on two tall-skinny bases: what the truncated SVD of the empirical
// cross operator C = k(xs, ys) / sqrt(n_x n_y) (neural_svd_amd/nystrom_svd.py) needs beside the two-sided matrix-free
// products of rbf_apply_pair.hip / dot_apply_pair.hip, which return P = C V and R = C^T U in one pass:
//   nsvd_tsgram3_f64         XtX = X^T X, XtY = X^T Y, YtY = Y^T Y of two (n, m) float32 blocks in ONE pass: each row tile
//                            of X and Y is staged once and feeds all three float64 accumulations (nystrom.hip's
//                            nsvd_tsgram_f64 needs two calls = four launches for the same three matrices). The kernels
//                            are ts_dense.h's: the <true, true, true> instance of nsvd_tsgram_f64's, three slots a slice
//   nsvd_svd_ritz_step_f64   the m x m solve of one iteration in ONE workgroup, float64, matrices in LDS:
//                            H = (PtU^T + RtV) / 2 = A diag(sigma) B^T (one-sided Jacobi on the columns of H, round-robin
//                            parallel ordering), Mp = B^T Sp B, Mr = A^T Sr A, the two residuals in their full
//                            three-term form, Tu = B chol(Mp)^-1, Tv = A chol(Mr)^-1
// m <= 80 throughout (ts_dense.h's limits, shared with nystrom.hip, whose nsvd_ts_rotate applies Tu and Tv). Every
// device loop has a trip count bounded by an argument or a constant; nothing waits on a data-dependent flag. No atomics:
// the row slices of the Gram are reduced in slice order by a second launch, so every result is bit-reproducible.
#include "ts_dense.h"

namespace {

constexpr int SV_MAX_THREADS = 512, SV_WIDE_M = 32;  // the small step runs 512 threads above m = 32, 256 up to it
constexpr int SV_SWEEPS = 40;   // one-sided Jacobi sweep cap (float64, m <= 80: at most 19 sweeps on graded spectra)

// ---- the m x m solve ------------------------------------------------------------------------------------------------
// LDS: three (m, ld) float64 matrices, ld = m | 1 (odd: a column walk touches every bank pair once) - 155 KB of the
// 160 KB at m = 80, so the kernel works in phases and the six inputs are loaded when their phase needs them:
//   1  Jacobi       B0 = G (starts as H, ends as A diag(sigma)), B1 = the accumulated right rotations
//   2  sort         B2 = A, then B0 = B (sigma descending, ties by ascending index); B1 is free from here on
//   3  four diagonals diag(X^T M Y), M = Hl, Hr, Cu, Cv loaded into B1 in turn and replaced IN PLACE by M Y (each
//      thread holds its 5 x 5 tile of the product in registers across the barrier that ends the reads of M)
//   4  left basis   B1 = Sp -> Sp B -> Mp = B^T (Sp B), both in place in the same way; chol(Mp) in place; Tu = B R^-1 in
//                   place in B0
//   5  right basis  the same with Sr and A in B2 -> Tv
constexpr double SV_BIG = 1.7e308;

__host__ __device__ inline size_t svd_lds_bytes(int m) {
    const int ld = m | 1, mp = (m + 1) & ~1;
    return ((size_t)3 * m * ld + 2 * m + mp) * sizeof(double) + (size_t)(mp + m) * sizeof(int);
}

// acc = (TL ? L^T : L) R for the 5 x 5 tile (ti + 16 a, tj + 16 b) of the thread; blocks beyond m are skipped (uniform
// per half wave) and indices are clamped, so nothing outside the (m, ld) matrices is read
template <bool TL>
__device__ __forceinline__ void sv_tile_mm(const double* L, const double* R, int m, int ld, double (&acc)[NY_CB][NY_CB]) {
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15, nb = (m + 15) >> 4;
    if (threadIdx.x >= NY_THREADS) return;  // (the tiles are the first 256 threads'; the barriers are the caller's)
    int ia[NY_CB], jb[NY_CB];
#pragma unroll
    for (int a = 0; a < NY_CB; ++a) {
        ia[a] = min(ti + 16 * a, m - 1);
        jb[a] = min(tj + 16 * a, m - 1);
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) acc[a][b] = 0.0;
    }
    for (int k = 0; k < m; ++k) {
        double la[NY_CB], rb[NY_CB];
#pragma unroll
        for (int a = 0; a < NY_CB; ++a)
            if (a < nb) {
                la[a] = TL ? L[k * ld + ia[a]] : L[ia[a] * ld + k];
                rb[a] = R[k * ld + jb[a]];
            }
#pragma unroll
        for (int a = 0; a < NY_CB; ++a)
#pragma unroll
            for (int b = 0; b < NY_CB; ++b)
                if (a < nb && b < nb) acc[a][b] = fma(la[a], rb[b], acc[a][b]);
    }
}

__device__ __forceinline__ void sv_tile_store(double* D, int m, int ld, const double (&acc)[NY_CB][NY_CB]) {
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    if (threadIdx.x >= NY_THREADS) return;
#pragma unroll
    for (int a = 0; a < NY_CB; ++a)
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) {
            const int i = ti + 16 * a, j = tj + 16 * b;
            if (i < m && j < m) D[i * ld + j] = acc[a][b];
        }
}

// Bw = M (row-major global, transposed on the way in when TR; null: the identity); leaves Bw = M Y and returns, in
// thread k < m, (X^T M Y)_kk. Enters and leaves behind a barrier.
template <int NT, bool TR>
__device__ __forceinline__ double sv_diag(const double* M, double* Bw, const double* X, const double* Y, int m, int ld) {
    const int t = threadIdx.x, mm = m * m;
    for (int e = t; e < mm; e += NT) {
        const int i = e / m, j = e - i * m;
        Bw[i * ld + j] = M ? (TR ? M[j * m + i] : M[e]) : (i == j ? 1.0 : 0.0);
    }
    __syncthreads();
    double acc[NY_CB][NY_CB];
    sv_tile_mm<false>(Bw, Y, m, ld, acc);
    __syncthreads();
    sv_tile_store(Bw, m, ld, acc);
    __syncthreads();
    double d = 0.0;
    if (t < m)
        for (int i = 0; i < m; ++i) d = fma(X[i * ld + t], Bw[i * ld + t], d);
    __syncthreads();
    return d;
}

// Bw = S (global) -> M = X^T S X in place; R = chol(M) (upper) in the upper triangle of Bw with R_jj in dg;
// X <- X R^-1 in place, zero from the first bad pivot on; T (global) = X, nothing non-finite stored. Thread k < m gets
// M_kk in mkk. Returns nonzero (uniformly) when a pivot was bad. Enters and leaves behind a barrier.
template <int NT>
__device__ __forceinline__ int sv_basis(const double* S, double* Bw, double* X, double* dg, int m, int ld, double* T,
                                        double& mkk) {
    const int t = threadIdx.x, mm = m * m;
    for (int e = t; e < mm; e += NT) {
        const int i = e / m, j = e - i * m;
        Bw[i * ld + j] = S[e];
    }
    __syncthreads();
    double acc[NY_CB][NY_CB];
    sv_tile_mm<false>(Bw, X, m, ld, acc);
    __syncthreads();
    sv_tile_store(Bw, m, ld, acc);
    __syncthreads();
    sv_tile_mm<true>(X, Bw, m, ld, acc);
    __syncthreads();
    sv_tile_store(Bw, m, ld, acc);
    __syncthreads();
    mkk = t < m ? Bw[t * ld + t] : 0.0;
    int bad = m;
    for (int j = 0; j < m; ++j) {
        const double d = Bw[j * ld + j];  // the same LDS word in every thread: the branch is uniform
        if (!(d > 0.0) || !(d < SV_BIG)) {
            bad = j;
            break;
        }
        const double rj = sqrt(d), inv = 1.0 / rj;
        if (t == 0) dg[j] = rj;
        for (int c = j + 1 + t; c < m; c += NT) Bw[j * ld + c] *= inv;
        __syncthreads();
        const int rem = m - j - 1;
        for (int e = t; e < rem * rem; e += NT) {
            const int i = j + 1 + e / rem, c = j + 1 + e % rem;
            if (c >= i) Bw[i * ld + c] = fma(-Bw[j * ld + i], Bw[j * ld + c], Bw[i * ld + c]);
        }
        __syncthreads();
    }
    __syncthreads();
    // forward substitution along each row of X (one thread per row)
    if (t < m) {
        double* row = X + t * ld;
        for (int j = 0; j < m; ++j) {
            if (j >= bad) {
                row[j] = 0.0;
                continue;
            }
            double s = row[j];
            for (int k = 0; k < j; ++k) s = fma(-row[k], Bw[k * ld + j], s);
            row[j] = s / dg[j];
        }
    }
    __syncthreads();
    int nonfinite = 0;
    for (int e = t; e < mm; e += NT) {
        const int i = e / m, j = e - i * m;
        double v = X[i * ld + j];
        if (!(fabs(v) < SV_BIG)) {  // (overflow behind a tiny positive pivot, or NaN)
            v = 0.0;
            nonfinite = 1;
        }
        T[e] = v;
    }
    return __syncthreads_or(nonfinite) | (bad < m ? 1 : 0);
}

__device__ __forceinline__ double sv_finite(double v, int& nonfinite) {
    if (fabs(v) < SV_BIG) return v;
    nonfinite = 1;
    return 0.0;
}

template <int NT>
__global__ void __launch_bounds__(NT) svd_ritz_step_kernel(const double* __restrict__ PtU,
                                                                   const double* __restrict__ RtV,
                                                                   const double* __restrict__ Sp,
                                                                   const double* __restrict__ Sr,
                                                                   const double* __restrict__ Cu,
                                                                   const double* __restrict__ Cv, int m,
                                                                   double* __restrict__ sigma, double* __restrict__ resid_l,
                                                                   double* __restrict__ resid_r, double* __restrict__ A,
                                                                   double* __restrict__ B, double* __restrict__ Tu,
                                                                   double* __restrict__ Tv, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, ld = m | 1, mp = (m + 1) & ~1, np = mp >> 1, mm = m * m;
    double* B0 = sm;
    double* B1 = B0 + m * ld;
    double* B2 = B1 + m * ld;
    double* sg = B2 + m * ld;   // (m) column norms as found; reused for the Cholesky diagonals
    double* sgs = sg + m;       // (m) sorted
    double* cc = sgs + m;       // (np) rotations of a round
    double* ss = cc + np;
    int* pp = (int*)(ss + np);  // (np) pairs of a round
    int* qq = pp + np;
    int* perm = qq + np;        // (m) sorted position -> column
    int bits = 0, nonfinite = 0;

    // ---- 1: H = (PtU^T + RtV) / 2 into B0, I into B1; one-sided Jacobi on the columns of B0
    for (int e = t; e < mm; e += NT) {
        const int i = e / m, j = e - i * m;
        B0[i * ld + j] = 0.5 * (PtU[j * m + i] + RtV[e]);
        B1[i * ld + j] = i == j ? 1.0 : 0.0;
    }
    // a pair's three column products are summed by a group of gs = 4 lanes (256 threads, m <= 32) or 8 (512 threads):
    // np gs <= 320 threads; the loads of a lane's rows are independent and overlap, a wider group at small m would only
    // add dependent shuffle steps. The flat index e = k m + i of the column update advances by the workgroup size
    // NT = q256 m + r256 without a division.
    constexpr int gs = NT >> 6;
    const int pr = t / gs, lane = t % gs;
    const int q256 = NT / m, r256 = NT % m, k0 = t / m, i0 = t % m;
    bool converged = false;
    __syncthreads();
    for (int sweep = 0; sweep < SV_SWEEPS; ++sweep) {
        int rotated = 0;
        // mp - 1 rounds of the round-robin tournament, np disjoint pairs each (index m is the bye of an odd m); two
        // barriers per round: pair parameters, column update
        for (int r = 0; r < mp - 1; ++r) {
            int p = -1, q = 0;
            if (pr < np) {
                const int a = pr == 0 ? mp - 1 : (r + pr) % (mp - 1);
                const int b = pr == 0 ? r : (r - pr + mp - 1) % (mp - 1);
                q = max(a, b);
                p = q < m ? min(a, b) : -1;
            }
            double al = 0.0, be = 0.0, ga = 0.0;
            if (p >= 0) {
#pragma unroll 4
                for (int i = lane; i < m; i += gs) {
                    const double gp = B0[i * ld + p], gq = B0[i * ld + q];
                    al = fma(gp, gp, al);
                    be = fma(gq, gq, be);
                    ga = fma(gp, gq, ga);
                }
            }
#pragma unroll
            for (int o = gs >> 1; o > 0; o >>= 1) {
                al += __shfl_xor(al, o, 64);
                be += __shfl_xor(be, o, 64);
                ga += __shfl_xor(ga, o, 64);
            }
            if (lane == 0 && pr < np) {
                double c = 1.0, s = 0.0;
                bool rot = false;
                if (p >= 0 && ga * ga > 1e-30 * (al * be)) {  // |g_p . g_q| > 1e-15 |g_p| |g_q| (false for NaN)
                    // tan of the rotation angle: the smaller root of t^2 + 2 zeta t - 1 = 0, zeta = (be - al) / (2 ga),
                    // written without the division for zeta (one square root, one division, one reciprocal square
                    // root a pair: the round waits for this chain)
                    const double d = be - al, h = fabs(d) + sqrt(fma(d, d, 4.0 * ga * ga));
                    const double tt = ((d >= 0.0) == (ga >= 0.0) ? 2.0 : -2.0) * fabs(ga) / h;
                    c = rsqrt(fma(tt, tt, 1.0));
                    s = tt * c;
                    rot = true;
                    rotated = 1;
                }
                pp[pr] = rot ? p : -1;
                qq[pr] = q;
                cc[pr] = c;
                ss[pr] = s;
            }
            __syncthreads();
            // columns p, q of G and of the accumulated rotations: G <- G J, B <- B J
            for (int k = k0, i = i0; k < np;) {
                const int cp = pp[k], cq = qq[k];
                if (cp >= 0) {
                    const double c = cc[k], s = ss[k];
                    const double gp = B0[i * ld + cp], gq = B0[i * ld + cq];
                    B0[i * ld + cp] = c * gp - s * gq;
                    B0[i * ld + cq] = s * gp + c * gq;
                    const double vp = B1[i * ld + cp], vq = B1[i * ld + cq];
                    B1[i * ld + cp] = c * vp - s * vq;
                    B1[i * ld + cq] = s * vp + c * vq;
                }
                k += q256;
                i += r256;
                if (i >= m) {
                    i -= m;
                    ++k;
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) {  // a sweep without a rotation
            converged = true;
            break;
        }
    }
    if (!converged) bits |= NSVD_RITZ_SWEEP_CAP;

    // ---- 2: sigma_k = |g_k|, descending, ties by ascending index; B2 = A (a_k = g_k / sigma_k, zero when sigma_k = 0),
    // then B0 = B
    if (t < m) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(B0[i * ld + t], B0[i * ld + t], s);
        sg[t] = sqrt(s);
        perm[t] = t;
    }
    __syncthreads();
    if (t < m) {
        const double v = sg[t];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const double u = sg[j];
            rank += (u > v || (u == v && j < t)) ? 1 : 0;
        }
        if (!(v != v)) perm[rank] = t;  // (a NaN leaves the identity entry: indices stay in range)
    }
    __syncthreads();
    if (t < m) {
        const int src = min(max(perm[t], 0), m - 1);
        perm[t] = src;
        sgs[t] = sv_finite(sg[src], nonfinite);
        if (sigma) sigma[t] = sgs[t];
    }
    __syncthreads();
    for (int e = t; e < mm; e += NT) {
        const int i = e / m, j = e - i * m;
        const double s = sgs[j];
        const double v = s > 0.0 ? sv_finite(B0[i * ld + perm[j]] / s, nonfinite) : 0.0;
        B2[i * ld + j] = v;
        if (A) A[e] = v;
    }
    __syncthreads();
    for (int e = t; e < mm; e += NT) {
        const int i = e / m, j = e - i * m;
        const double v = sv_finite(B1[i * ld + perm[j]], nonfinite);
        B0[i * ld + j] = v;
        if (B) B[e] = v;
    }
    __syncthreads();

    // ---- 3: thread k keeps (A^T Hl B)_kk, (A^T Hr B)_kk, (A^T Cu A)_kk, (B^T Cv B)_kk
    const double dl = sv_diag<NT, true>(PtU, B1, B2, B0, m, ld);
    const double dr = sv_diag<NT, false>(RtV, B1, B2, B0, m, ld);
    const double cu = sv_diag<NT, false>(Cu, B1, B2, B2, m, ld);
    const double cv = sv_diag<NT, false>(Cv, B1, B0, B0, m, ld);

    // ---- 4, 5: |P b_k - sigma_k U a_k|^2 = Mp_kk - 2 sigma_k dl_k + sigma_k^2 cu_k for ANY U, A, B (and the same on
    // the right); Tu = B chol(Mp)^-1, Tv = A chol(Mr)^-1
    double mkk;
    if (sv_basis<NT>(Sp, B1, B0, sg, m, ld, Tu, mkk)) bits |= NSVD_RITZ_BAD_PIVOT;
    if (resid_l && t < m) {
        const double s = sgs[t], d = mkk - 2.0 * s * dl + s * s * cu;
        resid_l[t] = d > 0.0 ? sv_finite(sqrt(d), nonfinite) : 0.0;
    }
    if (sv_basis<NT>(Sr, B1, B2, sg, m, ld, Tv, mkk)) bits |= NSVD_RITZ_BAD_PIVOT;
    if (resid_r && t < m) {
        const double s = sgs[t], d = mkk - 2.0 * s * dr + s * s * cv;
        resid_r[t] = d > 0.0 ? sv_finite(sqrt(d), nonfinite) : 0.0;
    }
    if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
    if (t == 0 && bits) *status = *status | bits;
}

// (the 256-thread instance serves m <= 32: 26 KB, inside the default limit. A function of its own ahead of the entry
// point: the instance named first in the file comes first in the code object, and the wide one did)
int svd_ritz_lds_opt_in() {
    static NsvdLdsOptIn st;
    return nsvd_lds_opt_in(st, {(const void*)svd_ritz_step_kernel<SV_MAX_THREADS>}, svd_lds_bytes(NY_MAXM));
}

}  // namespace

extern "C" size_t nsvd_tsgram3_f64_workspace_bytes(int n, int m) { return ts_gram_workspace_bytes(n, m, 3); }

extern "C" int nsvd_tsgram3_f64(const float* X, long ldx, const float* Y, long ldy, int n, int m, double* XtX,
                                double* XtY, double* YtY, void* ws, size_t ws_bytes, void* stream) {
    if (!XtX || !XtY || !YtY) return NSVD_EINVAL;
    return ts_gram<true>(X, ldx, Y, ldy, n, m, XtX, XtY, YtY, ws, ws_bytes, stream);
}

extern "C" int nsvd_svd_ritz_step_f64(const double* PtU, const double* RtV, const double* Sp, const double* Sr,
                                      const double* Cu, const double* Cv, int m, double* sigma, double* resid_l,
                                      double* resid_r, double* A, double* B, double* Tu, double* Tv, int* status,
                                      void* stream) {
    if (!PtU || !RtV || !Sp || !Sr || !Tu || !Tv || !status || m <= 0) return NSVD_EINVAL;
    if (m > NY_MAXM) return NSVD_EUNSUPPORTED;
    if (const int rc = svd_ritz_lds_opt_in()) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (m > SV_WIDE_M)
        svd_ritz_step_kernel<SV_MAX_THREADS><<<1, SV_MAX_THREADS, svd_lds_bytes(m), s>>>(
            PtU, RtV, Sp, Sr, Cu, Cv, m, sigma, resid_l, resid_r, A, B, Tu, Tv, status);
    else
        svd_ritz_step_kernel<NY_THREADS><<<1, NY_THREADS, svd_lds_bytes(m), s>>>(
            PtU, RtV, Sp, Sr, Cu, Cv, m, sigma, resid_l, resid_r, A, B, Tu, Tv, status);
    NSVD_CHECK_LAUNCH();
    return 0;
}
