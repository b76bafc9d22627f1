// SpINx on the matrix-free kernel operators: the one piece of reference methods/spinx.py that is SpINx's own. Its whole
// loss (spinx.py:13-23 SpINxLossFunction.forward, :92-99 SpINx._compute_loss) is a function of four L x L moment
// matrices, so the step shares everything tall with the other methods (nsvd_tsgram_f64 / nsvd_tsgram3_f64 for the
// moments, nsvd_ts_rotate2 / nsvd_ts_rotate for the cotangents, nsvd_model_backward):
//   nsvd_spinx_solve   forward AND reverse mode through cholesky(sigma + 1e-3 I), its inverse and the L + 1 losses, plus
//                      the moving average of sigma and its own factorisation, in ONE workgroup, float64.
// With A = cholesky(sigma + 1e-3 I)^-1 (rows a_l), lambda_l = a_l^T Gpk a_l, qk_l = a_l^T Gkk a_l, qp_l = a_l^T Gpp a_l:
//   losses = [sum_l tw_l lambda_l | r_l = qk_l - lambda_l^2 (2 - qp_l)],  loss = sum_k w_k losses_k / L
//   u_l = w_l / L, v_l = w_l lambda_l^2 / L, c_l = (w_0 tw_l - 2 w_l lambda_l (2 - qp_l)) / L
//   Gkk_bar = A^T diag(u) A, Gpp_bar = A^T diag(v) A, Gpk_bar = A^T diag(c) A
//   A_bar row l = u_l (Gkk + Gkk^T) a_l + v_l (Gpp + Gpp^T) a_l + c_l (Gpk + Gpk^T) a_l     (lower triangle)
//   C_bar = -A^T A_bar A^T, and C^T C_bar = -A_bar A^T since C^T A^T = I, so
//   sigma_bar = sym(A^T Phi(-A_bar A^T) A), Phi = lower triangle with the diagonal halved.
// LDS holds four L x (L | 1) float64 matrices (133 KB at L = 64, of the CU's 160 KiB). The four Grams stay in global
// memory (32 KB each at L = 64: L2); once the factor is inverted its matrix is free, and each Gram passes through it
// once as g_scale (G + G^T), which serves both the diagonal a_l^T G a_l and row l of A_bar. The two factorisations (the
// batch matrix and the moving average) share one column loop and its barriers. Nothing non-finite is ever stored: the
// state's factor is checked and leaves early, everything else after every output is known to be finite, and a failure
// writes zeros over all of them. Every loop has a trip count bounded by L; nothing waits on a data-dependent flag; no
// atomics.
#include "nsvd_kernels.h"

namespace {

constexpr int SX_THREADS = 256;
constexpr int SX_MAXL = 64;

__host__ __device__ inline size_t sx_lds_bytes(int L) { return ((size_t)4 * L * (L | 1) + 8 * L) * sizeof(double); }

__device__ __forceinline__ bool sx_finite(double v) { return fabs(v) < 1.7e308; }

// M and (two: also) N, each (L, ld) with the lower triangle given: their lower Cholesky factors in place below the
// diagonal, the diagonals in dgM / dgN; the upper triangles are never read. The two factorisations are independent and
// share the column loop, so the second costs no barrier of its own. Returns false (in every thread) at the first
// non-positive or non-finite pivot of either.
__device__ bool sx_cholesky2(double* M, double* dgM, double* N, double* dgN, bool two, int L, int ld, int t) {
    bool ok = true;
    for (int j = 0; j < L; ++j) {
        // the same LDS words in every thread: the branch is uniform
        const double d = M[j * ld + j], d2 = two ? N[j * ld + j] : 1.0;
        if (!(d > 0.0) || !sx_finite(d) || !(d2 > 0.0) || !sx_finite(d2)) {
            ok = false;
            break;
        }
        const double lj = sqrt(d), inv = 1.0 / lj, lj2 = sqrt(d2), inv2 = 1.0 / lj2;
        if (t == 0) {
            dgM[j] = lj;
            dgN[j] = lj2;
        }
        for (int i = j + 1 + t; i < L; i += SX_THREADS) {
            M[i * ld + j] *= inv;
            if (two) N[i * ld + j] *= inv2;
        }
        __syncthreads();
        const int rem = L - j - 1;
        for (int e = t; e < rem * rem; e += SX_THREADS) {
            const int i = j + 1 + e / rem, c = j + 1 + e % rem;
            if (c <= i) {
                M[i * ld + c] = fma(-M[i * ld + j], M[c * ld + j], M[i * ld + c]);
                if (two) N[i * ld + c] = fma(-N[i * ld + j], N[c * ld + j], N[i * ld + c]);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    return ok;
}

struct SpinxArgs {
    const double *S, *Gpp, *Gpk, *Gkk;  // raw Grams (L, L); S may be Gpp
    const double *w, *tw;               // (L + 1), (L) or null
    double s_scale, g_scale, decay;
    float *sigma_avg, *chol;            // state (touched only when update_state)
    double *out64, *Ts, *Tpp, *Tkp, *Tpk, *Tkk;
    int* status;
    int L, update_state;
};

__global__ void __launch_bounds__(SX_THREADS) spinx_solve_kernel(SpinxArgs P) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, L = P.L, ld = L | 1, LL = L * L;
    double* M0 = sm;            // sigma + 1e-3 I and its factor; then g_scale (G + G^T) of one Gram at a time; then W A
    double* M1 = M0 + L * ld;   // A = chol^-1 (zero above the diagonal)
    double* M2 = M1 + L * ld;   // A (Gpk + Gpk^T), then A_bar (lower triangle); at the end the losses
    double* M3 = M2 + L * ld;   // the state's matrix and factor; A (G + G^T) of Gpp, Gkk; W = Phi(-A_bar A^T); X = A^T W A
    double* dg = M3 + L * ld;   // (L) Cholesky diagonal of the batch sigma
    double* dg2 = dg + L;       // (L) Cholesky diagonal of the state
    double* lam = dg2 + L;      // (L) eigvals
    double* qk = lam + L;       // (L)
    double* qp = qk + L;        // (L)
    double* cu = qp + L;        // (L) u
    double* cv = cu + L;        // (L) v
    double* cc = cv + L;        // (L) c
    const double gs = P.g_scale;
    const bool upd = P.update_state != 0;
    int bits = 0;

    // sigma + 1e-3 I, and the state: sigma_avg <- (1 - decay) sigma_avg + decay sigma (a non-finite element is not stored)
    int nonfinite = 0;
    for (int e = t; e < LL; e += SX_THREADS) {
        const int i = e / L, j = e - i * L;
        const double s = P.s_scale * P.S[e];
        if (!sx_finite(s)) nonfinite = 1;
        M0[i * ld + j] = s + (i == j ? 1e-3 : 0.0);
        M1[i * ld + j] = 0.0;
        if (upd) {
            const double v = (1.0 - P.decay) * (double)P.sigma_avg[e] + P.decay * s;
            if (sx_finite(v)) P.sigma_avg[e] = (float)v;
            else nonfinite = 1;
            M3[i * ld + j] = v + (i == j ? 1e-3 : 0.0);
        }
    }
    if (t <= L && !sx_finite(P.w[t])) nonfinite = 1;
    if (P.tw && t < L && !sx_finite(P.tw[t])) nonfinite = 1;
    if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
    if (!bits && !sx_cholesky2(M0, dg, M3, dg2, upd, L, ld, t)) bits |= NSVD_RITZ_BAD_PIVOT;

    if (!bits) {
        // the state's factor leaves now (M3 is needed below); a later failure writes zeros over it, element e from the
        // thread that stores it here
        if (upd) {
            nonfinite = 0;
            for (int e = t; e < LL; e += SX_THREADS) {
                const int i = e / L, j = e - i * L;
                if (j < i && !sx_finite(M3[i * ld + j])) nonfinite = 1;
            }
            if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
            else
                for (int e = t; e < LL; e += SX_THREADS) {
                    const int i = e / L, j = e - i * L;
                    P.chol[e] = j < i ? (float)M3[i * ld + j] : (j == i ? (float)dg2[i] : 0.f);
                }
        }
    }
    if (!bits) {
        // column t of the inverse by forward substitution
        if (t < L) {
            for (int i = t; i < L; ++i) {
                double s = i == t ? 1.0 : 0.0;
                for (int k = t; k < i; ++k) s = fma(-M0[i * ld + k], M1[k * ld + t], s);
                M1[i * ld + t] = s / dg[i];
            }
        }
        __syncthreads();
        // M0 = g_scale (G + G^T): symmetric, so the products below walk it by rows of consecutive lanes
        auto stage = [&](const double* G) {
            for (int e = t; e < LL; e += SX_THREADS) {
                const int i = e / L, j = e - i * L;
                M0[i * ld + j] = gs * (G[e] + G[j * L + i]);
            }
            __syncthreads();
        };
        // element (l, j <= l) of A (G + G^T): with it row l of A_bar is coef_l times this row, and a_l^T G a_l half its
        // product with a_l
        auto hrow = [&](int l, int j) {
            double s = 0.0;
            for (int k = 0; k <= l; ++k) s = fma(M0[k * ld + j], M1[l * ld + k], s);
            return s;
        };
        auto rowdot = [&](const double* src, double* q) {
            if (t < L) {
                double s = 0.0;
                for (int j = 0; j <= t; ++j) s = fma(src[t * ld + j], M1[t * ld + j], s);
                q[t] = 0.5 * s;
            }
            __syncthreads();
        };
        stage(P.Gpk);
        for (int e = t; e < LL; e += SX_THREADS) {
            const int l = e / L, j = e - l * L;
            M2[l * ld + j] = j <= l ? hrow(l, j) : 0.0;
        }
        __syncthreads();
        rowdot(M2, lam);
        stage(P.Gpp);
        for (int e = t; e < LL; e += SX_THREADS) {
            const int l = e / L, j = e - l * L;
            M3[l * ld + j] = j <= l ? hrow(l, j) : 0.0;
        }
        __syncthreads();
        rowdot(M3, qp);
        if (t < L) {
            const double w0 = P.w[0], wl = P.w[1 + t], twl = P.tw ? P.tw[t] : 1.0, iL = 1.0 / (double)L;
            cu[t] = wl * iL;
            cv[t] = wl * lam[t] * lam[t] * iL;
            cc[t] = (w0 * twl - 2.0 * wl * lam[t] * (2.0 - qp[t])) * iL;
        }
        __syncthreads();
        stage(P.Gkk);
        // A_bar = diag(c) A (Gpk + Gpk^T) + diag(v) A (Gpp + Gpp^T) + diag(u) A (Gkk + Gkk^T); element e stays with its thread
        for (int e = t; e < LL; e += SX_THREADS) {
            const int l = e / L, j = e - l * L;
            const double h = j <= l ? hrow(l, j) : 0.0;
            M2[l * ld + j] = cc[l] * M2[l * ld + j] + cv[l] * M3[l * ld + j] + cu[l] * h;
            M3[l * ld + j] = h;
        }
        __syncthreads();
        rowdot(M3, qk);
        // W = Phi(-A_bar A^T)
        for (int e = t; e < LL; e += SX_THREADS) {
            const int i = e / L, j = e - i * L;
            double s = 0.0;
            if (j <= i) {
                for (int k = 0; k <= j; ++k) s = fma(M2[i * ld + k], M1[j * ld + k], s);
                s = i == j ? -0.5 * s : -s;
            }
            M3[i * ld + j] = s;
        }
        __syncthreads();
        // Y = W A, X = A^T Y
        for (int e = t; e < LL; e += SX_THREADS) {
            const int i = e / L, j = e - i * L;
            double s = 0.0;
            for (int k = j; k <= i; ++k) s = fma(M3[i * ld + k], M1[k * ld + j], s);
            M0[i * ld + j] = s;
        }
        __syncthreads();
        for (int e = t; e < LL; e += SX_THREADS) {
            const int i = e / L, j = e - i * L;
            double s = 0.0;
            for (int k = i; k < L; ++k) s = fma(M1[k * ld + i], M0[k * ld + j], s);
            M3[i * ld + j] = s;
        }
        __syncthreads();
    }

    // element (i, j) of A^T diag(coef) A
    auto gbar = [&](const double* coef, int i, int j) {
        double s = 0.0;
        for (int l = max(i, j); l < L; ++l) s = fma(coef[l] * M1[l * ld + i], M1[l * ld + j], s);
        return s;
    };
    if (!bits) {
        nonfinite = 0;
        for (int e = t; e < LL; e += SX_THREADS) {
            const int i = e / L, j = e - i * L;
            const double ts = (M3[i * ld + j] + M3[j * ld + i]) * P.s_scale;
            if (!sx_finite(ts) || !sx_finite(2.0 * gs * gbar(cv, i, j) + ts) || !sx_finite(2.0 * gs * gbar(cu, i, j)) ||
                !sx_finite(gs * gbar(cc, i, j)))
                nonfinite = 1;
        }
        if (t < L && (!sx_finite(lam[t]) || !sx_finite(qk[t]) || !sx_finite(qp[t]) ||
                      !sx_finite((qk[t] - lam[t] * lam[t] * (2.0 - qp[t])) * P.w[1 + t])))
            nonfinite = 1;
        if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
    }
    double* losses = M2;  // (L + 1), A_bar is spent
    if (!bits) {
        if (t < L) losses[1 + t] = qk[t] - lam[t] * lam[t] * (2.0 - qp[t]);
        if (t == 0) {
            double s = 0.0;
            for (int k = 0; k < L; ++k) s = fma(P.tw ? P.tw[k] : 1.0, lam[k], s);
            losses[0] = s;
        }
        __syncthreads();
        nonfinite = 0;
        if (t == 0) {
            double s = 0.0;
            for (int k = 0; k <= L; ++k) s = fma(losses[k], P.w[k], s);
            s /= (double)L;
            if (sx_finite(s) && sx_finite(losses[0])) P.out64[0] = s;
            else nonfinite = 1;
        }
        if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
    }
    if (bits) {
        // nothing non-finite is stored: every output of the failed solve is zero
        for (int e = t; e < LL; e += SX_THREADS) {
            P.Ts[e] = P.Tpp[e] = P.Tkp[e] = P.Tpk[e] = P.Tkk[e] = 0.0;
            if (upd) P.chol[e] = 0.f;
        }
        for (int e = t; e < 2 * L + 2; e += SX_THREADS) P.out64[e] = 0.0;
        if (t == 0) *P.status = *P.status | bits;
        return;
    }
    for (int e = t; e < LL; e += SX_THREADS) {
        const int i = e / L, j = e - i * L;
        const double ts = (M3[i * ld + j] + M3[j * ld + i]) * P.s_scale;
        const double gpk = gs * gbar(cc, i, j);
        P.Ts[e] = ts;
        P.Tpp[e] = 2.0 * gs * gbar(cv, i, j) + ts;
        P.Tkk[e] = 2.0 * gs * gbar(cu, i, j);
        P.Tpk[e] = gpk;
        P.Tkp[j * L + i] = gpk;
    }
    if (t <= L) P.out64[1 + t] = losses[t];
    if (t < L) P.out64[L + 2 + t] = lam[t];
}

}  // namespace

extern "C" int nsvd_spinx_solve(const double* S_raw, double s_scale, const double* Gpp_raw, const double* Gpk_raw,
                                const double* Gkk_raw, double g_scale, int L, const double* w, const double* trace_w,
                                double decay, int update_state, float* sigma_avg, float* chol, double* out64, double* T_s,
                                double* T_pp, double* T_kp, double* T_pk, double* T_kk, int* status, void* stream) {
    if (!S_raw || !Gpp_raw || !Gpk_raw || !Gkk_raw || !w || !out64 || !T_s || !T_pp || !T_kp || !T_pk || !T_kk || !status)
        return NSVD_EINVAL;
    if (update_state && (!sigma_avg || !chol)) return NSVD_EINVAL;
    if (L < 2) return NSVD_EINVAL;
    if (L > SX_MAXL) return NSVD_EUNSUPPORTED;
    if (!(decay >= 0.0 && decay <= 1.0)) return NSVD_EINVAL;
    SpinxArgs P;
    P.S = S_raw; P.Gpp = Gpp_raw; P.Gpk = Gpk_raw; P.Gkk = Gkk_raw;
    P.w = w; P.tw = trace_w;
    P.s_scale = s_scale; P.g_scale = g_scale; P.decay = decay;
    P.sigma_avg = sigma_avg; P.chol = chol;
    P.out64 = out64; P.Ts = T_s; P.Tpp = T_pp; P.Tkp = T_kp; P.Tpk = T_pk; P.Tkk = T_kk;
    P.status = status;
    P.L = L; P.update_state = update_state ? 1 : 0;
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)spinx_solve_kernel}, sx_lds_bytes(SX_MAXL))) return rc;
    spinx_solve_kernel<<<1, SX_THREADS, sx_lds_bytes(L), (hipStream_t)stream>>>(P);
    NSVD_CHECK_LAUNCH();
    return 0;
}
