// Eigenfunction accuracy against the analytic ground truths (reference examples/operator/pde/schrodinger/
// ground_truths.py: eigfunc; examples/linalg.py: subspace_distance, rotate, procrustes work on the (n, L) blocks this
// file never stores). Per chunk of the validation grid:
//   psi (B, Lg) float64 = the Lg ground-truth functions at x (eig_math.h), psi_w = psi / sqrt(p_val),
//   phi = nan_to_num(w f), w = sqrt(p_train(x)) / sqrt(p_val): spectrum.hip's phi, bit for bit,
//   gram += psi_w^T psi_w, cross += psi_w^T phi, cov += phi^T phi   - float64 products and sums.
// One workgroup per ER = 64 rows: one thread per (row, function) evaluates psi into LDS (doubles) beside the weighted phi
// (floats, as spectrum.hip keeps them), then one thread per output element sums over the rows and issues ONE atomic:
// spectrum.hip's contract (float64 atomic += across workgroups, the order of the sum not fixed). 64 rows x (80 doubles +
// 64 floats) = 57,344 bytes: under the 64 KB every kernel gets without an opt-in. The table of functions (quantum
// numbers and float64 normalisations, at most 80 x 16 bytes) travels BY VALUE in the launch arguments: a call
// allocates nothing, copies nothing and does not synchronise.
#include "nsvd_kernels.h"
#include "eig_math.h"

namespace {

constexpr int ER = 64;      // rows per workgroup
constexpr int EMAXL = 64;   // learned functions (spectrum.hip's SMAXL)

__global__ void __launch_bounds__(256) eigfunc_eval_kernel(NsvdEigTable tab, int kind, double param, int Lg,
                                                           const float* __restrict__ x, size_t total,
                                                           double* __restrict__ psi) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t r = i / Lg;
    const int c = (int)(i - r * Lg);
    const NsvdEigFn fn = tab.fn[c];
    psi[i] = nsvd_eig_eval(kind, param, fn.a, fn.b, fn.norm, (double)x[2 * r], (double)x[2 * r + 1]);
}

__global__ void __launch_bounds__(256) eigfunc_accumulate_kernel(NsvdEigTable tab, int kind, double param, int Lg,
                                                                 const float* __restrict__ f, int L,
                                                                 const float* __restrict__ x, int B, float sigma,
                                                                 float log_norm, int use_imp, float inv_sqrt_val,
                                                                 double* __restrict__ gram, double* __restrict__ cross,
                                                                 double* __restrict__ cov) {
    extern __shared__ __attribute__((aligned(16))) double esm[];  // psi_w[ER][Lg] doubles, phi[ER][L] floats
    double* ps = esm;
    float* ph = (float*)(esm + ER * Lg);
    const int r0 = blockIdx.x * ER;
    const int nr = min(ER, B - r0);
    for (int i = threadIdx.x; i < nr * Lg; i += 256) {
        const int r = i / Lg, c = i - r * Lg;
        const float* xr = x + (size_t)(r0 + r) * 2;
        const NsvdEigFn fn = tab.fn[c];
        ps[i] = nsvd_eig_eval(kind, param, fn.a, fn.b, fn.norm, (double)xr[0], (double)xr[1]) * (double)inv_sqrt_val;
    }
    for (int i = threadIdx.x; i < nr * L; i += 256) {
        const int r = i / L, c = i - r * L;
        const float* xr = x + (size_t)(r0 + r) * 2;
        const float sp = use_imp ? nsvd_sqrt_gauss_pdf(xr, 2, sigma, log_norm) : 1.f;
        const float w = sp * inv_sqrt_val;
        ph[i] = nsvd_nan_to_num(w * f[(size_t)(r0 + r) * L + c]);
    }
    __syncthreads();
    for (int o = threadIdx.x; o < Lg * Lg; o += 256) {
        const int i = o / Lg, j = o - i * Lg;
        double s = 0;
        for (int r = 0; r < nr; ++r) s = fma(ps[r * Lg + i], ps[r * Lg + j], s);
        atomicAdd(&gram[o], s);
    }
    for (int o = threadIdx.x; o < Lg * L; o += 256) {
        const int i = o / L, j = o - i * L;
        double s = 0;
        for (int r = 0; r < nr; ++r) s = fma(ps[r * Lg + i], (double)ph[r * L + j], s);
        atomicAdd(&cross[o], s);
    }
    if (!cov) return;
    for (int o = threadIdx.x; o < L * L; o += 256) {
        const int i = o / L, j = o - i * L;
        double s = 0;
        for (int r = 0; r < nr; ++r) s = fma((double)ph[r * L + i], (double)ph[r * L + j], s);
        atomicAdd(&cov[o], s);
    }
}

}  // namespace

extern "C" int nsvd_eigfunc_eval(int kind, double param, const int* qnums, int Lg, const float* x, int B, double* psi,
                                 void* stream) {
    if (!qnums || !x || !psi || B <= 0 || Lg <= 0) return NSVD_EINVAL;
    if (Lg > NSVD_EIG_MAX_FN) return NSVD_EUNSUPPORTED;
    NsvdEigTable tab = {};
    if (int rc = nsvd_eig_table_fill(kind, param, qnums, Lg, &tab)) return rc;
    const size_t total = (size_t)B * Lg;
    hipLaunchKernelGGL(eigfunc_eval_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab,
                       kind, param, Lg, x, total, psi);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_eigfunc_accumulate_f64(int kind, double param, const int* qnums, int Lg, const float* f, int L,
                                           const float* x, int B, float sigma, int use_importance, float lim,
                                           double* gram, double* cross, double* cov, void* stream) {
    if (!qnums || !f || !x || !gram || !cross || B <= 0 || L <= 0 || Lg <= 0 || !(lim > 0.f)) return NSVD_EINVAL;
    if (L > EMAXL || Lg > NSVD_EIG_MAX_FN) return NSVD_EUNSUPPORTED;
    // the three-way rule of nsvd_spectrum_accumulate: the uniform density is a constant the caller weights the rows by
    if (use_importance == NSVD_IMP_UNIFORM) return NSVD_EUNSUPPORTED;
    if (use_importance != NSVD_IMP_NONE && use_importance != NSVD_IMP_GAUSSIAN) return NSVD_EINVAL;
    if (use_importance == NSVD_IMP_GAUSSIAN && !(sigma > 0.f)) return NSVD_EINVAL;
    NsvdEigTable tab = {};
    if (int rc = nsvd_eig_table_fill(kind, param, qnums, Lg, &tab)) return rc;
    // p_val and its square root as spectrum.hip forms them (a float32 tensor in the reference, main_pde.py:130), D = 2
    const float pval = (float)(1.0 / pow(2.0 * (double)lim, 2.0));
    const float inv_sqrt_val = 1.f / sqrtf(pval);
    const size_t lds = (size_t)ER * Lg * sizeof(double) + (size_t)ER * L * sizeof(float);
    hipLaunchKernelGGL(eigfunc_accumulate_kernel, dim3(nsvd_cdiv(B, ER)), dim3(256), lds, (hipStream_t)stream, tab, kind,
                       param, Lg, f, L, x, B, sigma, nsvd_gauss_log_norm(2, use_importance ? sigma : 1.f), use_importance,
                       inv_sqrt_val, gram, cross, cov);
    NSVD_CHECK_LAUNCH();
    return 0;
}
