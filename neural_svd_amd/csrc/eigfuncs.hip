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
// Both kernels are templates over the dimension of x and the table's type: D = 2 with NsvdEigTable (the three 2-D ground
// truths, nsvd_eigfunc_*), D = 3 with NsvdEigTable3 (Hydrogen3D, 80 x 24 bytes, nsvd_eigfunc3_*). The dimension sets the
// row stride of x, the coordinates under the Gaussian weight and p_val = (2 lim)^-D; nothing else differs.
#include "nsvd_kernels.h"
#include "eig_math.h"

namespace {

constexpr int ER = 64;      // rows per workgroup
constexpr int EMAXL = 64;   // learned functions (spectrum.hip's SMAXL)

// one function at one row: the table entry decides the dimension (2 or 3 coordinates per row of x)
__device__ __forceinline__ double eig_at(const NsvdEigFn& fn, int kind, double param, const float* xr) {
    return nsvd_eig_eval(kind, param, fn.a, fn.b, fn.norm, (double)xr[0], (double)xr[1]);
}
__device__ __forceinline__ double eig_at(const NsvdEigFn3& fn, int kind, double param, const float* xr) {
    return nsvd_eig3_eval(kind, param, fn.n, fn.l, fn.m, fn.norm, (double)xr[0], (double)xr[1], (double)xr[2]);
}

template <int D, class Table>
__global__ void __launch_bounds__(256) eigfunc_eval_kernel(Table tab, int kind, double param, int Lg,
                                                           const float* __restrict__ x, size_t total,
                                                           double* __restrict__ psi) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t r = i / Lg;
    const int c = (int)(i - r * Lg);
    const auto fn = tab.fn[c];
    psi[i] = eig_at(fn, kind, param, x + D * r);
}

template <int D, class Table>
__global__ void __launch_bounds__(256) eigfunc_accumulate_kernel(Table tab, int kind, double param, int Lg,
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
        const float* xr = x + (size_t)(r0 + r) * D;
        const auto fn = tab.fn[c];
        ps[i] = eig_at(fn, kind, param, xr) * (double)inv_sqrt_val;
    }
    for (int i = threadIdx.x; i < nr * L; i += 256) {
        const int r = i / L, c = i - r * L;
        const float* xr = x + (size_t)(r0 + r) * D;
        const float sp = use_imp ? nsvd_sqrt_gauss_pdf(xr, D, sigma, log_norm) : 1.f;
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

inline int fill_table(int kind, double param, const int* qnums, int Lg, NsvdEigTable* t) {
    return nsvd_eig_table_fill(kind, param, qnums, Lg, t);
}
inline int fill_table(int kind, double param, const int* qnums, int Lg, NsvdEigTable3* t) {
    return nsvd_eig3_table_fill(kind, param, qnums, Lg, t);
}

// the two entry points of either dimension: the checks, the table (on the host, by value into the launch), one launch
template <int D, class Table>
int eval_call(int kind, double param, const int* qnums, int Lg, const float* x, int B, double* psi, void* stream) {
    if (!qnums || !x || !psi || B <= 0 || Lg <= 0) return NSVD_EINVAL;
    if (Lg > NSVD_EIG_MAX_FN) return NSVD_EUNSUPPORTED;
    Table tab = {};
    if (int rc = fill_table(kind, param, qnums, Lg, &tab)) return rc;
    const size_t total = (size_t)B * Lg;
    hipLaunchKernelGGL((eigfunc_eval_kernel<D, Table>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, tab, kind, param, Lg, x, total, psi);
    NSVD_CHECK_LAUNCH();
    return 0;
}

template <int D, class Table>
int accumulate_call(int kind, double param, const int* qnums, int Lg, const float* f, int L, const float* x, int B,
                    float sigma, int use_importance, float lim, double* gram, double* cross, double* cov,
                    void* stream) {
    if (!qnums || !f || !x || !gram || !cross || B <= 0 || L <= 0 || Lg <= 0 || !(lim > 0.f)) return NSVD_EINVAL;
    if (L > EMAXL || Lg > NSVD_EIG_MAX_FN) return NSVD_EUNSUPPORTED;
    // the three-way rule of nsvd_spectrum_accumulate: the uniform density is a constant the caller weights the rows by
    if (use_importance == NSVD_IMP_UNIFORM) return NSVD_EUNSUPPORTED;
    if (use_importance != NSVD_IMP_NONE && use_importance != NSVD_IMP_GAUSSIAN) return NSVD_EINVAL;
    if (use_importance == NSVD_IMP_GAUSSIAN && !(sigma > 0.f)) return NSVD_EINVAL;
    Table tab = {};
    if (int rc = fill_table(kind, param, qnums, Lg, &tab)) return rc;
    // p_val and its square root as spectrum.hip forms them (a float32 tensor in the reference, main_pde.py:130)
    const float pval = (float)(1.0 / pow(2.0 * (double)lim, (double)D));
    const float inv_sqrt_val = 1.f / sqrtf(pval);
    const size_t lds = (size_t)ER * Lg * sizeof(double) + (size_t)ER * L * sizeof(float);
    hipLaunchKernelGGL((eigfunc_accumulate_kernel<D, Table>), dim3(nsvd_cdiv(B, ER)), dim3(256), lds,
                       (hipStream_t)stream, tab, kind, param, Lg, f, L, x, B, sigma,
                       nsvd_gauss_log_norm(D, use_importance ? sigma : 1.f), use_importance, inv_sqrt_val, gram, cross,
                       cov);
    NSVD_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int nsvd_eigfunc_eval(int kind, double param, const int* qnums, int Lg, const float* x, int B, double* psi,
                                 void* stream) {
    return eval_call<2, NsvdEigTable>(kind, param, qnums, Lg, x, B, psi, stream);
}

extern "C" int nsvd_eigfunc_accumulate_f64(int kind, double param, const int* qnums, int Lg, const float* f, int L,
                                           const float* x, int B, float sigma, int use_importance, float lim,
                                           double* gram, double* cross, double* cov, void* stream) {
    return accumulate_call<2, NsvdEigTable>(kind, param, qnums, Lg, f, L, x, B, sigma, use_importance, lim, gram, cross,
                                            cov, stream);
}

extern "C" int nsvd_eigfunc3_eval(int kind, double param, const int* qnums, int Lg, const float* x, int B, double* psi,
                                  void* stream) {
    return eval_call<3, NsvdEigTable3>(kind, param, qnums, Lg, x, B, psi, stream);
}

extern "C" int nsvd_eigfunc3_accumulate_f64(int kind, double param, const int* qnums, int Lg, const float* f, int L,
                                            const float* x, int B, float sigma, int use_importance, float lim,
                                            double* gram, double* cross, double* cov, void* stream) {
    return accumulate_call<3, NsvdEigTable3>(kind, param, qnums, Lg, f, L, x, B, sigma, use_importance, lim, gram,
                                             cross, cov, stream);
}
