// SpIN (Spectral Inference Networks) on the matrix-free kernel operators: the two pieces of reference methods/spin.py
// that are SpIN's own, beside the moments (nsvd_tsgram_f64), the cotangent products (nsvd_ts_rotate) and the model
// backward (nsvd_model_backward) the step shares with the other methods:
//   nsvd_spin_solve     the L x L algebra of one step in ONE workgroup, float64, matrices in LDS: moving average of
//                       sigma, chol, chol^-1, Lambda, eigvals, loss, gsigma, gpi   (spin.py:33-38, 41-59, 139-148)
//   nsvd_spin_jac_step  j_new[a, c] = (2 / B1) sum_b phi[b, a] d phi_c(x_b) / d p, its moving average and
//                       grads += sum_a gsigma[a, c] j_avg[a, c]                     (spin.py:15-30, 155-167)
// The reference keeps j_avg as (L, L, *p.shape) per parameter tensor; head c of ParallelMLP depends on head c's
// parameters only, so only the (a, c, head c's slice) entries are ever non-zero. Here the state is those entries alone:
// J[a] is one parameter set ([W_0 | .. | W_n | b_0 | .. | b_n], no padding), L of them. Per (head c, layer i) the new
// contraction is the GEMM  (phi[:, a] * delta_i^c)  a_{i-1}^c^T  over the batch: the unit-seed deltas and the activations
// are recomputed into this file's own workspace by the layer kernels of the generic model path (gemm_generic.hip, fp32
// MFMA), then one kernel instance runs every (layer, head, 32 x 128 tile, block of <= 8 a's) on v_mfma_f32_32x32x2_f32,
// scales the delta operand by phi[b, a] as it leaves LDS, and applies the moving average and the gsigma reduction to the
// accumulators. The a's of a block are reduced in registers in ascending order; the blocks are added in block order
// by a second launch. No atomics: every result is bit-reproducible. Every device loop has a trip count bounded by an
// argument; nothing waits on a data-dependent flag.
#include <string.h>
#include "nsvd_kernels.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_MAXL = 64;
constexpr int SP_MAX_D = 64;
constexpr int SP_AB = 8;     // a's per block: 8 accumulators of 16 registers per wave
constexpr int SP_TM = 32;    // rows (units of layer i) per tile
constexpr int SP_TN = 128;   // columns (inputs of layer i) per tile: 32 per wave
constexpr int SP_KB = 32;    // samples per LDS chunk
constexpr int SP_LD = SP_KB + 4;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- the small solve ------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t solve_lds_bytes(int L) { return ((size_t)4 * L * (L | 1) + 2 * L) * sizeof(double); }

__device__ __forceinline__ bool sp_finite(double v) { return fabs(v) < 1.7e308; }

// sigma_raw, pi_raw: the Gram matrices as nsvd_tsgram_f64 leaves them; sigma = sigma_scale sigma_raw, pi = pi_scale pi_raw.
// out64 = [loss | eigvals (L)]. gpi_out = gpi * gpi_scale.
__global__ void __launch_bounds__(SP_THREADS) spin_solve_kernel(const double* __restrict__ sigma_raw, double sigma_scale,
                                                                const double* __restrict__ pi_raw, double pi_scale, int L,
                                                                double decay, double gpi_scale,
                                                                float* __restrict__ sigma_avg, float* __restrict__ chol,
                                                                double* __restrict__ out64, double* __restrict__ gsigma,
                                                                double* __restrict__ gpi, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int t = threadIdx.x, ld = L | 1, LL = L * L;
    double* M0 = sm;            // sigma_avg + 1e-3 I, then its lower Cholesky factor
    double* M1 = M0 + L * ld;   // chol^-1
    double* M2 = M1 + L * ld;   // pi, then Lambda, then gsigma
    double* M3 = M2 + L * ld;   // chol^-1 pi, then triu(Lambda diag(diag chol^-1))
    double* dg = M3 + L * ld;   // (L) the Cholesky diagonal
    double* ev = dg + L;        // (L) eigvals
    int bits = 0;

    // step 2: the moving average (no bias correction); a non-finite element is not stored
    int nonfinite = 0;
    for (int e = t; e < LL; e += SP_THREADS) {
        const int i = e / L, j = e - i * L;
        const double v = (1.0 - decay) * (double)sigma_avg[e] + decay * (sigma_scale * sigma_raw[e]);
        if (sp_finite(v)) sigma_avg[e] = (float)v;
        else nonfinite = 1;
        M0[i * ld + j] = v + (i == j ? 1e-3 : 0.0);
        M2[i * ld + j] = pi_scale * pi_raw[e];
        M1[i * ld + j] = 0.0;
    }
    if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
    // step 3: chol (lower, right-looking; the upper triangle is never read)
    int bad = bits ? 0 : L;
    for (int j = 0; j < bad; ++j) {
        const double d = M0[j * ld + j];  // the same LDS word in every thread: the branch is uniform
        if (!(d > 0.0) || !sp_finite(d)) {
            bad = j;
            break;
        }
        const double lj = sqrt(d), inv = 1.0 / lj;
        if (t == 0) dg[j] = lj;
        for (int i = j + 1 + t; i < L; i += SP_THREADS) M0[i * ld + j] *= inv;
        __syncthreads();
        const int rem = L - j - 1;
        for (int e = t; e < rem * rem; e += SP_THREADS) {
            const int i = j + 1 + e / rem, c = j + 1 + e % rem;
            if (c <= i) M0[i * ld + c] = fma(-M0[i * ld + j], M0[c * ld + j], M0[i * ld + c]);
        }
        __syncthreads();
    }
    if (bad < L) bits |= NSVD_RITZ_BAD_PIVOT;
    __syncthreads();
    if (!bits) {
        // the factor in full (zero above the diagonal), and column t of its inverse by forward substitution
        for (int e = t; e < LL; e += SP_THREADS) {
            const int i = e / L, j = e - i * L;
            if (j > i) M0[i * ld + j] = 0.0;
            else if (j == i) M0[i * ld + j] = dg[i];
        }
        __syncthreads();
        if (t < L) {
            for (int i = t; i < L; ++i) {
                double s = i == t ? 1.0 : 0.0;
                for (int k = t; k < i; ++k) s = fma(-M0[i * ld + k], M1[k * ld + t], s);
                M1[i * ld + t] = s / dg[i];
            }
        }
        __syncthreads();
        // step 4: Lambda = Ci pi Ci^T
        for (int e = t; e < LL; e += SP_THREADS) {
            const int i = e / L, j = e - i * L;
            double s = 0.0;
            for (int k = 0; k <= i; ++k) s = fma(M1[i * ld + k], M2[k * ld + j], s);
            M3[i * ld + j] = s;
        }
        __syncthreads();
        for (int e = t; e < LL; e += SP_THREADS) {
            const int i = e / L, j = e - i * L;
            double s = 0.0;
            for (int k = 0; k <= j; ++k) s = fma(M3[i * ld + k], M1[j * ld + k], s);
            M2[i * ld + j] = s;
        }
        __syncthreads();
        if (t < L) ev[t] = M2[t * ld + t];
        // step 5: U = triu(Lambda diag(diag Ci)); gsigma = Ci^T U
        for (int e = t; e < LL; e += SP_THREADS) {
            const int i = e / L, j = e - i * L;
            M3[i * ld + j] = j >= i ? M2[i * ld + j] * M1[j * ld + j] : 0.0;
        }
        __syncthreads();
        for (int e = t; e < LL; e += SP_THREADS) {
            const int i = e / L, j = e - i * L;
            double s = 0.0;
            for (int k = i; k < L; ++k) s = fma(M1[k * ld + i], M3[k * ld + j], s);
            M2[i * ld + j] = s;
        }
        __syncthreads();
        nonfinite = 0;
        for (int e = t; e < LL; e += SP_THREADS) {
            const int i = e / L, j = e - i * L;
            if (!sp_finite(M0[i * ld + j]) || !sp_finite(M1[i * ld + j]) || !sp_finite(M2[i * ld + j]) ||
                !sp_finite(M1[i * ld + j] * M1[i * ld + i] * gpi_scale))
                nonfinite = 1;
        }
        if (t < L && !sp_finite(ev[t])) nonfinite = 1;
        if (__syncthreads_or(nonfinite)) bits |= NSVD_RITZ_BAD_PIVOT;
    }
    if (bits) {
        // nothing non-finite is stored: every output of the failed solve is zero
        for (int e = t; e < LL; e += SP_THREADS) {
            chol[e] = 0.f;
            gsigma[e] = 0.0;
            gpi[e] = 0.0;
        }
        if (t <= L) out64[t] = 0.0;
        if (t == 0) *status = *status | bits;
        return;
    }
    for (int e = t; e < LL; e += SP_THREADS) {
        const int i = e / L, j = e - i * L;
        chol[e] = (float)M0[i * ld + j];
        gsigma[e] = M2[i * ld + j];
        gpi[e] = -M1[j * ld + i] * M1[j * ld + j] * gpi_scale;  // gpi = -Ci^T diag(diag Ci)
    }
    if (t < L) out64[1 + t] = ev[t];
    if (t == 0) {
        double s = 0.0;
        for (int k = 0; k < L; ++k) s += ev[k];
        out64[0] = s;
    }
}

// ---- the Jacobian contraction -----------------------------------------------------------------------------------------
struct SpinLayer {
    const float* act;    // a_{i-1}: (L, kin, R), or the Fourier features (kin, R) shared by the heads (act_stride 0)
    const float* delta;  // delta_i: (L, h, R)
    long act_stride, delta_stride;
    long offW, offb;     // offsets of W_i, b_i inside one parameter set of the state
    float* gW;
    float* gb;
    int h, kin, nrt, nkt, tile0;
};
struct SpinArgs {
    SpinLayer ly[NSVD_MAX_LAYERS];
    const float* phi;      // (B1, L)
    const double* gsigma;  // (L, L)
    float* J;              // (L, P)
    float* part;           // (nblocks, P)
    long P;
    int nlayers, L, B1, R, AB, nblocks;
    float omd, dec, scale;
};

// accumulator register r of lane-half hi holds row (r & 3) + 8 (r >> 2) + 4 hi of the 32-row tile, column = lane & 31
__device__ __forceinline__ int sp_acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__global__ void __launch_bounds__(SP_THREADS) spin_jac_kernel(SpinArgs A) {
    __shared__ __attribute__((aligned(16))) float dl[SP_TM][SP_LD];  // delta rows x samples
    __shared__ __attribute__((aligned(16))) float ac[SP_TN][SP_LD];  // input rows x samples
    __shared__ __attribute__((aligned(16))) float ph[SP_AB][SP_LD];  // phi[b][a0 + a], transposed
    __shared__ float bsm[SP_AB][SP_TM];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, li = lane & 31, hi = lane >> 5;
    int lyi = 0;
    for (int i = 1; i < A.nlayers; ++i)
        if ((int)blockIdx.x >= A.ly[i].tile0) lyi = i;
    const SpinLayer& Y = A.ly[lyi];
    const int idx = blockIdx.x - Y.tile0, per = Y.nrt * Y.nkt;
    const int c = idx / per, rem = idx - c * per, rt = rem / Y.nkt, kt = rem - rt * Y.nkt;
    const int r0 = rt * SP_TM, k0 = kt * SP_TN, h = Y.h, kin = Y.kin, L = A.L, B1 = A.B1;
    const size_t R = (size_t)A.R;
    const int ab = blockIdx.y, a0 = ab * A.AB, na = min(A.AB, L - a0);
    const float* dptr = Y.delta + (size_t)c * Y.delta_stride;
    const float* aptr = Y.act + (size_t)c * Y.act_stride;
    const bool wave_on = k0 + wv * 32 < kin;

    f32x16 acc[SP_AB];
#pragma unroll
    for (int a = 0; a < SP_AB; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    float bacc = 0.f;  // bias sum of (row t & 31, a0 + (t >> 5))

    // staging: thread t moves samples 4 (t & 7) .. + 3 of row t >> 3 (+ 32 j) and phi[b0 + (t >> 3)][a0 + (t & 7)]
    const int srow = t >> 3, sb4 = (t & 7) * 4, pa = t & 7;
    float4 pd, pac[4];
    float pp;
    auto masked = [&](const float* row, bool row_ok, int b) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row_ok && b < B1) {
            v = *reinterpret_cast<const float4*>(row + b);  // (rows are R >= ceil32(B1) floats: in bounds)
            if (b + 1 >= B1) v.y = 0.f;
            if (b + 2 >= B1) v.z = 0.f;
            if (b + 3 >= B1) v.w = 0.f;
        }
        return v;
    };
    auto request = [&](int ch) {
        const int b = ch * SP_KB + sb4;
        pd = masked(dptr + (size_t)(r0 + srow) * R, r0 + srow < h, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + srow + 32 * j;
            pac[j] = masked(aptr + (size_t)k * R, k < kin, b);
        }
        const int bp = ch * SP_KB + srow;
        pp = (bp < B1 && pa < na) ? A.phi[(size_t)bp * L + a0 + pa] : 0.f;
    };
    const int nchunks = (B1 + SP_KB - 1) / SP_KB;
    request(0);
    for (int ch = 0; ch < nchunks; ++ch) {
        __syncthreads();
        *reinterpret_cast<float4*>(&dl[srow][sb4]) = pd;
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(&ac[srow + 32 * j][sb4]) = pac[j];
        ph[pa][srow] = pp;
        __syncthreads();
        if (ch + 1 < nchunks) request(ch + 1);
        if (kt == 0) {
            const int br = t & 31, ba = t >> 5;
#pragma unroll
            for (int b = 0; b < SP_KB; ++b) bacc = fmaf(dl[br][b], ph[ba][b], bacc);
        }
        if (wave_on) {
#pragma unroll
            for (int q = 0; q < SP_KB / 8; ++q) {
                const int bo = q * 8 + hi * 4;
                const float4 dv = *reinterpret_cast<const float4*>(&dl[li][bo]);
                const float4 av = *reinterpret_cast<const float4*>(&ac[wv * 32 + li][bo]);
#pragma unroll
                for (int a = 0; a < SP_AB; ++a) {
                    if (a < na) {
                        const float4 pv = *reinterpret_cast<const float4*>(&ph[a][bo]);
                        acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.x * pv.x, av.x, acc[a], 0, 0, 0);
                        acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.y * pv.y, av.y, acc[a], 0, 0, 0);
                        acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.z * pv.z, av.z, acc[a], 0, 0, 0);
                        acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv.w * pv.w, av.w, acc[a], 0, 0, 0);
                    }
                }
            }
        }
    }

    // epilogue: j_avg <- (1 - decay) j_avg + decay j_new, g = sum_a gsigma[a, c] j_avg[a], a ascending
    float* part = A.part + (size_t)ab * A.P;
    if (wave_on) {
        float g[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = 0.f;
        const int col = k0 + wv * 32 + li;
#pragma unroll
        for (int a = 0; a < SP_AB; ++a) {
            if (a < na) {
                const float gs = (float)A.gsigma[(size_t)(a0 + a) * L + c];
                float* Jp = A.J + (size_t)(a0 + a) * A.P + Y.offW + (size_t)c * h * kin;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = r0 + sp_acc_row(r, hi);
                    if (row < h && col < kin) {
                        float* p = Jp + (size_t)row * kin + col;
                        const float v = A.omd * *p + A.dec * (acc[a][r] * A.scale);
                        *p = v;
                        g[r] = fmaf(gs, v, g[r]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + sp_acc_row(r, hi);
            if (row < h && col < kin) part[Y.offW + ((size_t)c * h + row) * kin + col] = g[r];
        }
    }
    if (kt == 0) {
        const int br = t & 31, ba = t >> 5;
        float v = 0.f;
        if (ba < na && r0 + br < h) {
            float* p = A.J + (size_t)(a0 + ba) * A.P + Y.offb + (size_t)c * h + r0 + br;
            v = A.omd * *p + A.dec * (bacc * A.scale);
            *p = v;
        }
        bsm[ba][br] = v;
        __syncthreads();
        if (t < SP_TM && r0 + t < h) {
            float gb = 0.f;
            for (int a = 0; a < na; ++a) gb = fmaf((float)A.gsigma[(size_t)(a0 + a) * L + c], bsm[a][t], gb);
            part[Y.offb + (size_t)c * h + r0 + t] = gb;
        }
    }
}

// grads += sum over the a-blocks, in block order
__global__ void __launch_bounds__(SP_THREADS) spin_reduce_kernel(SpinArgs A) {
    const long e = (long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (e >= A.P) return;
    float* dst = nullptr;
    for (int i = 0; i < A.nlayers; ++i) {
        const SpinLayer& Y = A.ly[i];
        const long nW = (long)A.L * Y.h * Y.kin, nb = (long)A.L * Y.h;
        if (e >= Y.offW && e < Y.offW + nW) dst = Y.gW + (e - Y.offW);
        if (e >= Y.offb && e < Y.offb + nb) dst = Y.gb + (e - Y.offb);
    }
    if (!dst) return;
    float s = 0.f;
    for (int b = 0; b < A.nblocks; ++b) s += A.part[(size_t)b * A.P + e];
    *dst += s;
}

__global__ void spin_fill_kernel(float* p, long n, float v) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) p[e] = v;
}

int spin_validate(const nsvd_model_desc* d) {
    if (!d) return NSVD_EINVAL;
    if (d->L <= 0 || d->D <= 0 || d->m <= 0) return NSVD_EINVAL;
    if (d->nlayers < 1 || d->nlayers > NSVD_MAX_LAYERS) return NSVD_EINVAL;
    for (int i = 0; i < d->nlayers; ++i)
        if (d->dims[i] <= 0) return NSVD_EINVAL;
    if (d->dims[d->nlayers - 1] != 1) return NSVD_EINVAL;
    if (d->has_exp_mask || d->box_mask != NSVD_BOX_NONE) return NSVD_EUNSUPPORTED;  // the kernel-operator models have none
    if (d->D > SP_MAX_D || d->L > SP_MAXL) return NSVD_EUNSUPPORTED;
    return 0;
}

struct SpinWs {
    float* phiT;                     // (F, R)
    float* act[NSVD_MAX_LAYERS];     // a_i, i < nlayers - 1: (L, h_i, R)
    float* delta[NSVD_MAX_LAYERS];   // delta_i: (L, h_i, R)
    float* part;                     // (nblocks, P)
    int R, nblocks, AB;
    size_t P, bytes;
};

SpinWs spin_carve(const nsvd_model_desc& d, int B1, void* base) {
    SpinWs w;
    memset(&w, 0, sizeof(w));
    w.R = nsvd_cdiv(B1, SP_KB) * SP_KB;
    w.nblocks = nsvd_cdiv(d.L, SP_AB);
    w.AB = nsvd_cdiv(d.L, w.nblocks);  // balanced blocks of at most SP_AB
    size_t P = 0;
    int kin = 2 * d.m;
    for (int i = 0; i < d.nlayers; ++i) {
        P += (size_t)d.L * d.dims[i] * kin + (size_t)d.L * d.dims[i];
        kin = d.dims[i];
    }
    w.P = P;
    NsvdArena a(base);
    w.phiT = a.take((size_t)2 * d.m * w.R);
    for (int i = 0; i + 1 < d.nlayers; ++i) w.act[i] = a.take((size_t)d.L * d.dims[i] * w.R);
    for (int i = 0; i < d.nlayers; ++i) w.delta[i] = a.take((size_t)d.L * d.dims[i] * w.R);
    w.part = a.take((size_t)w.nblocks * P);
    w.bytes = a.off;
    return w;
}

}  // namespace

extern "C" int nsvd_spin_solve(const double* sigma_raw, double sigma_scale, const double* pi_raw, double pi_scale, int L,
                               double decay, double gpi_scale, float* sigma_avg, float* chol, double* loss_eigvals,
                               double* gsigma, double* gpi_scaled, int* status, void* stream) {
    if (!sigma_raw || !pi_raw || !sigma_avg || !chol || !loss_eigvals || !gsigma || !gpi_scaled || !status)
        return NSVD_EINVAL;
    if (L < 2) return NSVD_EINVAL;
    if (L > SP_MAXL) return NSVD_EUNSUPPORTED;
    if (!(decay >= 0.0 && decay <= 1.0)) return NSVD_EINVAL;
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)spin_solve_kernel}, solve_lds_bytes(SP_MAXL)))
        return rc;
    spin_solve_kernel<<<1, SP_THREADS, solve_lds_bytes(L), (hipStream_t)stream>>>(
        sigma_raw, sigma_scale, pi_raw, pi_scale, L, decay, gpi_scale, sigma_avg, chol, loss_eigvals, gsigma, gpi_scaled,
        status);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nsvd_spin_state_floats(const nsvd_model_desc* desc) {
    if (spin_validate(desc) != 0) return 0;
    return spin_carve(*desc, 32, nullptr).P;
}

extern "C" size_t nsvd_spin_jac_workspace_bytes(const nsvd_model_desc* desc, int B1) {
    if (spin_validate(desc) != 0 || B1 < 2) return 0;
    return spin_carve(*desc, B1, nullptr).bytes;
}

extern "C" int nsvd_spin_jac_step(const nsvd_model_desc* desc, const nsvd_params* params, const float* x, int B1,
                                  const float* phi, float hard_mul_const, const double* gsigma, double decay, float* J,
                                  const nsvd_params* grads, void* ws, size_t ws_bytes, void* stream) {
    int rc = spin_validate(desc);
    if (rc) return rc;
    if (!params || !grads || !x || !phi || !gsigma || !J || !ws || B1 < 2) return NSVD_EINVAL;
    if (!(decay >= 0.0 && decay <= 1.0)) return NSVD_EINVAL;
    const nsvd_model_desc& d = *desc;
    if (!params->fourier_B) return NSVD_EINVAL;
    for (int i = 0; i < d.nlayers; ++i)
        if (!params->W[i] || !params->b[i] || !grads->W[i] || !grads->b[i]) return NSVD_EINVAL;
    const SpinWs w = spin_carve(d, B1, ws);
    if (!nsvd_ws_ok(ws, ws_bytes, w.bytes)) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int R = w.R, F = 2 * d.m, nl = d.nlayers;

    // activations a_0 .. a_{n-2} of the B1 rows: the layer sequence of the generic model path, rows of R floats
    rc = nsvd_fourier_features(x, params->fourier_B, w.phiT, B1, d.D, d.m, 0.f, 1, R, stream);
    if (rc) return rc;
    int kin = F;
    for (int i = 0; i + 1 < nl; ++i) {
        NsvdGemm g;
        g.batch = d.L;
        g.M = d.dims[i]; g.N = B1; g.K = kin;
        g.A = params->W[i]; g.sAm = kin; g.sAk = 1; g.bA = (long)d.dims[i] * kin;
        g.B = (i == 0) ? w.phiT : w.act[i - 1]; g.sBk = R; g.sBn = 1; g.bB = (i == 0) ? 0 : (long)kin * R;
        g.C = w.act[i]; g.sCm = R; g.bC = (long)d.dims[i] * R;
        g.bias = params->b[i]; g.bBias = d.dims[i];
        rc = nsvd_gemm_generic(g, s);
        if (rc) return rc;
        // (the pad columns B1 .. R are transformed with the rest and never read unmasked)
        rc = nsvd_softplus_inplace(w.act[i], (long)d.L * d.dims[i], R, 1, s);
        if (rc) return rc;
        kin = d.dims[i];
    }
    // unit-seed deltas: delta_{n-1} = hard_mul_const, delta_{i-1} = (W_i^T delta_i) sigmoid(z_{i-1})
    {
        const long n = (long)d.L * R;
        spin_fill_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(w.delta[nl - 1], n, hard_mul_const);
        NSVD_CHECK_LAUNCH();
    }
    for (int i = nl - 1; i > 0; --i) {
        const int hi = d.dims[i], kk = d.dims[i - 1];
        NsvdGemm dg;
        dg.batch = d.L;
        dg.M = kk; dg.N = B1; dg.K = hi;
        dg.A = params->W[i]; dg.sAm = 1; dg.sAk = kk; dg.bA = (long)hi * kk;
        dg.B = w.delta[i]; dg.sBk = R; dg.sBn = 1; dg.bB = (long)hi * R;
        dg.C = w.delta[i - 1]; dg.sCm = R; dg.bC = (long)kk * R;
        dg.Z = w.act[i - 1]; dg.sZm = R; dg.bZ = (long)kk * R;
        dg.sigmoid_mul = 1;
        rc = nsvd_gemm_generic(dg, s);
        if (rc) return rc;
    }

    SpinArgs A;
    memset(&A, 0, sizeof(A));
    A.nlayers = nl; A.L = d.L; A.B1 = B1; A.R = R; A.AB = w.AB; A.nblocks = w.nblocks; A.P = (long)w.P;
    A.phi = phi; A.gsigma = gsigma; A.J = J; A.part = w.part;
    A.omd = (float)(1.0 - decay); A.dec = (float)decay; A.scale = (float)(2.0 / (double)B1);
    long offW = 0, offb = 0;
    kin = F;
    for (int i = 0; i < nl; ++i) {
        offb += (long)d.L * d.dims[i] * kin;
        kin = d.dims[i];
    }
    kin = F;
    int tiles = 0;
    for (int i = 0; i < nl; ++i) {
        SpinLayer& Y = A.ly[i];
        Y.h = d.dims[i]; Y.kin = kin;
        Y.act = (i == 0) ? w.phiT : w.act[i - 1];
        Y.act_stride = (i == 0) ? 0 : (long)kin * R;
        Y.delta = w.delta[i];
        Y.delta_stride = (long)d.dims[i] * R;
        Y.offW = offW; Y.offb = offb;
        Y.gW = grads->W[i]; Y.gb = grads->b[i];
        Y.nrt = nsvd_cdiv(Y.h, SP_TM); Y.nkt = nsvd_cdiv(kin, SP_TN);
        Y.tile0 = tiles;
        tiles += d.L * Y.nrt * Y.nkt;
        offW += (long)d.L * d.dims[i] * kin;
        offb += (long)d.L * d.dims[i];
        kin = d.dims[i];
    }
    spin_jac_kernel<<<dim3(tiles, w.nblocks), SP_THREADS, 0, s>>>(A);
    NSVD_CHECK_LAUNCH();
    spin_reduce_kernel<<<(unsigned)((A.P + SP_THREADS - 1) / SP_THREADS), SP_THREADS, 0, s>>>(A);
    NSVD_CHECK_LAUNCH();
    return 0;
}
