// NeuralEF (mu-EigenGame) on the operator path: the reference's NeuralEigenfunctions over BatchL2NormalizedFunctions
// (methods/neuralef.py:37-62,139-152, methods/utils.py:36-68) on top of the operator forward / centre backward.
//   nef_norms_kernel     per head: the batch norms n_e of every stencil point (n_+- as n_0^2 + mean_b (u_+-^2 - u0^2),
//                        formed from the even / odd rows), then the 1 + 2D running-norm updates in stencil order
//   nef_epilogue_kernel  phi, Tphi with 1 / n_e folded into the even / odd stencil (fd_math.h: nsvd_nef_evenodd); h, r,
//                        jac / dsc of u0 for the backward
//   nef_gram_kernel      partial Gram matrices phi_h^T phi_h (or phi_h^T Tphi_h) over 64-row blocks of each half
//   nef_gram_sum_kernel  the partials of each half added in block order
//   nef_align_kernel     coeff_h from the Grams, align_h = Tphi_h coeff_h / B_h, d loss / d phi, per-block loss partials
//   nef_loss_kernel      the loss partials added in block order
//   nef_norm_bwd_kernel  du0 = (dh - h mean_b(dh h)) / n0, dh = r dphi, then the existing centre backward
// Every reduction runs in a fixed order; no float atomics.
#include <string.h>
#include "nsvd_kernels.h"
#include "fd_math.h"

namespace {

constexpr int NEF_ROWS = 64;    // rows per block of the Gram / align kernels
constexpr int NEF_MAXL = 64;    // heads the loss kernels take
constexpr int NEF_MAXE = 2 * NSVD_FD_MAXD + 1;

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    // fixed order: wave butterfly, then the four wave sums in wave order
    v = nsvd_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(256) nef_norms_kernel(const float* __restrict__ raw, int ldr,
                                                        const float* __restrict__ x, const float* __restrict__ scales,
                                                        nsvd_problem prob, int B, int D, int L,
                                                        float* __restrict__ stats, float* __restrict__ rn_b,
                                                        float* __restrict__ rn_u, const int* __restrict__ initialized,
                                                        float momentum) {
    __shared__ float red[4];
    const int l = blockIdx.x;
    const float* br = raw + (size_t)l * ldr;
    const bool has_mask = scales != nullptr;
    const float s_l = has_mask ? scales[l] : 1.f;
    const float c = prob.hard_mul_const;
    float s0 = 0.f, de[NSVD_FD_MAXD], dodd[NSVD_FD_MAXD];
    for (int d = 0; d < NSVD_FD_MAXD; ++d) de[d] = dodd[d] = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float xc[NSVD_FD_MAXD];
        float r2 = 0.f;
        for (int d = 0; d < D; ++d) {
            xc[d] = x[(size_t)b * D + d];
            r2 = fmaf(xc[d], xc[d], r2);
        }
        const float r0 = sqrtf(r2);
        const float mk0 = has_mask ? expf(-r0 / s_l) : 1.f;
        const float base0 = br[b];
        const float u0 = c * base0 * mk0;
        s0 = fmaf(u0, u0, s0);
        for (int d = 0; d < D; ++d) {
            // the mask alone (u is the WaveFunctions output: no importance weight)
            const NsvdEvenOdd m = has_mask ? nsvd_fd_ratio_eo(xc[d], r2, r0, prob.eps, 0.f, true, s_l) : NsvdEvenOdd{0.f, 0.f};
            const NsvdNefDelta q = nsvd_nef_sqdelta(u0, c * mk0, base0, br[(size_t)(1 + 2 * d) * B + b],
                                                    br[(size_t)(2 + 2 * d) * B + b], m);
            de[d] += q.even;
            dodd[d] += q.odd;
        }
    }
    const float S0 = block_sum_256(s0, red);
    float De[NSVD_FD_MAXD], Do[NSVD_FD_MAXD];
    for (int d = 0; d < D; ++d) {
        De[d] = block_sum_256(de[d], red);
        Do[d] = block_sum_256(dodd[d], red);
    }
    if (threadIdx.x != 0) return;
    const float n0 = sqrtf(S0 / (float)B);
    float n[NEF_MAXE];
    n[0] = n0;
    stats[l] = n0;
    for (int d = 0; d < D; ++d) {
        for (int sgn = 0; sgn < 2; ++sgn) {
            const float a = (sgn == 0 ? De[d] + Do[d] : De[d] - Do[d]) / S0;  // n_e^2 / n0^2 - 1
            const float s = sqrtf(1.f + a);
            const float kap = a / (s + 1.f);                                  // n_e / n0 - 1
            n[1 + 2 * d + sgn] = n0 * s;
            stats[(size_t)(1 + 2 * d + sgn) * L + l] = -kap / (1.f + kap);   // n0 / n_e - 1
        }
    }
    // BatchL2NormalizedFunctions.update_norm once per stencil point, in the reference's call order
    float rb = rn_b[l], ru = rn_u[l];
    const int init = *initialized;
    const float m1 = 1.f - momentum;
    for (int e = 0; e < 1 + 2 * D; ++e) {
        if (e == 0 && !init) {
            rb = n[0];
            ru = n[0];
        } else {
            rb = momentum * rb + m1 * n[e];
            ru = sqrtf(momentum * (ru * ru) + m1 * (n[e] * n[e]));
        }
    }
    rn_b[l] = rb;
    rn_u[l] = ru;
}

__global__ void __launch_bounds__(256) nef_epilogue_kernel(const float* __restrict__ raw, int ldr,
                                                           const float* __restrict__ x,
                                                           const float* __restrict__ scales, nsvd_problem prob,
                                                           float log_norm, int B, int D, int L,
                                                           const float* __restrict__ stats, float* __restrict__ phi,
                                                           float* __restrict__ Tphi, float* __restrict__ h,
                                                           float* __restrict__ r, float* __restrict__ jac,
                                                           float* __restrict__ dsc, int* __restrict__ initialized) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0 && initialized) *initialized = 1;  // (nef_norms_kernel of this step has read it)
    if (idx >= B * L) return;
    const int b = idx / L, l = idx - b * L;
    float xc[NSVD_FD_MAXD], bE[NSVD_FD_MAXD], bO[NSVD_FD_MAXD], nu[2 * NSVD_FD_MAXD];
    for (int d = 0; d < D; ++d) {
        xc[d] = x[(size_t)b * D + d];
        bE[d] = raw[(size_t)l * ldr + (size_t)(1 + 2 * d) * B + b];
        bO[d] = raw[(size_t)l * ldr + (size_t)(2 + 2 * d) * B + b];
        nu[2 * d] = stats[(size_t)(1 + 2 * d) * L + l];
        nu[2 * d + 1] = stats[(size_t)(2 + 2 * d) * L + l];
    }
    const float s_l = scales ? scales[l] : 0.f;
    const NsvdNefOut o = nsvd_nef_evenodd(raw[(size_t)l * ldr + b], bE, bO, xc, D, scales != nullptr, s_l, prob, log_norm,
                                          stats[l], nu);
    phi[idx] = o.phi;
    Tphi[idx] = o.Tphi;
    h[idx] = o.h;
    r[idx] = o.r;
    jac[idx] = o.jac;
    if (dsc) dsc[idx] = o.dsc;
}

// ---------------------------------------------------------------------------------------------- loss
struct NefLossArgs {
    const float* phi;   // (B, L) and its operator image: the variance term
    const float* Tphi;
    const float* ph[2];  // (B_h, L): the halves of the alignment term
    const float* Tph[2];
    int B, Bh[2], L;
    int unbiased, diagonal;
    int chunked;         // ph / Tph are the two chunks of phi / Tphi: one d loss / d phi, both terms per row
    int nblk[2];         // 64-row blocks of each half
    int nvar;            // 64-row blocks of the separate variance pass (not chunked)
    float* part;         // (nblk[0] + nblk[1]) L L partial Grams
    float* gram;         // 2 L L
    float* lpart;        // per align / variance block loss partials
    float* loss;
    float* dphi;         // (B, L): 4 variance (+ 2 align when chunked)
    float* dph[2];       // (B_h, L): 2 align (not chunked)
};

__global__ void __launch_bounds__(256) nef_gram_kernel(NefLossArgs a) {
    __shared__ float As[NEF_ROWS * NEF_MAXL];
    __shared__ float Cs[NEF_ROWS * NEF_MAXL];
    const int hh = blockIdx.x < a.nblk[0] ? 0 : 1;
    const int blk = blockIdx.x - (hh ? a.nblk[0] : 0);
    const int L = a.L, r0 = blk * NEF_ROWS;
    const int nr = min(NEF_ROWS, a.Bh[hh] - r0);
    const float* A = a.ph[hh] + (size_t)r0 * L;
    const float* Cm = (a.unbiased ? a.ph[hh] : a.Tph[hh]) + (size_t)r0 * L;
    for (int t = threadIdx.x; t < nr * L; t += blockDim.x) {
        As[t] = A[t];
        Cs[t] = Cm[t];
    }
    __syncthreads();
    float* out = a.part + (size_t)blockIdx.x * L * L;
    for (int t = threadIdx.x; t < L * L; t += blockDim.x) {
        const int i = t / L, j = t - i * L;
        float s = 0.f;
        for (int k = 0; k < nr; ++k) s = fmaf(As[k * L + i], Cs[k * L + j], s);
        out[t] = s;
    }
}

__global__ void __launch_bounds__(256) nef_gram_sum_kernel(NefLossArgs a) {
    const int LL = a.L * a.L;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * LL) return;
    const int hh = t / LL, e = t - hh * LL;
    const float* p = a.part + (size_t)(hh ? a.nblk[0] : 0) * LL + e;
    float s = 0.f;
    for (int k = 0; k < a.nblk[hh]; ++k) s += p[(size_t)k * LL];
    a.gram[t] = s / (float)a.Bh[hh];  // compute_gram: einsum / B_h
}

__global__ void __launch_bounds__(256) nef_align_kernel(NefLossArgs a) {
    __shared__ float coef[NEF_MAXL * NEF_MAXL];
    __shared__ float Ts[NEF_ROWS * NEF_MAXL];
    __shared__ float red[4];
    const int L = a.L, LL = L * L;
    const int na = a.nblk[0] + a.nblk[1];
    float lsum = 0.f;
    if ((int)blockIdx.x < na) {
        const int hh = blockIdx.x < a.nblk[0] ? 0 : 1;
        const int r0 = (blockIdx.x - (hh ? a.nblk[0] : 0)) * NEF_ROWS;
        const int nr = min(NEF_ROWS, a.Bh[hh] - r0);
        // coeff_h (methods/neuralef.py:43-50): triu(G_h, diagonal) unbiased; biased: triu(Q_o) / (diag(Q_o) + 1e-5) by
        // row with Q_o the OTHER half's phi^T Tphi
        const float* G = a.gram + (size_t)(a.unbiased ? hh : 1 - hh) * LL;
        // biased with the diagonal kept, chunked: coeff_ii = Q_ii / (Q_ii + 1e-5) is 1 to 1e-5 / Q_ii, and 2 align's own
        // head term cancels 4 variance down to that remainder (all of d loss / d phi at L = 1, or once the off-diagonal
        // of Q has gone): `coef` then holds coeff - I with the remainder formed directly, the identity's part added below
        const bool own = !a.unbiased && a.diagonal == 0 && a.chunked;
        for (int t = threadIdx.x; t < LL; t += blockDim.x) {
            const int i = t / L, j = t - i * L;
            float v = (j - i >= a.diagonal) ? G[t] : 0.f;
            if (!a.unbiased) v = (own && i == j) ? -1e-5f / (G[t] + 1e-5f) : v / (G[i * L + i] + 1e-5f);
            coef[t] = v;
        }
        const float* Tp = a.Tph[hh] + (size_t)r0 * L;
        for (int t = threadIdx.x; t < nr * L; t += blockDim.x) Ts[t] = Tp[t];
        __syncthreads();
        const float* P = a.ph[hh] + (size_t)r0 * L;
        const float Bh = (float)a.Bh[hh], Bf = (float)a.B;
        for (int t = threadIdx.x; t < nr * L; t += blockDim.x) {
            const int k = t / L, m = t - k * L;
            float s = 0.f;
            for (int i = 0; i < L; ++i) s = fmaf(Ts[k * L + i], coef[i * L + m], s);
            const float al = own ? (s + Ts[t]) / Bh : s / Bh;
            const float pv = P[t];
            if (a.chunked) {
                const float var = -Ts[t] / Bf;
                // own: 4 var + 2 al = 2 s / B_h + Tphi (2 / B_h - 4 / B), the bracket from the integers (0 at even B)
                a.dphi[(size_t)(r0 + (hh ? a.Bh[0] : 0)) * L + t] =
                    own ? 2.f * (s / Bh) + Ts[t] * ((float)(2 * a.B - 4 * a.Bh[hh]) / (Bh * Bf)) : 4.f * var + 2.f * al;
                lsum += pv * var + 0.5f * (pv * al);
            } else {
                a.dph[hh][(size_t)r0 * L + t] = 2.f * al;
                lsum += 0.5f * (pv * al);
            }
        }
    } else {
        // variance term on its own rows (independent halves)
        const int r0 = (blockIdx.x - na) * NEF_ROWS;
        const int nr = min(NEF_ROWS, a.B - r0);
        const float Bf = (float)a.B;
        for (int t = threadIdx.x; t < nr * L; t += blockDim.x) {
            const size_t o = (size_t)r0 * L + t;
            const float var = -a.Tphi[o] / Bf;
            a.dphi[o] = 4.f * var;
            lsum += a.phi[o] * var;
        }
    }
    const float s = block_sum_256(lsum, red);
    if (threadIdx.x == 0) a.lpart[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) nef_loss_kernel(const float* __restrict__ lpart, int n, float* __restrict__ loss) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += lpart[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) loss[0] = s;
}

// ---------------------------------------------------------------------------------------------- backward
__global__ void __launch_bounds__(256) nef_norm_bwd_kernel(const float* __restrict__ dphi, const float* __restrict__ h,
                                                           const float* __restrict__ r,
                                                           const float* __restrict__ stats, int B, int L,
                                                           float* __restrict__ du0) {
    __shared__ float red[4];
    const int l = blockIdx.x;
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const size_t o = (size_t)b * L + l;
        s = fmaf(r[o] * dphi[o], h[o], s);
    }
    const float cl = block_sum_256(s, red) / (float)B;
    const float n0 = stats[l];
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const size_t o = (size_t)b * L + l;
        du0[o] = (r[o] * dphi[o] - h[o] * cl) / n0;
    }
}

__global__ void __launch_bounds__(256) nef_scale_heads_kernel(float* __restrict__ f, float* __restrict__ Tf,
                                                              const float* __restrict__ norm, int B, int L) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * L) return;
    const float n = norm[idx % L];
    f[idx] = f[idx] / n;
    Tf[idx] = Tf[idx] / n;
}

NefLossArgs loss_args(const float* phi, const float* Tphi, int B, const float* phi1, const float* Tphi1, int B1,
                      const float* phi2, const float* Tphi2, int B2, int L) {
    NefLossArgs a;
    memset(&a, 0, sizeof(a));
    a.phi = phi; a.Tphi = Tphi;
    a.ph[0] = phi1; a.Tph[0] = Tphi1; a.ph[1] = phi2; a.Tph[1] = Tphi2;
    a.B = B; a.Bh[0] = B1; a.Bh[1] = B2; a.L = L;
    a.chunked = phi1 == phi && Tphi1 == Tphi && phi2 == phi + (size_t)B1 * L && Tphi2 == Tphi + (size_t)B1 * L &&
                B1 + B2 == B;
    a.nblk[0] = nsvd_cdiv(B1, NEF_ROWS);
    a.nblk[1] = nsvd_cdiv(B2, NEF_ROWS);
    a.nvar = a.chunked ? 0 : nsvd_cdiv(B, NEF_ROWS);
    return a;
}

size_t loss_ws_bytes(const NefLossArgs& a) {
    const size_t LL = (size_t)a.L * a.L;
    return nsvd_align(((size_t)(a.nblk[0] + a.nblk[1]) * LL) * sizeof(float)) + nsvd_align(2 * LL * sizeof(float)) +
           nsvd_align((size_t)(a.nblk[0] + a.nblk[1] + a.nvar) * sizeof(float));
}

bool loss_shape_ok(int B, int B1, int B2, int L) {
    return L >= 1 && L <= NEF_MAXL && B >= 1 && B1 >= 1 && B2 >= 1 && B <= 65536 && B1 <= 65536 && B2 <= 65536;
}

}  // namespace

extern "C" size_t nsvd_nef_loss_workspace_bytes(int B, int B1, int B2, int L) {
    if (!loss_shape_ok(B, B1, B2, L)) return 0;
    // (the larger of the chunked and independent layouts: the same scratch serves either)
    NefLossArgs a;
    memset(&a, 0, sizeof(a));
    a.L = L;
    a.nblk[0] = nsvd_cdiv(B1, NEF_ROWS);
    a.nblk[1] = nsvd_cdiv(B2, NEF_ROWS);
    a.nvar = nsvd_cdiv(B, NEF_ROWS);
    return loss_ws_bytes(a);
}

extern "C" int nsvd_nef_loss(const float* phi, const float* Tphi, int B, const float* phi1, const float* Tphi1, int B1,
                             const float* phi2, const float* Tphi2, int B2, int L, int unbiased, int diagonal,
                             float* loss, float* dphi, float* dphi1, float* dphi2, void* scratch, size_t scratch_bytes,
                             void* stream) {
    if (!loss_shape_ok(B, B1, B2, L)) return NSVD_EUNSUPPORTED;
    if (!phi || !Tphi || !phi1 || !Tphi1 || !phi2 || !Tphi2 || !loss || !dphi || !scratch) return NSVD_EINVAL;
    if (diagonal != 0 && diagonal != 1) return NSVD_EINVAL;
    NefLossArgs a = loss_args(phi, Tphi, B, phi1, Tphi1, B1, phi2, Tphi2, B2, L);
    if (!a.chunked && (!dphi1 || !dphi2)) return NSVD_EINVAL;
    if (!nsvd_ws_ok(scratch, scratch_bytes, nsvd_nef_loss_workspace_bytes(B, B1, B2, L))) return NSVD_EINVAL;
    a.unbiased = unbiased ? 1 : 0;
    a.diagonal = diagonal;
    const size_t LL = (size_t)L * L;
    char* p = (char*)scratch;
    a.part = (float*)p;
    p += nsvd_align((size_t)(a.nblk[0] + a.nblk[1]) * LL * sizeof(float));
    a.gram = (float*)p;
    p += nsvd_align(2 * LL * sizeof(float));
    a.lpart = (float*)p;
    a.loss = loss;
    a.dphi = dphi;
    a.dph[0] = dphi1;
    a.dph[1] = dphi2;
    hipStream_t s = (hipStream_t)stream;
    const int nab = a.nblk[0] + a.nblk[1];
    hipLaunchKernelGGL(nef_gram_kernel, dim3(nab), dim3(256), 0, s, a);
    NSVD_CHECK_LAUNCH();
    hipLaunchKernelGGL(nef_gram_sum_kernel, dim3(nsvd_cdiv(2 * (int)LL, 256)), dim3(256), 0, s, a);
    NSVD_CHECK_LAUNCH();
    hipLaunchKernelGGL(nef_align_kernel, dim3(nab + a.nvar), dim3(256), 0, s, a);
    NSVD_CHECK_LAUNCH();
    hipLaunchKernelGGL(nef_loss_kernel, dim3(1), dim3(256), 0, s, a.lpart, nab + a.nvar, loss);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_nef_operator_forward(const nsvd_model_desc* desc, const nsvd_params* params,
                                         const nsvd_problem* prob, const float* x, int B, float* phi, float* Tphi,
                                         float* h, float* r, float* stats, float* norm_biased, float* norm_unbiased,
                                         int* initialized, float momentum, void* ws, size_t ws_bytes, int path,
                                         void* stream) {
    if (!desc || !params || !prob || !x || !phi || !Tphi || !h || !r || !stats || !norm_biased || !norm_unbiased ||
        !initialized || !ws || B <= 0)
        return NSVD_EINVAL;
    if (desc->D < 1 || desc->L <= 0) return NSVD_EINVAL;
    if (desc->D > NSVD_FD_MAXD) return NSVD_EUNSUPPORTED;  // (the per-point batch norms stop at the small stencil)
    if (desc->has_exp_mask && !params->scales) return NSVD_EINVAL;
    if (!nsvd_ws_ok(ws, ws_bytes, nsvd_workspace_bytes(desc, B))) return NSVD_EINVAL;
    const int st = nsvd_problem_status(*desc, *prob);
    if (st) return st;
    // NeuralEF is built on the Schroedinger kind (every potential of nsvd_potential)
    if (prob->operator_kind != NSVD_OP_SCHROEDINGER) return NSVD_EUNSUPPORTED;
    // the per-point batch norms know neither the box mask nor the uniform density (nsvd_operator_forward_raw refuses too)
    if (desc->box_mask != NSVD_BOX_NONE || prob->use_importance > NSVD_IMP_GAUSSIAN) return NSVD_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    NsvdRawOut o;
    int rc = nsvd_operator_forward_raw(*desc, *params, *prob, x, B, ws, path, s, &o);
    if (rc) return rc;
    const float* scales = desc->has_exp_mask ? params->scales : nullptr;
    hipLaunchKernelGGL(nef_norms_kernel, dim3(desc->L), dim3(256), 0, s, o.raw, o.ldr, x, scales, *prob, B, desc->D,
                       desc->L, stats, norm_biased, norm_unbiased, (const int*)initialized, momentum);
    NSVD_CHECK_LAUNCH();
    hipLaunchKernelGGL(nef_epilogue_kernel, dim3(nsvd_cdiv(B * desc->L, 256)), dim3(256), 0, s, o.raw, o.ldr, x, scales,
                       *prob, nsvd_gauss_log_norm(desc->D, prob->sigma), B, desc->D, desc->L, (const float*)stats, phi,
                       Tphi, h, r, o.jac, o.dsc, initialized);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_nef_operator_backward(const nsvd_model_desc* desc, const nsvd_params* params,
                                          const nsvd_problem* prob, const float* x, int B, const float* dphi,
                                          const float* h, const float* r, const float* stats, float* du0,
                                          const nsvd_params* grads, void* ws, size_t ws_bytes, int path, void* stream) {
    if (!desc || !dphi || !h || !r || !stats || !du0 || B <= 0 || desc->L <= 0) return NSVD_EINVAL;
    // (nsvd_operator_backward judges the workspace again, behind this launch: a bad one is refused before anything runs)
    if (!nsvd_ws_ok(ws, ws_bytes, nsvd_workspace_bytes(desc, B))) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nef_norm_bwd_kernel, dim3(desc->L), dim3(256), 0, s, dphi, h, r, stats, B, desc->L, du0);
    NSVD_CHECK_LAUNCH();
    // jac / dsc in `ws` are those of u0 (nef_epilogue_kernel): the centre backward takes du0 for df
    return nsvd_operator_backward(desc, params, prob, x, B, du0, grads, ws, ws_bytes, path, stream);
}

extern "C" int nsvd_nef_scale_heads(float* f, float* Tf, const float* norm, int B, int L, void* stream) {
    if (!f || !Tf || !norm || B <= 0 || L <= 0) return NSVD_EINVAL;
    hipLaunchKernelGGL(nef_scale_heads_kernel, dim3(nsvd_cdiv(B * L, 256)), dim3(256), 0, (hipStream_t)stream, f, Tf,
                       norm, B, L);
    NSVD_CHECK_LAUNCH();
    return 0;
}
