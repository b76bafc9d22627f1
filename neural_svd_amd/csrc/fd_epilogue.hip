// Importance-weighted central-difference Hamiltonian on the head outputs, and the head of its
// backward.  Generic-path version (the fused MFMA kernel has the same math in its epilogue:
// nsvd_fd_point below is shared).
//   reference: WaveFunctions.forward           examples/operator/pde/__init__.py:15-16
//              ExponentialMask.forward         examples/operator/pde/boundary.py:46-53
//              VectorizedLaplacian.__call__    examples/operator/pde/diff_ops.py:9-23, 25-52
//              NegativeHamiltonian.__call__    examples/operator/pde/schrodinger/__init__.py:16-22
//              OperatorWrapper.__call__        examples/__init__.py:7-9
#include "nsvd_kernels.h"
#include "fd_math.h"

namespace {

// TRIG: the instance of the periodic problems (cosine potential, Fokker-Planck kind: fd_math.h)
template <bool TRIG>
__global__ void __launch_bounds__(256) fd_epilogue_kernel(const float* __restrict__ base, int ldr,
                                                          const float* __restrict__ x,
                                                          const float* __restrict__ scales, nsvd_problem prob,
                                                          float log_norm, int B, int D, int L, float* __restrict__ f,
                                                          float* __restrict__ Tf, float* __restrict__ jac,
                                                          float* __restrict__ dsc, int evenodd, NsvdBox box) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * L) return;
    const int b = idx / L, l = idx - b * L;
    float xc[NSVD_FD_MAXD];
    for (int d = 0; d < D; ++d) xc[d] = x[(size_t)b * D + d];
    const int E = 1 + 2 * D;
    float bv[2 * NSVD_FD_MAXD + 1];
    for (int e = 0; e < E; ++e) bv[e] = base[(size_t)l * ldr + (size_t)e * B + b];
    const float s_l = scales ? scales[l] : 0.f;
    NsvdFdOut o;
    if (evenodd) {  // rows 1 + 2 d / 2 + 2 d hold the even / odd perturbations of direction d (fused split-stencil form)
        float bE[NSVD_FD_MAXD], bO[NSVD_FD_MAXD];
        for (int d = 0; d < D; ++d) {
            bE[d] = bv[1 + 2 * d];
            bO[d] = bv[2 + 2 * d];
        }
        o = nsvd_fd_evenodd<TRIG>(bv[0], bE, bO, xc, D, scales != nullptr, s_l, prob, log_norm, box);
    } else {
        o = nsvd_fd_point<TRIG>(bv, xc, D, scales != nullptr, s_l, prob, log_norm, box);
    }
    f[idx] = o.f;
    Tf[idx] = o.Tf;
    if (jac) jac[idx] = o.jac;
    if (dsc) dsc[idx] = o.dsc;
}

// ---- 5 <= D <= NSVD_MAX_D: the direction-loop form (fd_math.h: nsvd_fd_evenodd_nd), even / odd rows only ---------------
// A workgroup takes ND_ROWS samples; wave g of its four takes the heads l = g (mod 4). Within a wave the lane is the
// sample, so each of the 2 D + 1 loads of `base` per head is one contiguous run of ND_ROWS floats, and what the L heads
// of a row share is computed once: per row by every thread (nsvd_fd_row_nd), per row and direction by one of the four
// waves into LDS (nsvd_fd_dir_nd). The (B, L) row-major outputs go through an LDS tile of
// ND_ROWS x ND_HEADS per output and leave as runs of ND_HEADS floats per row.
constexpr int ND_ROWS = 64, ND_HEADS = 16;
template <bool TRIG>
__global__ void __launch_bounds__(256) fd_epilogue_nd_kernel(const float* __restrict__ base, int ldr,
                                                             const float* __restrict__ x,
                                                             const float* __restrict__ scales, nsvd_problem prob,
                                                             float log_norm, int B, int D, int L, float* __restrict__ f,
                                                             float* __restrict__ Tf, float* __restrict__ jac,
                                                             float* __restrict__ dsc, NsvdBox box) {
    __shared__ float tile[4][ND_ROWS][ND_HEADS + 1];
    __shared__ float dirs[NSVD_MAX_D * NSVD_FD_DIR_FIELDS][ND_ROWS];  // nsvd_fd_dir_nd's table, the row fastest
    const int bl = threadIdx.x & (ND_ROWS - 1), g = threadIdx.x >> 6;
    const int b0 = blockIdx.x * ND_ROWS, b = b0 + bl;
    const bool bok = b < B;
    const float* xr = x + (size_t)(bok ? b : 0) * D;
    NsvdFdRowNd w;
    if (bok) {
        w = nsvd_fd_row_nd<TRIG>(xr, D, prob, log_norm, box);
        // wave g fills the directions d = g (mod 4) of its 64 rows: what the heads share along a direction, once
        for (int d = g; d < D; d += 4) nsvd_fd_dir_nd<TRIG>(w, xr, d, D, scales != nullptr, prob, box, &dirs[0][bl], ND_ROWS);
    }
    __syncthreads();
    for (int l0 = 0; l0 < L; l0 += ND_HEADS) {
        for (int lh = g; lh < ND_HEADS; lh += 4) {
            const int l = l0 + lh;
            if (!bok || l >= L) continue;
            const NsvdFdOut o = nsvd_fd_evenodd_nd<TRIG>(w, xr, base + (size_t)l * ldr + b, (size_t)B, D,
                                                         scales != nullptr, scales ? scales[l] : 0.f, prob, box,
                                                         &dirs[0][bl], ND_ROWS);
            tile[0][bl][lh] = o.f;
            tile[1][bl][lh] = o.Tf;
            tile[2][bl][lh] = o.jac;
            tile[3][bl][lh] = o.dsc;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ND_ROWS * ND_HEADS; i += 256) {
            const int r = i / ND_HEADS, h = i - r * ND_HEADS;
            if (b0 + r < B && l0 + h < L) {
                const size_t o = (size_t)(b0 + r) * L + l0 + h;
                f[o] = tile[0][r][h];
                Tf[o] = tile[1][r][h];
                if (jac) jac[o] = tile[2][r][h];
                if (dsc) dsc[o] = tile[3][r][h];
            }
        }
        __syncthreads();
    }
}

// ---- exact-Laplacian mode on the generic jets (NSVD_PATH_GENERIC_EXACT): `base` is (L, ldr) with row block 0 the head's
// value, blocks 1 .. D its derivatives along each axis, block D + 1 its Laplacian -------------------------------------
// D <= NSVD_FD_MAXD: one thread per (sample, head) gathers the jet and calls nsvd_fd_exact (the fused kernels' product rule)
__global__ void __launch_bounds__(256) fd_exact_kernel(const float* __restrict__ base, int ldr,
                                                       const float* __restrict__ x, const float* __restrict__ scales,
                                                       nsvd_problem prob, float log_norm, int B, int D, int L,
                                                       float* __restrict__ f, float* __restrict__ Tf,
                                                       float* __restrict__ jac, float* __restrict__ dsc, NsvdBox box) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * L) return;
    const int b = idx / L, l = idx - b * L;
    const float* bcol = base + (size_t)l * ldr + b;
    float xc[NSVD_FD_MAXD], db[NSVD_FD_MAXD];
#pragma unroll
    for (int d = 0; d < NSVD_FD_MAXD; ++d) {
        xc[d] = d < D ? x[(size_t)b * D + d] : 0.f;
        db[d] = d < D ? bcol[(size_t)(1 + d) * B] : 0.f;
    }
    const NsvdFdOut o = nsvd_fd_exact(bcol[0], db, bcol[(size_t)(D + 1) * B], xc, D, scales != nullptr,
                                      scales ? scales[l] : 0.f, prob, log_norm, box);
    f[idx] = o.f;
    Tf[idx] = o.Tf;
    if (jac) jac[idx] = o.jac;
    if (dsc) dsc[idx] = o.dsc;
}

// 5 <= D <= NSVD_MAX_D: the direction-loop form (fd_math.h: nsvd_fd_exact_nd), built like fd_epilogue_nd_kernel - ND_ROWS
// samples per workgroup, the lane is the sample, wave g takes the heads l = g (mod 4). Wave 0 fills the per-direction
// table of its 64 rows in LDS (x_d and the box factors by prefix / suffix products: sequential in d, once per row) and
// the two row sums the heads share; the outputs leave through the LDS tile as runs of ND_HEADS floats per row.
template <bool TRIG>
__global__ void __launch_bounds__(256) fd_exact_nd_kernel(const float* __restrict__ base, int ldr,
                                                          const float* __restrict__ x, const float* __restrict__ scales,
                                                          nsvd_problem prob, float log_norm, int B, int D, int L,
                                                          float* __restrict__ f, float* __restrict__ Tf,
                                                          float* __restrict__ jac, float* __restrict__ dsc, NsvdBox box) {
    __shared__ float tile[4][ND_ROWS][ND_HEADS + 1];
    __shared__ float dirs[NSVD_MAX_D * NSVD_FDX_DIR_FIELDS][ND_ROWS];
    __shared__ float rowsum[2][ND_ROWS];
    const int bl = threadIdx.x & (ND_ROWS - 1), g = threadIdx.x >> 6;
    const int b0 = blockIdx.x * ND_ROWS, b = b0 + bl;
    const bool bok = b < B;
    const float* xr = x + (size_t)(bok ? b : 0) * D;
    NsvdFdRowNd w;
    if (bok) {
        w = nsvd_fd_row_nd<TRIG>(xr, D, prob, log_norm, box);
        if (g == 0) {
            const NsvdFdExactRowNd e = nsvd_fd_exact_dirs_nd(xr, D, box, &dirs[0][bl], ND_ROWS);
            rowsum[0][bl] = e.xG;
            rowsum[1][bl] = e.lM;
        }
    }
    __syncthreads();
    NsvdFdExactRowNd e;
    e.xG = rowsum[0][bl];
    e.lM = rowsum[1][bl];
    for (int l0 = 0; l0 < L; l0 += ND_HEADS) {
        for (int lh = g; lh < ND_HEADS; lh += 4) {
            const int l = l0 + lh;
            if (!bok || l >= L) continue;
            const NsvdFdOut o = nsvd_fd_exact_nd(w, e, base + (size_t)l * ldr + b, (size_t)B, D, scales != nullptr,
                                                 scales ? scales[l] : 0.f, prob, box, &dirs[0][bl], ND_ROWS);
            tile[0][bl][lh] = o.f;
            tile[1][bl][lh] = o.Tf;
            tile[2][bl][lh] = o.jac;
            tile[3][bl][lh] = o.dsc;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ND_ROWS * ND_HEADS; i += 256) {
            const int r = i / ND_HEADS, h = i - r * ND_HEADS;
            if (b0 + r < B && l0 + h < L) {
                const size_t o = (size_t)(b0 + r) * L + l0 + h;
                f[o] = tile[0][r][h];
                Tf[o] = tile[1][r][h];
                if (jac) jac[o] = tile[2][r][h];
                if (dsc) dsc[o] = tile[3][r][h];
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) head_backward_kernel(const float* __restrict__ df,
                                                            const float* __restrict__ jac, int B, int L,
                                                            float* __restrict__ dzT) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * L) return;
    const int l = idx / B, b = idx - l * B;
    dzT[idx] = df[(size_t)b * L + l] * jac[(size_t)b * L + l];
}

__global__ void __launch_bounds__(256) dscales_kernel(const float* __restrict__ df, const float* __restrict__ dsc,
                                                      int B, int L, float* __restrict__ dscales) {
    __shared__ float red[4];
    const int l = blockIdx.x;
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) s += df[(size_t)b * L + l] * dsc[(size_t)b * L + l];
    s = nsvd_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) dscales[l] = red[0] + red[1] + red[2] + red[3];
}

__global__ void __launch_bounds__(256) model_out_kernel(const float* __restrict__ base, int ldr,
                                                        const float* __restrict__ x,
                                                        const float* __restrict__ scales, float c, int B, int D, int L,
                                                        float* __restrict__ out, float* __restrict__ jac,
                                                        float* __restrict__ dsc, NsvdBox box) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * L) return;
    const int b = idx / L, l = idx - b * L;
    const float bv = base[(size_t)l * ldr + b];
    float mk = 1.f, r = 0.f;
    if (scales) {
        float r2 = 0.f;
        for (int d = 0; d < D; ++d) r2 = fmaf(x[(size_t)b * D + d], x[(size_t)b * D + d], r2);
        r = sqrtf(r2);
        mk = expf(-r / scales[l]);
    }
    if (box.mode) {  // the box mask is a plain factor of the model output: it joins mk (and with it jac, dsc)
        float M = 1.f;
        for (int d = 0; d < D; ++d) {
            const float xv = x[(size_t)b * D + d];
            M *= nsvd_box_m1(box.lim - xv, box.lim + xv, box);
        }
        mk *= M;
    }
    out[idx] = c * bv * mk;
    if (jac) jac[idx] = c * mk;                                              // d out / d base
    if (dsc) dsc[idx] = scales ? c * bv * mk * r / (scales[l] * scales[l]) : 0.f;  // d out / d scales_l
}

}  // namespace

int nsvd_model_out(const float* base, int ldr, const float* x, const float* scales, float c, int B, int D, int L,
                   float* out, float* jac, float* dsc, hipStream_t s, NsvdBox box) {
    hipLaunchKernelGGL(model_out_kernel, dim3(nsvd_cdiv(B * L, 256)), dim3(256), 0, s, base, ldr, x, scales, c, B, D,
                       L, out, jac, dsc, box);
    NSVD_CHECK_LAUNCH();
    return 0;
}

int nsvd_fd_epilogue(const float* base, int ldr, const float* x, const float* scales, const nsvd_problem& prob,
                     int B, int D, int L, float* f, float* Tf, float* jac, float* dsc, hipStream_t s, int evenodd,
                     NsvdBox box) {
    const float log_norm = nsvd_importance_log_norm(D, prob);
    const bool trig = prob.potential == NSVD_POT_COSINE || prob.operator_kind == NSVD_OP_FOKKER_PLANCK;
    if (D > NSVD_FD_MAXD) {  // the direction-loop form: even / odd rows, the finite-difference mode
        if (D > NSVD_MAX_D || !evenodd || !(prob.eps > 0.f)) return NSVD_EUNSUPPORTED;
        hipLaunchKernelGGL(trig ? fd_epilogue_nd_kernel<true> : fd_epilogue_nd_kernel<false>,
                           dim3(nsvd_cdiv(B, ND_ROWS)), dim3(256), 0, s, base, ldr, x, scales, prob, log_norm, B, D, L,
                           f, Tf, jac, dsc, box);
        NSVD_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(trig ? fd_epilogue_kernel<true> : fd_epilogue_kernel<false>, dim3(nsvd_cdiv(B * L, 256)),
                       dim3(256), 0, s, base, ldr, x, scales, prob, log_norm, B, D, L, f, Tf, jac, dsc, evenodd, box);
    NSVD_CHECK_LAUNCH();
    return 0;
}

int nsvd_fd_epilogue_exact(const float* base, int ldr, const float* x, const float* scales, const nsvd_problem& prob,
                           int B, int D, int L, float* f, float* Tf, float* jac, float* dsc, hipStream_t s, NsvdBox box) {
    if (D < 1 || D > NSVD_MAX_D || ldr < (D + 2) * B || prob.operator_kind != NSVD_OP_SCHROEDINGER)
        return NSVD_EUNSUPPORTED;
    const float log_norm = nsvd_importance_log_norm(D, prob);
    if (D > NSVD_FD_MAXD) {
        const bool trig = prob.potential == NSVD_POT_COSINE;
        hipLaunchKernelGGL(trig ? fd_exact_nd_kernel<true> : fd_exact_nd_kernel<false>, dim3(nsvd_cdiv(B, ND_ROWS)),
                           dim3(256), 0, s, base, ldr, x, scales, prob, log_norm, B, D, L, f, Tf, jac, dsc, box);
        NSVD_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(fd_exact_kernel, dim3(nsvd_cdiv(B * L, 256)), dim3(256), 0, s, base, ldr, x, scales, prob,
                       log_norm, B, D, L, f, Tf, jac, dsc, box);
    NSVD_CHECK_LAUNCH();
    return 0;
}

int nsvd_head_backward(const float* df, const float* jac, const float* dsc, int B, int L, float* dzT,
                       float* dscales, hipStream_t s) {
    hipLaunchKernelGGL(head_backward_kernel, dim3(nsvd_cdiv(B * L, 256)), dim3(256), 0, s, df, jac, B, L, dzT);
    NSVD_CHECK_LAUNCH();
    if (dscales) {
        hipLaunchKernelGGL(dscales_kernel, dim3(L), dim3(256), 0, s, df, dsc, B, L, dscales);
        NSVD_CHECK_LAUNCH();
    }
    return 0;
}
