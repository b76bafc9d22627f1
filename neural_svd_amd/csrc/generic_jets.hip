// Forward-mode jets on the generic path (NSVD_PATH_GENERIC_EXACT): the exact Laplacian of the reference
// (VectorizedLaplacian.exact_laplacian, examples/operator/pde/diff_ops.py:54-61) for any model and 1 <= D <= 12.
// Every sample carries D + 2 streams through the network - the value, its D first derivatives and its Laplacian - laid
// out as D + 2 column blocks of B samples: block 0 the value, block 1 + d the derivative along d, block D + 1 the
// Laplacian. A linear layer maps each stream by itself (nsvd_gemm_generic with eo_cols = B: the bias joins block 0 only);
// the two kernels here are the jet of the Fourier map and the jet through softplus. The product rule with sqrt p, the
// masks and the potential is fd_epilogue.hip's (nsvd_fd_epilogue_exact).
#include "nsvd_kernels.h"
#include "fourier_body.h"

using nsvd_feat::sincos_d2f;

namespace {

// One thread per (frequency j, W consecutive samples): the projection in double and one sincos per sample, as
// fourier_evenodd_kernel; then for phi = [sin p | cos p], p = x . B_j:
//   d phi / d x_d = [cos p | -sin p] B_dj,      Lap phi = -|B_j|^2 [sin p | cos p]
// VEC: B % 4 == 0 - every block starts on a 16-byte boundary and the W = 4 samples leave as one store per row and block.
template <bool VEC>
__global__ void __launch_bounds__(256) fourier_jets_kernel(const float* __restrict__ x, const float* __restrict__ fB,
                                                           float* __restrict__ phiT, int B, int D, int m, int ldr) {
    constexpr int W = VEC ? 4 : 1;
    const int b = (blockIdx.x * blockDim.x + threadIdx.x) * W;
    const int j = blockIdx.y;
    if (b >= B) return;  // (VEC: B is a multiple of 4, so b + 3 < B)
    float s[W], c[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        double proj = 0.0;
        for (int d = 0; d < D; ++d) proj = fma((double)x[(size_t)(b + k) * D + d], (double)fB[(size_t)d * m + j], proj);
        sincos_d2f(proj, &s[k], &c[k]);
    }
    float* ps = phiT + (size_t)j * ldr + b;
    float* pc = phiT + (size_t)(m + j) * ldr + b;
    auto put = [&](float* dst, float fs, bool from_cos) {  // dst[k] = fs * (from_cos ? c[k] : s[k])
        if constexpr (VEC) {
            *(float4*)dst = from_cos ? make_float4(fs * c[0], fs * c[1], fs * c[2], fs * c[W - 1])
                                     : make_float4(fs * s[0], fs * s[1], fs * s[2], fs * s[W - 1]);
        } else {
            dst[0] = fs * (from_cos ? c[0] : s[0]);
        }
    };
    put(ps, 1.f, false);
    put(pc, 1.f, true);
    float q = 0.f;  // |B_j|^2
    for (int d = 0; d < D; ++d) {
        const float bdj = fB[(size_t)d * m + j];
        q = fmaf(bdj, bdj, q);
        put(ps + (size_t)(1 + d) * B, bdj, true);    // d sin / d x_d =  cos p B_dj
        put(pc + (size_t)(1 + d) * B, -bdj, false);  // d cos / d x_d = -sin p B_dj
    }
    put(ps + (size_t)(D + 1) * B, -q, false);
    put(pc + (size_t)(D + 1) * B, -q, true);
}

// The jet through softplus, in place. With s = sigmoid(z0) and s' = s (1 - s):
//   a = softplus(z0),   t_d <- s t_d,   l <- s l + s' sum_d t_d^2   (the sum over the incoming t_d)
// s and s' from t = e^-|z0| without a difference of O(1) numbers: r = 1 / (1 + t), s = r or t r, s' = t r^2; above
// torch's softplus threshold s = 1 and s' = 0, as autograd has them. A thread owns one (row, W consecutive samples) in
// every block: it walks d, accumulates the sum of squares and writes each t_d back as it goes - no array indexed by d.
// Block 0 afterwards holds the activation: what the next layer, the weight gradient and the backward's sigmoid factor
// (nsvd_sigmoid_from_softplus) read.
template <bool VEC>
__global__ void __launch_bounds__(256) softplus_jets_kernel(float* __restrict__ z, long rows, int B, int D, long R) {
    constexpr int W = VEC ? 4 : 1;
    const long per = B / W;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * per) return;
    const long row = idx / per;
    const int b = (int)(idx - row * per) * W;
    float* p = z + row * R + b;
    float z0[W], sg[W], sp[W], sq[W];
    if constexpr (VEC) {
        const float4 v = *(const float4*)p;
        z0[0] = v.x; z0[1] = v.y; z0[2] = v.z; z0[W - 1] = v.w;
    } else {
        z0[0] = p[0];
    }
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const float t = __builtin_amdgcn_exp2f(-fabsf(z0[c]) * NSVD_LOG2E);
        const float r = __builtin_amdgcn_rcpf(1.0f + t);
        const bool lin = z0[c] > NSVD_SOFTPLUS_THRESHOLD;
        sg[c] = lin ? 1.0f : (z0[c] >= 0.0f ? r : t * r);
        sp[c] = lin ? 0.0f : t * r * r;
        sq[c] = 0.f;
    }
    for (int d = 0; d < D; ++d) {
        float* pt = p + (long)(1 + d) * B;
        float t[W];
        if constexpr (VEC) {
            const float4 v = *(const float4*)pt;
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[W - 1] = v.w;
        } else {
            t[0] = pt[0];
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            sq[c] = fmaf(t[c], t[c], sq[c]);
            t[c] *= sg[c];
        }
        if constexpr (VEC) *(float4*)pt = make_float4(t[0], t[1], t[2], t[W - 1]);
        else pt[0] = t[0];
    }
    float* pl = p + (long)(D + 1) * B;
    float l[W];
    if constexpr (VEC) {
        const float4 v = *(const float4*)pl;
        l[0] = v.x; l[1] = v.y; l[2] = v.z; l[W - 1] = v.w;
    } else {
        l[0] = pl[0];
    }
#pragma unroll
    for (int c = 0; c < W; ++c) {
        l[c] = fmaf(sg[c], l[c], sp[c] * sq[c]);
        z0[c] = nsvd_softplus(z0[c]);
    }
    if constexpr (VEC) {
        *(float4*)pl = make_float4(l[0], l[1], l[2], l[W - 1]);
        *(float4*)p = make_float4(z0[0], z0[1], z0[2], z0[W - 1]);
    } else {
        pl[0] = l[0];
        p[0] = z0[0];
    }
}

}  // namespace

extern "C" int nsvd_fourier_features_jets(const float* x, const float* fourier_B, float* phiT, int B, int D, int m,
                                          int ldr, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!x || !fourier_B || !phiT || B <= 0 || D <= 0 || m <= 0 || ldr < (D + 2) * B) return NSVD_EINVAL;
    const bool vec = (B & 3) == 0 && (ldr & 3) == 0 && ((uintptr_t)phiT & 15) == 0;
    if (vec) hipLaunchKernelGGL(fourier_jets_kernel<true>, dim3(nsvd_cdiv(B / 4, 256), m), dim3(256), 0, s, x, fourier_B,
                                phiT, B, D, m, ldr);
    else hipLaunchKernelGGL(fourier_jets_kernel<false>, dim3(nsvd_cdiv(B, 256), m), dim3(256), 0, s, x, fourier_B, phiT,
                            B, D, m, ldr);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_softplus_jets_inplace(float* z, long long rows, int B, int D, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!z || rows <= 0 || B <= 0 || D < 1) return NSVD_EINVAL;
    const long R = (long)(D + 2) * B;
    const bool vec = (B & 3) == 0 && ((uintptr_t)z & 15) == 0;
    const long n = (long)rows * (vec ? B / 4 : B);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (vec) hipLaunchKernelGGL(softplus_jets_kernel<true>, dim3(blocks), dim3(256), 0, s, z, (long)rows, B, D, R);
    else hipLaunchKernelGGL(softplus_jets_kernel<false>, dim3(blocks), dim3(256), 0, s, z, (long)rows, B, D, R);
    NSVD_CHECK_LAUNCH();
    return 0;
}
