// CDK towers: Linear -> BatchNorm1d -> LeakyReLU -> Linear -> BatchNorm1d, forward and backward,
// as hand-written gfx950 kernels. Reference: examples/models/mlp.py:129-164 (get_mlp), used as the two backbones of
// examples/models/siam.py:132-166 (HeteroNetwork) by examples/cdk/sketchy/main_sketchy.py:107-116 with sizes
// 512 -> 8192 -> 512, lrelu0.2, BatchNorm on every layer, batch 1024 (BASELINE configs[4]).
//
// Every contraction is brought into the "NT" form C = A B^T with both operands contraction-contiguous and runs on the
// 128 x 128 fp32-MFMA tile loop shared with the layer-0 weight gradient (tile128_dma.h); the producers write the
// transposed copies the backward contractions need (the activations, the pre-activation gradients) so that no GEMM
// ever stages a strided operand:
//   forward   Y1 = X W1^T + b1            A = X (B, d0)       B = W1 (d1, d0)          K = d0
//             A1 = lrelu(BN1(Y1))         strip kernel: also writes A1^T (d1, B)
//             Y2 = A1 W2^T + b2           A = A1 (B, d1)      B = W2 (d2, d1)          K = d1, split-K partials, summed
//                                         (with the bias) by a coalesced elementwise kernel
//             Z  = BN2(Y2)                strip kernel
//   backward  dY2 = BN2'(dZ)              strip kernel: also writes dY2^T (d2, B), db2, dgamma2, dbeta2
//             dW2 = dY2^T A1              A = dY2^T (d2, B)   B = A1^T (d1, B)         K = B
//             dA1 = dY2 W2                A = dY2 (B, d2)     B = W2^T (d1, d2)        K = d2   (W2^T: transpose kernel)
//             dY1 = BN1'(lrelu'(dA1))     strip kernel: writes dY1^T (d1, B) only, db1, dgamma1, dbeta1
//             dW1 = dY1^T X               A = dY1^T (d1, B)   B = X^T (d0, B)          K = B    (X^T: transpose kernel)
// BatchNorm is training-mode torch.nn.BatchNorm1d: biased batch variance for the normalisation, unbiased for the
// running estimate, momentum update of running_mean / running_var (eps 1e-5, momentum 0.1 by default).
// Shapes: B, d0, d1, d2 multiples of 128, B <= 1024 (a BatchNorm strip's rows live in the registers of one workgroup).
#include "nsvd_kernels.h"
#include "tile128_dma.h"
#include "gemm16.h"
#include "tower_col.h"

using namespace nsvd_pmlp;

namespace {

// ---------------------------------------------------------------------------------------------- C = A B^T
struct GemmNT {
    const float* A;   // (M, lda) rows contraction-contiguous
    const float* B;   // (N, ldb)
    float* C;         // (M, ldc), or split-K slice s at C + s * slice_stride
    const float* bias;  // per column of C (N) or null (never with split-K: the strip kernel adds it)
    float* sumsq;       // null, or one float per workgroup: the sum of squares of its tile of C (gradient-norm clipping
                        // of the fused training step: the norm costs no extra pass over the weight gradients)
    size_t lda, ldb, ldc, slice_stride;
    int M, N, K, S;   // S split-K slices of K / S columns each
};

__global__ void __launch_bounds__(256, 2) tower_gemm_nt_kernel(GemmNT g) {
    __shared__ __attribute__((aligned(16))) float smem[T128D_LDS_FLOATS];  // 64 KB: two blocks per CU
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int wm = w >> 1, wn = w & 1;
    const int tn = g.N / 128, tm = g.M / 128;
    int bid = blockIdx.x;
    const int slice = bid / (tm * tn);
    bid -= slice * tm * tn;
    // tiles that share their A rows (same tile row) are neighbours in block order: blocks b, b + 8, .. share an XCD
    const int trow = bid / tn, tcol = bid - trow * tn;
    const int Ks = g.K / g.S;  // floats per row and slice
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const float* a_base = g.A + (size_t)128 * trow * g.lda + (size_t)slice * Ks;
    const float* b_base = g.B + (size_t)128 * tcol * g.ldb + (size_t)slice * Ks;
    nsvd_tile128_dma<2>(a_base, b_base, (unsigned)g.lda, (unsigned)g.ldb, Ks / BK, smem, acc);
    float* C = g.C + (size_t)slice * g.slice_stride + ((size_t)128 * trow + 64 * wm) * g.ldc + 128 * tcol + 64 * wn + li;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float bv = g.bias ? g.bias[128 * tcol + 64 * wn + 32 * j + li] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float cv = acc[i][j][r] + bv;
                C[(size_t)(32 * i + acc_row(r, hi)) * g.ldc + 32 * j] = cv;
                ss = fmaf(cv, cv, ss);
            }
    }
    if (g.sumsq) {  // fixed order: lanes of a wave (butterfly), then the four waves
        ss = nsvd_wave_sum(ss);
        __syncthreads();  // the tile loop's last fragment reads are done: reuse its LDS
        if (lane == 0) smem[w] = ss;
        __syncthreads();
        if (tid == 0) g.sumsq[blockIdx.x] = (smem[0] + smem[1]) + (smem[2] + smem[3]);
    }
}

// ---------------------------------------------------------------------------------------------- transposes
// out (C, R) = in (R, C)^T, 32 x 32 tiles through LDS
// float32 -> bfloat16, round to nearest even (v_cvt_pk_bf16_f32)
typedef __bf16 nsvd_bf16x2 __attribute__((ext_vector_type(2)));
typedef float nsvd_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned bf16_pack2(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((nsvd_f32x2){a, b}, nsvd_bf16x2));
}
__device__ __forceinline__ uint2 bf16_pack4(const float4& v) { return make_uint2(bf16_pack2(v.x, v.y), bf16_pack2(v.z, v.w)); }
// the half type by a (wave-uniform) code: 1 = bfloat16, 2 = IEEE float16 (gemm16.h: pack_h)
__device__ __forceinline__ uint2 half_pack4(const float4& v, int code) {
    if (code == 2) return make_uint2(nsvd_g16::pack_h<true>(v.x, v.y), nsvd_g16::pack_h<true>(v.z, v.w));
    return bf16_pack4(v);
}
__device__ __forceinline__ unsigned short bf16_one(float a) { return (unsigned short)(bf16_pack2(a, 0.f) & 0xffffu); }

__global__ void __launch_bounds__(256) tower_transpose_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              int R, int Cc) {
    __shared__ float t[32][33];
    const int tiles_c = Cc / 32;
    const int tr = blockIdx.x / tiles_c, tc = blockIdx.x - tr * tiles_c;
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;  // 8 rows per pass
#pragma unroll
    for (int k = 0; k < 4; ++k) t[y + 8 * k][x] = in[(size_t)(32 * tr + y + 8 * k) * Cc + 32 * tc + x];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out[(size_t)(32 * tc + y + 8 * k) * R + 32 * tr + x] = t[x][y + 8 * k];
    }
}

// out (B, N) = bias + sum of the S split-K partial outputs, slices added in order (fully coalesced 16-byte accesses: as
// part of the narrow BatchNorm strips each row contributed 16-32 bytes of a 128-byte line per slice)
__global__ void __launch_bounds__(256) tower_sum_slices_kernel(const float* __restrict__ part, size_t slice_stride,
                                                               int S, const float* __restrict__ bias,
                                                               float* __restrict__ out, int N, size_t n4) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    const int c = (int)((q * 4) % (size_t)N);
    float4 v = bias ? *reinterpret_cast<const float4*>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s0 = 0; s0 < S; s0 += 8) {
        float4 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            t[j] = s0 + j < S ? *reinterpret_cast<const float4*>(part + (size_t)(s0 + j) * slice_stride + 4 * q)
                              : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v.x += t[j].x; v.y += t[j].y; v.z += t[j].z; v.w += t[j].w;
        }
    }
    *reinterpret_cast<float4*>(out + 4 * q) = v;
}

// ---------------------------------------------------------------------------------------------- BatchNorm strips
// One workgroup = STRIP columns x all B rows, held in REGISTERS: thread t owns the four columns 4 (t % CG).. of rows
// (t / CG) + RG k, k < B / RG (CG = STRIP / 4 column groups, RG = 256 / CG row groups; B <= 1024 gives at most 16 rows
// of 4 floats per thread). Every row load of the strip is issued before the first is consumed (128 KB in flight per
// workgroup), nothing but a transpose tile and the reduction scratch lives in LDS, so several workgroups share a CU.
// (With the strip in LDS - 132 KB, one workgroup per CU - the 1024 x 8192 forward strip took 90 us for 96 MB.)
// Column statistics in a fixed order: RG row groups per column, combined in LDS.
struct BnFwd {
    const float* Y;       // (S, B, N) split-K partials of the pre-normalisation output (S = 1: the output itself)
    size_t slice_stride;
    int S;
    const float* bias;    // added to the summed partials (null: already added by the GEMM)
    const float* gamma;   // BatchNorm weight / bias (N)
    const float* beta;
    float* running_mean;  // updated in place (null: no running statistics)
    float* running_var;
    float* mean;          // (N) saved for the backward
    float* invstd;        // (N)
    float* Ysum;          // (B, N) summed pre-normalisation output, written when S > 1 or bias != null (else null)
    float* out;           // (B, N)  lrelu(BN(Y))  (slope 1: no activation)
    float* outT;          // (N, B) transposed copy or null
    int B, N;
    float eps, momentum, slope;
    int bf16_out;         // out / outT hold 16-bit values (operands of mixed-precision contractions): 1 bfloat16, 2 float16
};

constexpr int BN_MAXR = 16;  // rows per thread: B / RG with B <= 1024 and RG >= 64

template <int STRIP, int NT = 256>
struct StripGeom {
    static constexpr int CG = STRIP / 4, RG = NT / CG;
};

// per-column totals of the threads' 4-column partials: red[rg][c], then STRIP threads add the row groups in order
template <int STRIP, int NT>
__device__ __forceinline__ void strip_reduce(float* red, const float4& part, float* total, int tid) {
    constexpr int CG = StripGeom<STRIP, NT>::CG, RG = StripGeom<STRIP, NT>::RG;
    const int c0 = 4 * (tid % CG), rg = tid / CG;
    float* p = red + rg * STRIP + c0;
    p[0] = part.x; p[1] = part.y; p[2] = part.z; p[3] = part.w;
    __syncthreads();
    if (tid < STRIP) {
        float t = 0.f;
        for (int k = 0; k < RG; ++k) t += red[k * STRIP + tid];
        total[tid] = t;
    }
    __syncthreads();
}

// rows {rg + RG k} of the strip (one float4 per thread) -> the transposed copy, through a [RG][STRIP + 1] LDS tile:
// thread t then owns column t / (RG / 4) and rows 4 (t % (RG / 4)).. of the batch: one 16-byte store
template <int STRIP, int NT>
__device__ __forceinline__ void strip_transpose_out(float* tile, const float4& v, float* outT, int n0, int B, int k,
                                                    int tid, int bf16 = 0) {
    constexpr int CG = StripGeom<STRIP, NT>::CG, RG = StripGeom<STRIP, NT>::RG, LD = STRIP + 1;
    const int c0 = 4 * (tid % CG), rg = tid / CG;
    __syncthreads();  // the previous batch has been read out
    float* p = tile + rg * LD + c0;
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    __syncthreads();
    const int col = tid / (RG / 4), r4 = 4 * (tid % (RG / 4));
    const float4 o = make_float4(tile[r4 * LD + col], tile[(r4 + 1) * LD + col], tile[(r4 + 2) * LD + col],
                                 tile[(r4 + 3) * LD + col]);
    const size_t off = (size_t)(n0 + col) * B + (size_t)RG * k + r4;
    if (bf16) *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(outT) + off) = half_pack4(o, bf16);
    else *reinterpret_cast<float4*>(outT + off) = o;
}

template <int STRIP, int NT>
__global__ void __launch_bounds__(NT) tower_bn_forward_kernel(BnFwd a) {
    constexpr int CG = StripGeom<STRIP, NT>::CG, RG = StripGeom<STRIP, NT>::RG;
    __shared__ float red[RG * STRIP];
    __shared__ float tile[RG * (STRIP + 1)];
    __shared__ float csum[STRIP], cmean[STRIP], cinv[STRIP];
    const int tid = threadIdx.x;
    const int c0 = 4 * (tid % CG), rg = tid / CG;
    const int n0 = blockIdx.x * STRIP;
    const int nr = a.B / RG;
    const float4 bv = a.bias ? *reinterpret_cast<const float4*>(a.bias + n0 + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v[BN_MAXR];
#pragma unroll
    for (int k = 0; k < BN_MAXR; ++k) {
        v[k] = bv;
        if (k < nr) {
            const float* src = a.Y + (size_t)(rg + RG * k) * a.N + n0 + c0;
            for (int s0 = 0; s0 < a.S; s0 += 8) {  // the slices of a row eight at a time, all loads issued first
                float4 t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    t[j] = s0 + j < a.S ? *reinterpret_cast<const float4*>(src + (size_t)(s0 + j) * a.slice_stride)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < 8; ++j) {  // slice order: the sum does not depend on the grouping
                    v[k].x += t[j].x; v[k].y += t[j].y; v[k].z += t[j].z; v[k].w += t[j].w;
                }
            }
        }
    }
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < BN_MAXR; ++k) {
        if (k < nr) {
            s1.x += v[k].x; s1.y += v[k].y; s1.z += v[k].z; s1.w += v[k].w;
            if (a.Ysum) *reinterpret_cast<float4*>(a.Ysum + (size_t)(rg + RG * k) * a.N + n0 + c0) = v[k];
        }
    }
    strip_reduce<STRIP, NT>(red, s1, csum, tid);
    if (tid < STRIP) cmean[tid] = csum[tid] / (float)a.B;
    __syncthreads();
    const float4 mu = make_float4(cmean[c0], cmean[c0 + 1], cmean[c0 + 2], cmean[c0 + 3]);
    float4 s2 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < BN_MAXR; ++k) {  // two-pass variance: mean first, then the squared deviations
        if (k < nr) {
            const float dx = v[k].x - mu.x, dy = v[k].y - mu.y, dz = v[k].z - mu.z, dw = v[k].w - mu.w;
            s2.x = fmaf(dx, dx, s2.x); s2.y = fmaf(dy, dy, s2.y); s2.z = fmaf(dz, dz, s2.z); s2.w = fmaf(dw, dw, s2.w);
        }
    }
    strip_reduce<STRIP, NT>(red, s2, csum, tid);
    if (tid < STRIP) {
        const float var = csum[tid];
        const float inv = 1.0f / sqrtf(var / (float)a.B + a.eps);
        cinv[tid] = inv;
        a.mean[n0 + tid] = cmean[tid];
        a.invstd[n0 + tid] = inv;
        if (a.running_mean) {
            const float unb = var / (float)(a.B - 1);
            a.running_mean[n0 + tid] = (1.f - a.momentum) * a.running_mean[n0 + tid] + a.momentum * cmean[tid];
            a.running_var[n0 + tid] = (1.f - a.momentum) * a.running_var[n0 + tid] + a.momentum * unb;
        }
    }
    __syncthreads();
    const float4 inv = make_float4(cinv[c0], cinv[c0 + 1], cinv[c0 + 2], cinv[c0 + 3]);
    const float4 ga = *reinterpret_cast<const float4*>(a.gamma + n0 + c0);
    const float4 be = *reinterpret_cast<const float4*>(a.beta + n0 + c0);
#pragma unroll
    for (int k = 0; k < BN_MAXR; ++k) {
        if (k < nr) {
            float4 o;
            o.x = fmaf((v[k].x - mu.x) * inv.x, ga.x, be.x); o.y = fmaf((v[k].y - mu.y) * inv.y, ga.y, be.y);
            o.z = fmaf((v[k].z - mu.z) * inv.z, ga.z, be.z); o.w = fmaf((v[k].w - mu.w) * inv.w, ga.w, be.w);
            o.x = o.x > 0.f ? o.x : a.slope * o.x; o.y = o.y > 0.f ? o.y : a.slope * o.y;
            o.z = o.z > 0.f ? o.z : a.slope * o.z; o.w = o.w > 0.f ? o.w : a.slope * o.w;
            const size_t off = (size_t)(rg + RG * k) * a.N + n0 + c0;
            if (a.bf16_out) *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(a.out) + off) = half_pack4(o, a.bf16_out);
            else *reinterpret_cast<float4*>(a.out + off) = o;
            v[k] = o;
        }
    }
    if (a.outT) {
        for (int k = 0; k < nr; ++k) {
            float4 o = v[0];
#pragma unroll
            for (int j = 1; j < BN_MAXR; ++j)
                if (j == k) o = v[j];  // (a run-time index into the register array would put it in scratch)
            strip_transpose_out<STRIP, NT>(tile, o, a.outT, n0, a.B, k, tid, a.bf16_out);
        }
    }
}

struct BnBwd {
    const float* dout;    // (B, N) gradient w.r.t. the strip kernel's output (after the activation)
    const float* Y;       // (B, N) pre-normalisation output (what the forward normalised)
    const float* mean;    // (N)
    const float* invstd;  // (N)
    const float* gamma;
    const float* beta;    // needed for the activation's sign only (slope != 1)
    float* dY;            // (B, N) or null
    float* dYT;           // (N, B) or null
    float* dgamma;        // (N)
    float* dbeta;         // (N)
    float* dbias;         // (N): column sums of dY (the Linear bias in front of the BatchNorm), or null
    int B, N;
    float slope;
    int bf16_out;         // dY / dYT hold 16-bit values (operands of mixed-precision contractions): 1 bfloat16, 2 float16
};

template <int STRIP, int NT>
__global__ void __launch_bounds__(NT) tower_bn_backward_kernel(BnBwd a) {
    constexpr int CG = StripGeom<STRIP, NT>::CG, RG = StripGeom<STRIP, NT>::RG;
    __shared__ float red[RG * STRIP];
    __shared__ float tile[RG * (STRIP + 1)];
    __shared__ float c1[STRIP], c2[STRIP], c3[STRIP];
    const int tid = threadIdx.x;
    const int c0 = 4 * (tid % CG), rg = tid / CG;
    const int n0 = blockIdx.x * STRIP;
    const int nr = a.B / RG;
    const float4 mu = *reinterpret_cast<const float4*>(a.mean + n0 + c0);
    const float4 inv = *reinterpret_cast<const float4*>(a.invstd + n0 + c0);
    const float4 ga = *reinterpret_cast<const float4*>(a.gamma + n0 + c0);
    const float4 be = *reinterpret_cast<const float4*>(a.beta + n0 + c0);
    float4 yh[BN_MAXR], dh[BN_MAXR];  // normalised pre-activation, gradient behind the activation
#pragma unroll
    for (int k = 0; k < BN_MAXR; ++k) {
        yh[k] = dh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < nr) {
            yh[k] = *reinterpret_cast<const float4*>(a.Y + (size_t)(rg + RG * k) * a.N + n0 + c0);
            dh[k] = *reinterpret_cast<const float4*>(a.dout + (size_t)(rg + RG * k) * a.N + n0 + c0);
        }
    }
    // dh = dout * act'(h), column sums of dh and dh * yhat
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
#pragma unroll
    for (int k = 0; k < BN_MAXR; ++k) {
        if (k < nr) {
            float4 y = yh[k];
            y.x = (y.x - mu.x) * inv.x; y.y = (y.y - mu.y) * inv.y; y.z = (y.z - mu.z) * inv.z; y.w = (y.w - mu.w) * inv.w;
            float4 d = dh[k];
            d.x *= fmaf(y.x, ga.x, be.x) > 0.f ? 1.f : a.slope;
            d.y *= fmaf(y.y, ga.y, be.y) > 0.f ? 1.f : a.slope;
            d.z *= fmaf(y.z, ga.z, be.z) > 0.f ? 1.f : a.slope;
            d.w *= fmaf(y.w, ga.w, be.w) > 0.f ? 1.f : a.slope;
            yh[k] = y;
            dh[k] = d;
            s1.x += d.x; s1.y += d.y; s1.z += d.z; s1.w += d.w;
            s2.x = fmaf(d.x, y.x, s2.x); s2.y = fmaf(d.y, y.y, s2.y); s2.z = fmaf(d.z, y.z, s2.z); s2.w = fmaf(d.w, y.w, s2.w);
        }
    }
    strip_reduce<STRIP, NT>(red, s1, c1, tid);
    strip_reduce<STRIP, NT>(red, s2, c2, tid);
    if (tid < STRIP) {
        a.dbeta[n0 + tid] = c1[tid];
        a.dgamma[n0 + tid] = c2[tid];
    }
    // dY = gamma * invstd * (dh - mean(dh) - yhat * mean(dh * yhat))
    const float rB = 1.0f / (float)a.B;
    const float4 m1 = make_float4(c1[c0] * rB, c1[c0 + 1] * rB, c1[c0 + 2] * rB, c1[c0 + 3] * rB);
    const float4 m2 = make_float4(c2[c0] * rB, c2[c0 + 1] * rB, c2[c0 + 2] * rB, c2[c0 + 3] * rB);
    float4 sb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < BN_MAXR; ++k) {
        if (k < nr) {
            float4 dy;
            dy.x = ga.x * inv.x * (dh[k].x - m1.x - yh[k].x * m2.x);
            dy.y = ga.y * inv.y * (dh[k].y - m1.y - yh[k].y * m2.y);
            dy.z = ga.z * inv.z * (dh[k].z - m1.z - yh[k].z * m2.z);
            dy.w = ga.w * inv.w * (dh[k].w - m1.w - yh[k].w * m2.w);
            dh[k] = dy;
            sb.x += dy.x; sb.y += dy.y; sb.z += dy.z; sb.w += dy.w;
            if (a.dY) {
                const size_t off = (size_t)(rg + RG * k) * a.N + n0 + c0;
                if (a.bf16_out) *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(a.dY) + off) = half_pack4(dy, a.bf16_out);
                else *reinterpret_cast<float4*>(a.dY + off) = dy;
            }
        }
    }
    strip_reduce<STRIP, NT>(red, sb, c3, tid);
    if (a.dbias && tid < STRIP) a.dbias[n0 + tid] = c3[tid];
    if (a.dYT) {
        for (int k = 0; k < nr; ++k) {
            float4 o = dh[0];
#pragma unroll
            for (int j = 1; j < BN_MAXR; ++j)
                if (j == k) o = dh[j];
            strip_transpose_out<STRIP, NT>(tile, o, a.dYT, n0, a.B, k, tid, a.bf16_out);
        }
    }
}

// Wide layers (>= 4096 columns): 32-column strips in 512-thread workgroups - a row of the strip is one whole 128-byte
// line (with 16-column strips the two halves of a line went to two workgroups, as a rule on two XCDs: every line
// crossed the fabric twice) and 8 waves keep the rows-per-thread count at 16 float4 (8192 columns = 256 workgroups,
// one per CU; every tower width is a multiple of 128, so no wide layer needs a narrower strip). Narrower strips below
// 4096 columns so that a 512-wide layer spreads over 128 (4 columns, batch a multiple of 256) or 64 (8 columns)
// workgroups instead of 16.
inline int launch_bn_forward(const BnFwd& f, hipStream_t s) {
    if (f.B % 128 || f.B > 1024 || f.N % (f.N >= 4096 ? 32 : 16)) return NSVD_EINVAL;
    if (f.N >= 4096) hipLaunchKernelGGL((tower_bn_forward_kernel<32, 512>), dim3(f.N / 32), dim3(512), 0, s, f);
    else if (f.B % 256 == 0) hipLaunchKernelGGL((tower_bn_forward_kernel<4, 256>), dim3(f.N / 4), dim3(256), 0, s, f);
    else hipLaunchKernelGGL((tower_bn_forward_kernel<8, 256>), dim3(f.N / 8), dim3(256), 0, s, f);
    NSVD_CHECK_LAUNCH();
    return 0;
}
inline int launch_bn_backward(const BnBwd& b, hipStream_t s) {
    if (b.B % 128 || b.B > 1024 || b.N % (b.N >= 4096 ? 32 : 16)) return NSVD_EINVAL;
    if (b.N >= 4096) hipLaunchKernelGGL((tower_bn_backward_kernel<32, 512>), dim3(b.N / 32), dim3(512), 0, s, b);
    else if (b.B % 256 == 0) hipLaunchKernelGGL((tower_bn_backward_kernel<4, 256>), dim3(b.N / 4), dim3(256), 0, s, b);
    else hipLaunchKernelGGL((tower_bn_backward_kernel<8, 256>), dim3(b.N / 8), dim3(256), 0, s, b);
    NSVD_CHECK_LAUNCH();
    return 0;
}

// prof: bracket the contraction for bench.py
inline int launch_gemm(const GemmNT& g, hipStream_t s, bool prof = false) {
    if (g.M % 128 || g.N % 128 || g.S < 1 || g.K % (32 * g.S)) return NSVD_EINVAL;
    const dim3 grid((g.M / 128) * (g.N / 128) * g.S);
    if (prof) nsvd_prof_begin(s);
    hipLaunchKernelGGL(tower_gemm_nt_kernel, grid, dim3(256), 0, s, g);
    if (prof) nsvd_prof_end(s);
    NSVD_CHECK_LAUNCH();
    return 0;
}

// split-K of the second forward GEMM: as many slices as it takes to give every CU a tile (K / S a multiple of 32)
inline int fwd2_slices(int B, int d1, int d2) {
    const int tiles = (B / 128) * (d2 / 128);
    int S = 1;
    while (S < 16 && tiles * S < 256 && d1 % (64 * S) == 0) S *= 2;
    return S;
}

// the same for the mixed-precision contraction (256 x 128 tiles, gemm16.h; nt towers per launch): slices until the launch
// has 256 workgroups
inline int fwd2_slices16(int nt, int B, int d1, int d2) {
    const int tiles = nt * (B / 256) * (d2 / 128);
    int S = 1;
    while (S < 16 && tiles > 0 && tiles * S < 256 && d1 % (128 * S) == 0) S *= 2;
    return S;
}

struct TowerWs {
    float *Y1, *A1, *A1T, *Y2p, *Y2, *XT, *W2T, *dY2, *dY2T, *dA1, *dY1T;
    float *mean1, *inv1, *mean2, *inv2;
    void *hA, *hB;  // bfloat16 copies of the operands that are cast per call (mixed-precision mode)
    size_t capA, capB;  // their capacities in bfloat16 values
    size_t bytes;
};

inline TowerWs carve_tower(int B, int d0, int d1, int d2, void* base) {
    TowerWs w;
    memset(&w, 0, sizeof(w));
    NsvdArena a(base);
    int S = fwd2_slices(B, d1, d2);  // (the larger of the two modes' slice counts: one layout for both)
    if (B % 256 == 0 && fwd2_slices16(1, B, d1, d2) > S) S = fwd2_slices16(1, B, d1, d2);
    w.Y1 = a.take((size_t)B * d1);
    w.A1 = a.take((size_t)B * d1);
    w.A1T = a.take((size_t)B * d1);
    w.Y2p = a.take((size_t)S * B * d2);
    w.Y2 = a.take((size_t)B * d2);
    w.XT = a.take((size_t)B * d0);
    w.W2T = a.take((size_t)d1 * d2);
    w.dY2 = a.take((size_t)B * d2);
    w.dY2T = a.take((size_t)B * d2);
    w.dA1 = a.take((size_t)B * d1);
    w.dY1T = a.take((size_t)B * d1);
    w.mean1 = a.take(d1);
    w.inv1 = a.take(d1);
    w.mean2 = a.take(d2);
    w.inv2 = a.take(d2);
    {   // the operands cast per call (every other one is written as bfloat16 by its producer): X (B, d0) on the A
        // side; the master weights W1 (d1, d0) and W2 (d2, d1), one after the other, on the B side. Two bytes per value.
        w.capA = (size_t)B * d0;
        w.capB = (size_t)d1 * (d0 > d2 ? d0 : d2);
        w.hA = a.take((w.capA + 1) / 2);
        w.hB = a.take((w.capB + 1) / 2);
    }
    w.bytes = a.off;
    return w;
}

inline bool tower_shape_ok(int B, int d0, int d1, int d2) {
    return B > 0 && B <= 1024 && B % 128 == 0 && d0 > 0 && d0 % 128 == 0 && d1 > 0 && d1 % 128 == 0 && d2 > 0 &&
           d2 % 128 == 0;
}


// =====================================================================================================================
// MIXED PRECISION (gemm_bf16 != 0): the counterpart of the reference's autocast branch
// (examples/cdk/sketchy/main_sketchy.py:161,182: Linear outputs and BatchNorm / activation outputs are HALF tensors
// there, statistics and master weights float32). Here the half type is bfloat16:
//   stored as bfloat16: X, W1, W2 (copies of the float32 masters), Y1 = X W1^T + b1, A1 = lrelu(BN1(Y1)),
//                       dY2 = BN2'(dZ), dA1 = dY2 W2, dY1 = BN1'(lrelu'(dA1))
//   float32:            every accumulation, BatchNorm statistics, Y2 / Z / dZ (the narrow end), all parameter gradients
// The five contractions run on gemm16.h (bf16 MFMA, 256 x 128 tiles) in the operand forms that need NO transposed copy
// of anything; both towers of a step go through every launch together (nt = 2: twice the workgroups per launch).
//   forward   Y1h = Xh W1h^T + b1                 T T   (B, d1) bf16
//             A1h = lrelu(BN1(Y1h))               strip kernel over 64 columns (one 128-byte line of bf16 per row)
//             Y2  = A1h W2h^T (+ b2)              T T   split-K slices (float32), summed by tower_sum_slices_kernel
//             Z   = BN2(Y2)                       float32 strip kernel
//   backward  dY2h = BN2'(dZ)                     float32 strip kernel, bfloat16 output
//             dW2 = dY2h^T A1h                    S S   (contraction over the batch: both operands as stored)
//             dA1h = dY2h W2h                     T S   (W2 as stored)
//             dY1h = BN1'(lrelu'(dA1h))           strip kernel
//             dW1 = dY1h^T Xh                     S S
// Shapes: B, d1, d2 multiples of 256, d0 a multiple of 128, B <= 1024 (nsvd_tower_mixed_supported).
typedef unsigned short bf16_t;

__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
// (opaque: the compiler may not keep the eight floats of a row alive from one phase of a strip kernel to the next - the
// strip lives in registers PACKED, 4 registers per row, and is unpacked again where it is used)
template <bool F16 = false>
__device__ __forceinline__ void unpack8_fresh(uint4 u, float (&v)[8]) {
    asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z), "+v"(u.w));
    using nsvd_g16::h_hi;
    using nsvd_g16::h_lo;
    v[0] = h_lo<F16>(u.x); v[1] = h_hi<F16>(u.x);
    v[2] = h_lo<F16>(u.y); v[3] = h_hi<F16>(u.y);
    v[4] = h_lo<F16>(u.z); v[5] = h_hi<F16>(u.z);
    v[6] = h_lo<F16>(u.w); v[7] = h_hi<F16>(u.w);
}
__device__ __forceinline__ void unpack8(const uint4& u, float (&v)[8]) {
    v[0] = bf16_lo(u.x); v[1] = bf16_hi(u.x); v[2] = bf16_lo(u.y); v[3] = bf16_hi(u.y);
    v[4] = bf16_lo(u.z); v[5] = bf16_hi(u.z); v[6] = bf16_lo(u.w); v[7] = bf16_hi(u.w);
}
template <bool F16 = false>
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    using nsvd_g16::pack_h;
    return make_uint4(pack_h<F16>(v[0], v[1]), pack_h<F16>(v[2], v[3]), pack_h<F16>(v[4], v[5]), pack_h<F16>(v[6], v[7]));
}

// 16-byte write-through store (sc1): a strip's 32 MB of output leaves for memory while the kernel runs instead of sitting
// dirty in the XCDs' L2s until the kernel-end write-back (MI355X_MICROARCH.md, stores of each flavour; gemm16.h's
// epilogue does the same)
__device__ __forceinline__ void store16_wt(void* dst, const uint4& v) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 vv = {v.x, v.y, v.z, v.w};
    // (s_nop 1 inside the string: hipcc pads nothing behind an asm store - its next instruction may overwrite the
    // data registers before the store has read them: intermittent wrong elements, found in round 6)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(vv) : "memory");
}

// several float32 -> bfloat16 casts in one launch (blockIdx.y = segment)
struct CastList {
    const float4* in[6];
    uint4* out[6];
    size_t n8[6];
};
template <bool F16>
__global__ void __launch_bounds__(256) tower_cast_list_kernel(CastList c) {
    using nsvd_g16::pack_h;
    const int k = blockIdx.y;
    const float4* in = c.in[k];
    uint4* out = c.out[k];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < c.n8[k]; i += (size_t)gridDim.x * 256) {
        const float4 a = in[2 * i], b = in[2 * i + 1];
        out[i] = make_uint4(pack_h<F16>(a.x, a.y), pack_h<F16>(a.z, a.w), pack_h<F16>(b.x, b.y), pack_h<F16>(b.z, b.w));
    }
}

// BatchNorm strips on bfloat16 activations: one workgroup (512 threads) = 64 columns (one 128-byte line per row) x all
// B rows in registers; thread t owns columns 8 (t & 7) .. + 7 of rows (t >> 3) + 64 k, k < B / 64 <= 16.
// Column totals in a fixed order: 64 row groups per column through LDS, added in order by one thread per column.
constexpr int BN16_STRIP = 64, BN16_NT = 512, BN16_RG = 64, BN16_MAXR = 16;

__device__ __forceinline__ void bn16_reduce(float* red, const float (&part)[8], float* total, int tid) {
    const int c0 = 8 * (tid & 7), rg = tid >> 3;
    float* p = red + rg * BN16_STRIP + c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = part[j];
    __syncthreads();
    if (tid < BN16_STRIP) {
        float t = 0.f;
        for (int k = 0; k < BN16_RG; ++k) t += red[k * BN16_STRIP + tid];
        total[tid] = t;
    }
    __syncthreads();
}

struct Bn16Fwd {
    const bf16_t* Y[2];   // (B, N) bfloat16 pre-normalisation output (bias included)
    const float* gamma[2];
    const float* beta[2];
    float* running_mean[2];  // updated in place (null: no running statistics)
    float* running_var[2];
    float* mean[2];       // (N) saved for the backward
    float* invstd[2];
    bf16_t* out[2];       // (B, N) bfloat16  lrelu(BN(Y))
    int B, N;
    float eps, momentum, slope;
};

template <bool F16>
__global__ void __launch_bounds__(BN16_NT) tower_bn16_forward_kernel(Bn16Fwd a) {
    __shared__ float red[BN16_RG * BN16_STRIP];
    __shared__ float csum[BN16_STRIP], cmean[BN16_STRIP], cinv[BN16_STRIP];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int c0 = 8 * (tid & 7), rg = tid >> 3;
    const int n0 = blockIdx.x * BN16_STRIP;
    const int nr = a.B / BN16_RG;
    const bf16_t* Y = a.Y[t];
    uint4 raw[BN16_MAXR];
#pragma unroll
    for (int k = 0; k < BN16_MAXR; ++k)
        if (k < nr) raw[k] = *reinterpret_cast<const uint4*>(Y + (size_t)(rg + BN16_RG * k) * a.N + n0 + c0);
    float s1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = 0.f;
#pragma unroll
    for (int k = 0; k < BN16_MAXR; ++k)
        if (k < nr) {
            float v[8];
            unpack8_fresh<F16>(raw[k], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) s1[j] += v[j];
        }
    bn16_reduce(red, s1, csum, tid);
    if (tid < BN16_STRIP) cmean[tid] = csum[tid] / (float)a.B;
    __syncthreads();
    float mu[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mu[j] = cmean[c0 + j];
        s2[j] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < BN16_MAXR; ++k)  // two-pass variance: mean first, then the squared deviations
        if (k < nr) {
            float v[8];
            unpack8_fresh<F16>(raw[k], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[j] - mu[j];
                s2[j] = fmaf(d, d, s2[j]);
            }
        }
    bn16_reduce(red, s2, csum, tid);
    if (tid < BN16_STRIP) {
        const float var = csum[tid];
        const float inv = 1.0f / sqrtf(var / (float)a.B + a.eps);
        cinv[tid] = inv;
        a.mean[t][n0 + tid] = cmean[tid];
        a.invstd[t][n0 + tid] = inv;
        if (a.running_mean[t]) {
            const float unb = var / (float)(a.B - 1);
            a.running_mean[t][n0 + tid] = (1.f - a.momentum) * a.running_mean[t][n0 + tid] + a.momentum * cmean[tid];
            a.running_var[t][n0 + tid] = (1.f - a.momentum) * a.running_var[t][n0 + tid] + a.momentum * unb;
        }
    }
    __syncthreads();
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = cinv[c0 + j];
        sh[j] = a.gamma[t][n0 + c0 + j];
    }
    float be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) be[j] = a.beta[t][n0 + c0 + j];
    bf16_t* out = a.out[t];
#pragma unroll
    for (int k = 0; k < BN16_MAXR; ++k)
        if (k < nr) {
            float v[8];
            unpack8_fresh<F16>(raw[k], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float o = fmaf((v[j] - mu[j]) * sc[j], sh[j], be[j]);
                v[j] = o > 0.f ? o : a.slope * o;
            }
            store16_wt(out + (size_t)(rg + BN16_RG * k) * a.N + n0 + c0, pack8<F16>(v));
        }
}

struct Bn16Bwd {
    const bf16_t* dout[2];  // (B, N) bfloat16 gradient w.r.t. the strip's output (behind the activation)
    const bf16_t* Y[2];     // (B, N) bfloat16 pre-normalisation output
    const float* mean[2];
    const float* invstd[2];
    const float* gamma[2];
    const float* beta[2];
    bf16_t* dY[2];          // (B, N) bfloat16
    float* dgamma[2];
    float* dbeta[2];
    float* dbias[2];        // column sums of the (unrounded) dY
    float* sumsq[2];        // null, or one float per workgroup (N / 64 per tower): the sum of the squares of the 3 x 64
                            // bias / BatchNorm-weight gradients it wrote (clip_grad_norm_ without a pass over them)
    int B, N;
    float slope;
};

template <bool F16>
__global__ void __launch_bounds__(BN16_NT) tower_bn16_backward_kernel(Bn16Bwd a) {
    __shared__ float red[BN16_RG * BN16_STRIP];
    __shared__ float c1[BN16_STRIP], c2[BN16_STRIP], c3[BN16_STRIP];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int c0 = 8 * (tid & 7), rg = tid >> 3;
    const int n0 = blockIdx.x * BN16_STRIP;
    const int nr = a.B / BN16_RG;
    float mu[8], inv[8], ga[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mu[j] = a.mean[t][n0 + c0 + j];
        inv[j] = a.invstd[t][n0 + c0 + j];
        ga[j] = a.gamma[t][n0 + c0 + j];
        be[j] = a.beta[t][n0 + c0 + j];
    }
    uint4 yr[BN16_MAXR], dr[BN16_MAXR];
#pragma unroll
    for (int k = 0; k < BN16_MAXR; ++k)
        if (k < nr) {
            const size_t off = (size_t)(rg + BN16_RG * k) * a.N + n0 + c0;
            yr[k] = *reinterpret_cast<const uint4*>(a.Y[t] + off);
            dr[k] = *reinterpret_cast<const uint4*>(a.dout[t] + off);
        }
    // dh = dout * act'(h); column sums of dh and dh * yhat
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
#pragma unroll
    for (int k = 0; k < BN16_MAXR; ++k)
        if (k < nr) {
            float y[8], d[8];
            unpack8_fresh<F16>(yr[k], y);
            unpack8_fresh<F16>(dr[k], d);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float yh = (y[j] - mu[j]) * inv[j];
                const float dh = d[j] * (fmaf(yh, ga[j], be[j]) > 0.f ? 1.f : a.slope);
                s1[j] += dh;
                s2[j] = fmaf(dh, yh, s2[j]);
            }
        }
    bn16_reduce(red, s1, c1, tid);
    bn16_reduce(red, s2, c2, tid);
    if (tid < BN16_STRIP) {
        a.dbeta[t][n0 + tid] = c1[tid];
        a.dgamma[t][n0 + tid] = c2[tid];
    }
    const float rB = 1.0f / (float)a.B;
    float m1[8], m2[8], sb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        m1[j] = c1[c0 + j] * rB;
        m2[j] = c2[c0 + j] * rB;
        sb[j] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < BN16_MAXR; ++k)
        if (k < nr) {
            float y[8], d[8];
            unpack8_fresh<F16>(yr[k], y);
            unpack8_fresh<F16>(dr[k], d);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float yh = (y[j] - mu[j]) * inv[j];
                const float dh = d[j] * (fmaf(yh, ga[j], be[j]) > 0.f ? 1.f : a.slope);
                const float dy = ga[j] * inv[j] * (dh - m1[j] - yh * m2[j]);
                sb[j] += dy;
                d[j] = dy;
            }
            store16_wt(a.dY[t] + (size_t)(rg + BN16_RG * k) * a.N + n0 + c0, pack8<F16>(d));
        }
    bn16_reduce(red, sb, c3, tid);
    if (tid < BN16_STRIP) a.dbias[t][n0 + tid] = c3[tid];
    if (a.sumsq[t] && tid < 64) {  // (BN16_STRIP == 64: one wave holds the strip's columns; butterfly = fixed order)
        float q = fmaf(c1[tid], c1[tid], fmaf(c2[tid], c2[tid], c3[tid] * c3[tid]));
        q = nsvd_wave_sum(q);
        if (tid == 0) a.sumsq[t][blockIdx.x] = q;
    }
}

inline bool tower16_shape_ok(int B, int d0, int d1, int d2) {
    return tower_shape_ok(B, d0, d1, d2) && B % 256 == 0 && d1 % 256 == 0 && d2 % 256 == 0;
}

// the bfloat16 tensors of a mixed-precision tower, laid over the float32 layout's buffers (each at least twice as large)
struct Tower16 {
    bf16_t *Xh, *W1h, *W2h, *Y1h, *A1h, *dY2h, *dA1h, *dY1h;
};
inline Tower16 views16(const TowerWs& w) {
    Tower16 v;
    v.Xh = (bf16_t*)w.hA;      // capA = B d0 values
    v.W1h = (bf16_t*)w.hB;     // capB >= d1 d0 values
    v.W2h = (bf16_t*)w.W2T;    // d1 d2 floats
    v.Y1h = (bf16_t*)w.Y1;
    v.A1h = (bf16_t*)w.A1;
    v.dY2h = (bf16_t*)w.dY2;
    v.dA1h = (bf16_t*)w.dA1;
    v.dY1h = (bf16_t*)w.dY1T;
    return v;
}

// The wide layer with BatchNorm inside the contraction's epilogue (tower_col.h: no Y1h / dA1h round trip, no strip
// launches) where its recovery of the normalised value from the stored activation is defined: slope > 0. Otherwise (and
// with NSVD_TOWER16_FUSED=0, for A/B measurements) the contraction + strip pairs below.
inline bool tower16_fused(int B, int d0, int d1, int d2, float slope) {
    const char* e = getenv("NSVD_TOWER16_FUSED");  // (read per call: the tests switch forms inside one process)
    if (e && e[0] == '0') return false;
    return slope >= 1e-3f && nsvd_tcol::shape_ok(B, d1, d0) && nsvd_tcol::shape_ok(B, d1, d2);
}

// gemm_bf16 flag bits: 1 = mixed precision; 2 = the bfloat16 copies of W1 / W2 in the workspace are current (written by
// the previous step's optimiser kernel, cdk_step.hip): the forward does not cast them again
constexpr int MIXED_WEIGHTS_READY = 2;
// bit 4 (NSVD_TOWER16_F16 = 16): the half type is IEEE float16 instead of bfloat16

// the <true> (IEEE float16) or <false> (bfloat16) instance of a `template <bool F16>` kernel
#define TOWER_LAUNCH_HALF(kernel, f16, grid, block, s, arg)                     \
    do {                                                                        \
        if (f16) hipLaunchKernelGGL(kernel<true>, grid, block, 0, s, arg);      \
        else hipLaunchKernelGGL(kernel<false>, grid, block, 0, s, arg);         \
        NSVD_CHECK_LAUNCH();                                                    \
    } while (0)

// tiles (= sum-of-squares partials) of the two weight-gradient contractions in mixed precision: dW2's, then dW1's
inline int sumsq_count16(int d0, int d1, int d2) { return (d2 / 256) * (d1 / 128) + (d1 / 256) * (d0 / 128); }

// One call over nt <= 2 towers of one shape, each with a workspace of its own. Every entry point builds one at its top
// (tower_call, then tower_forward / tower_backward with that side's tensors), and the launch sequences below are its
// members; the workspaces are carved there and nowhere else. float32 calls have nt = 1; mixed-precision calls put their
// nt towers through every launch together.
struct TowerCall {
    int nt, B, d0, d1, d2;
    float slope, eps, momentum;
    int update_running, flags, phase;
    bool mixed, wide_only, fused;  // fused: tower16_fused, asked once per call
    int f16;                       // the half type is IEEE float16 (0: bfloat16)
    int S;                         // split-K slices of the second forward contraction, in this call's mode
    const float* x[2];
    const nsvd_tower_params* p[2];
    float* z[2];                        // forward
    const float* dz[2];                 // backward
    const nsvd_tower_params* grads[2];
    float* sumsq[2];                    // null: no sums of squares
    TowerWs w[2];
    Tower16 v[2];
    hipStream_t s;

    BnFwd bn2_forward_desc(int t, bool bias_here) const;
    BnBwd bn2_backward_desc(int t, int out16) const;
    int forward_narrow_end() const;
    int forward16() const;
    int forward32() const;
    int backward16() const;
    int backward32() const;
};

// Z = BN2(Y2), from the summed Y2 in the workspace. bias_here: b2 joins in the strip kernel, which writes the biased sum
// back for the backward (second half of a hidden-width-sharded tower: Y2 holds the all-reduced partial products)
BnFwd TowerCall::bn2_forward_desc(int t, bool bias_here) const {
    BnFwd f;
    memset(&f, 0, sizeof(f));
    f.Y = w[t].Y2; f.S = 1; f.gamma = p[t]->g2; f.beta = p[t]->be2;
    if (bias_here) {
        f.bias = p[t]->b2;
        f.Ysum = w[t].Y2;
    }
    f.running_mean = update_running ? p[t]->rm2 : nullptr; f.running_var = update_running ? p[t]->rv2 : nullptr;
    f.mean = w[t].mean2; f.invstd = w[t].inv2; f.out = z[t]; f.outT = nullptr; f.B = B; f.N = d2;
    f.eps = eps; f.momentum = momentum; f.slope = 1.0f;
    return f;
}

// dY2 = BN2'(dZ), db2 = its column sums. out16 = 0: float32 dY2 and dY2^T; 1 / 2: bfloat16 / float16 dY2 alone (the
// Tower16 view dY2h of the same buffer)
BnBwd TowerCall::bn2_backward_desc(int t, int out16) const {
    BnBwd b;
    memset(&b, 0, sizeof(b));
    b.dout = dz[t]; b.Y = w[t].Y2; b.mean = w[t].mean2; b.invstd = w[t].inv2; b.gamma = p[t]->g2; b.beta = p[t]->be2;
    b.dY = w[t].dY2; b.dYT = out16 ? nullptr : w[t].dY2T;
    b.dgamma = grads[t]->g2; b.dbeta = grads[t]->be2; b.dbias = grads[t]->b2;
    b.B = B; b.N = d2; b.slope = 1.0f; b.bf16_out = out16;
    return b;
}

// The narrow end of either forward: Y2 = b2 + the sum of the S split-K partials, then Z = BN2(Y2). phase 1 stops behind
// the sum (no bias: this rank's partial Y2 is in the workspace, nsvd_tower_y2_offset); phase 2 is the BatchNorm alone,
// on the all-reduced Y2, with the bias joining there.
int TowerCall::forward_narrow_end() const {
    for (int t = 0; t < nt && phase != 2; ++t) {
        const size_t n4 = (size_t)B * d2 / 4;
        hipLaunchKernelGGL(tower_sum_slices_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, w[t].Y2p,
                           (size_t)B * d2, S, phase == 1 ? nullptr : p[t]->b2, w[t].Y2, d2, n4);
        NSVD_CHECK_LAUNCH();
    }
    if (phase == 1) return 0;
    for (int t = 0; t < nt; ++t) {
        const int rc = launch_bn_forward(bn2_forward_desc(t, phase == 2), s);
        if (rc) return rc;
    }
    return 0;
}

int TowerCall::forward16() const {
    int rc = 0;
    {   // casts: X always; the weights unless their copies are current
        CastList c;
        memset(&c, 0, sizeof(c));
        int n = 0;
        size_t maxn = 0;
        for (int t = 0; t < nt; ++t) {
            c.in[n] = (const float4*)x[t]; c.out[n] = (uint4*)v[t].Xh; c.n8[n] = (size_t)B * d0 / 8; ++n;
            if (!(flags & MIXED_WEIGHTS_READY)) {
                c.in[n] = (const float4*)p[t]->W1; c.out[n] = (uint4*)v[t].W1h; c.n8[n] = (size_t)d1 * d0 / 8; ++n;
                c.in[n] = (const float4*)p[t]->W2; c.out[n] = (uint4*)v[t].W2h; c.n8[n] = (size_t)d2 * d1 / 8; ++n;
            }
        }
        for (int k = 0; k < n; ++k) maxn = c.n8[k] > maxn ? c.n8[k] : maxn;
        size_t blocks = (maxn + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        TOWER_LAUNCH_HALF(tower_cast_list_kernel, f16, dim3((unsigned)blocks, n), dim3(256), s, c);
    }
    nsvd_g16::Args g;
    if (fused) {
        // A1h = lrelu(BN1(Xh W1h^T + b1)) in ONE launch (whole columns per workgroup: tower_col.h)
        nsvd_tcol::Args c;
        memset(&c, 0, sizeof(c));
        for (int t = 0; t < nt; ++t) {
            nsvd_tcol::Prob& q = c.p[t];
            q.A = v[t].Xh; q.W = v[t].W1h; q.bias = p[t]->b1; q.gamma = p[t]->g1; q.beta = p[t]->be1;
            q.running_mean = update_running ? p[t]->rm1 : nullptr;
            q.running_var = update_running ? p[t]->rv1 : nullptr;
            q.mean = w[t].mean1; q.invstd = w[t].inv1; q.out = v[t].A1h;
        }
        c.nt = nt; c.M = B; c.N = d1; c.K = d0; c.eps = eps; c.momentum = momentum; c.slope = slope;
        c.f16 = f16;
        nsvd_prof_begin(s);  // bench.py --config cfg5 --amp brackets this launch (nsvd_profile_next_forward)
        rc = nsvd_tcol::launch<false>(c, s);
        nsvd_prof_end(s);
        if (rc) return rc;
    } else {
        // Y1h = Xh W1h^T + b1
        memset(&g, 0, sizeof(g));
        for (int t = 0; t < nt; ++t) {
            g.p[t].A = v[t].Xh; g.p[t].B = v[t].W1h; g.p[t].C = v[t].Y1h; g.p[t].bias = p[t]->b1;
        }
        g.nprob = nt; g.K = d0; g.S = 1; g.f16 = f16;
        nsvd_g16::set_uniform(g, B, d1, d0, d0, d1);
        nsvd_prof_begin(s);  // bench.py --config cfg5 --amp brackets this contraction (nsvd_profile_next_forward)
        rc = nsvd_g16::launch(g, false, false, true, s);
        nsvd_prof_end(s);
        if (rc) return rc;
        // A1h = lrelu(BN1(Y1h))
        Bn16Fwd f;
        memset(&f, 0, sizeof(f));
        for (int t = 0; t < nt; ++t) {
            f.Y[t] = v[t].Y1h; f.gamma[t] = p[t]->g1; f.beta[t] = p[t]->be1;
            f.running_mean[t] = update_running ? p[t]->rm1 : nullptr;
            f.running_var[t] = update_running ? p[t]->rv1 : nullptr;
            f.mean[t] = w[t].mean1; f.invstd[t] = w[t].inv1; f.out[t] = v[t].A1h;
        }
        f.B = B; f.N = d1; f.eps = eps; f.momentum = momentum; f.slope = slope;
        TOWER_LAUNCH_HALF(tower_bn16_forward_kernel, f16, dim3(d1 / BN16_STRIP, nt), dim3(BN16_NT), s, f);
    }
    // Y2 partial products, split-K
    memset(&g, 0, sizeof(g));
    for (int t = 0; t < nt; ++t) {
        g.p[t].A = v[t].A1h; g.p[t].B = v[t].W2h; g.p[t].C = w[t].Y2p;
    }
    g.nprob = nt; g.K = d1; g.S = S; g.f16 = f16;
    nsvd_g16::set_uniform(g, B, d2, d1, d1, d2);
    g.slice_stride = (long)B * d2;
    rc = nsvd_g16::launch(g, false, false, false, s);
    if (rc) return rc;
    if (wide_only) return 0;  // the narrow end is the caller's (cdk_narrow.hip)
    return forward_narrow_end();
}

int TowerCall::forward32() const {
    int rc = 0;
    GemmNT g;
    BnFwd f;
    // Y1 = X W1^T + b1
    memset(&g, 0, sizeof(g));
    g.A = x[0]; g.lda = d0; g.B = p[0]->W1; g.ldb = d0; g.C = w[0].Y1; g.ldc = d1; g.bias = p[0]->b1;
    g.M = B; g.N = d1; g.K = d0; g.S = 1;
    rc = launch_gemm(g, s, true);  // bench.py --config cfg5 brackets this contraction (nsvd_profile_next_forward)
    if (rc) return rc;
    // A1 = lrelu(BN1(Y1)), A1^T
    memset(&f, 0, sizeof(f));
    f.Y = w[0].Y1; f.S = 1; f.gamma = p[0]->g1; f.beta = p[0]->be1;
    f.running_mean = update_running ? p[0]->rm1 : nullptr; f.running_var = update_running ? p[0]->rv1 : nullptr;
    f.mean = w[0].mean1; f.invstd = w[0].inv1; f.out = w[0].A1; f.outT = w[0].A1T; f.B = B; f.N = d1;
    f.eps = eps; f.momentum = momentum; f.slope = slope;
    rc = launch_bn_forward(f, s);
    if (rc) return rc;
    // Y2 = A1 W2^T, split-K partials (b2 joins in the narrow end)
    memset(&g, 0, sizeof(g));
    g.A = w[0].A1; g.lda = d1; g.B = p[0]->W2; g.ldb = d1; g.C = w[0].Y2p; g.ldc = d2; g.slice_stride = (size_t)B * d2;
    g.M = B; g.N = d2; g.K = d1; g.S = S;
    rc = launch_gemm(g, s);
    if (rc) return rc;
    return forward_narrow_end();
}

int TowerCall::backward16() const {
    int rc = 0;
    for (int t = 0; t < nt && !wide_only; ++t) {  // dY2h = BN2'(dZ), db2
        rc = launch_bn_backward(bn2_backward_desc(t, 1 + f16), s);
        if (rc) return rc;
    }
    // the squares of the b1 / g1 / be1 gradients, behind the contractions' partials
    float* small_sumsq[2];
    for (int t = 0; t < nt; ++t) {
        const bool want = sumsq[t] && (flags & NSVD_TOWER16_SMALL_SUMSQ);
        small_sumsq[t] = want ? sumsq[t] + sumsq_count16(d0, d1, d2) : nullptr;
    }
    nsvd_g16::Args g;
    if (fused) {
        // dY1h = BN1'(lrelu'(dY2h W2h)), dgamma1, dbeta1, db1 in ONE launch (tower_col.h)
        nsvd_tcol::Args c;
        memset(&c, 0, sizeof(c));
        for (int t = 0; t < nt; ++t) {
            nsvd_tcol::Prob& q = c.p[t];
            q.A = v[t].dY2h; q.W = v[t].W2h; q.gamma = p[t]->g1; q.beta = p[t]->be1; q.invstd = w[t].inv1;
            q.out = v[t].dY1h; q.A1 = v[t].A1h; q.dgamma = grads[t]->g1; q.dbeta = grads[t]->be1; q.dbias = grads[t]->b1;
            q.sumsq = small_sumsq[t];
        }
        c.nt = nt; c.M = B; c.N = d1; c.K = d2; c.slope = slope;
        c.f16 = f16;
        rc = nsvd_tcol::launch<true>(c, s);
        if (rc) return rc;
    } else {
        // dA1h = dY2h W2h
        memset(&g, 0, sizeof(g));
        for (int t = 0; t < nt; ++t) {
            g.p[t].A = v[t].dY2h; g.p[t].B = v[t].W2h; g.p[t].C = v[t].dA1h;
        }
        g.nprob = nt; g.K = d2; g.S = 1; g.f16 = f16;
        nsvd_g16::set_uniform(g, B, d1, d2, d1, d1);
        rc = nsvd_g16::launch(g, false, true, true, s);
        if (rc) return rc;
        // dY1h = BN1'(lrelu'(dA1h)), db1
        Bn16Bwd b;
        memset(&b, 0, sizeof(b));
        for (int t = 0; t < nt; ++t) {
            b.dout[t] = v[t].dA1h; b.Y[t] = v[t].Y1h; b.mean[t] = w[t].mean1; b.invstd[t] = w[t].inv1;
            b.gamma[t] = p[t]->g1; b.beta[t] = p[t]->be1; b.dY[t] = v[t].dY1h; b.dgamma[t] = grads[t]->g1;
            b.dbeta[t] = grads[t]->be1; b.dbias[t] = grads[t]->b1;
            b.sumsq[t] = small_sumsq[t];
        }
        b.B = B; b.N = d1; b.slope = slope;
        TOWER_LAUNCH_HALF(tower_bn16_backward_kernel, f16, dim3(d1 / BN16_STRIP, nt), dim3(BN16_NT), s, b);
    }
    // dW2 = dY2h^T A1h and dW1 = dY1h^T Xh of every tower in ONE launch (same operand forms, same contraction length B,
    // different output shapes): a kernel boundary of these launches costs as much as a third of their MFMA work
    memset(&g, 0, sizeof(g));
    for (int t = 0; t < nt; ++t) {
        nsvd_g16::Prob& q2 = g.p[t];
        q2.A = v[t].dY2h; q2.B = v[t].A1h; q2.C = grads[t]->W2; q2.sumsq = sumsq[t];
        q2.M = d2; q2.N = d1; q2.lda = d2; q2.ldb = d1; q2.ldc = d1;
        nsvd_g16::Prob& q1 = g.p[nt + t];
        q1.A = v[t].dY1h; q1.B = v[t].Xh; q1.C = grads[t]->W1;
        q1.sumsq = sumsq[t] ? sumsq[t] + (d2 / 256) * (d1 / 128) : nullptr;
        q1.M = d1; q1.N = d0; q1.lda = d1; q1.ldb = d0; q1.ldc = d0;
    }
    g.nprob = 2 * nt; g.K = B; g.S = 1; g.f16 = f16;
    return nsvd_g16::launch(g, true, true, false, s);
}

int TowerCall::backward32() const {
    // dY2 = BN2'(dZ), dY2^T, db2 = column sums of dY2
    int rc = launch_bn_backward(bn2_backward_desc(0, 0), s);
    if (rc) return rc;
    // dW2 = dY2^T A1  (A = dY2^T (d2, B), B = A1^T (d1, B), K = B)
    GemmNT g;
    memset(&g, 0, sizeof(g));
    g.A = w[0].dY2T; g.lda = B; g.B = w[0].A1T; g.ldb = B; g.C = grads[0]->W2; g.ldc = d1;
    g.M = d2; g.N = d1; g.K = B; g.S = 1;
    g.sumsq = sumsq[0];
    rc = launch_gemm(g, s);
    if (rc) return rc;
    // W2^T (d1, d2), then dA1 = dY2 W2  (A = dY2 (B, d2), B = W2^T (d1, d2), K = d2)
    hipLaunchKernelGGL(tower_transpose_kernel, dim3((d2 / 32) * (d1 / 32)), dim3(256), 0, s, p[0]->W2, w[0].W2T, d2, d1);
    NSVD_CHECK_LAUNCH();
    memset(&g, 0, sizeof(g));
    g.A = w[0].dY2; g.lda = d2; g.B = w[0].W2T; g.ldb = d2; g.C = w[0].dA1; g.ldc = d1;
    g.M = B; g.N = d1; g.K = d2; g.S = 1;
    rc = launch_gemm(g, s);
    if (rc) return rc;
    // dY1^T = (BN1'(lrelu'(dA1)))^T, db1
    BnBwd b;
    memset(&b, 0, sizeof(b));
    b.dout = w[0].dA1; b.Y = w[0].Y1; b.mean = w[0].mean1; b.invstd = w[0].inv1; b.gamma = p[0]->g1; b.beta = p[0]->be1;
    b.dY = nullptr; b.dYT = w[0].dY1T; b.dgamma = grads[0]->g1; b.dbeta = grads[0]->be1; b.dbias = grads[0]->b1;
    b.B = B; b.N = d1; b.slope = slope;
    rc = launch_bn_backward(b, s);
    if (rc) return rc;
    // X^T (d0, B), then dW1 = dY1^T X  (A = dY1^T (d1, B), B = X^T (d0, B), K = B)
    hipLaunchKernelGGL(tower_transpose_kernel, dim3((B / 32) * (d0 / 32)), dim3(256), 0, s, x[0], w[0].XT, B, d0);
    NSVD_CHECK_LAUNCH();
    memset(&g, 0, sizeof(g));
    g.A = w[0].dY1T; g.lda = B; g.B = w[0].XT; g.ldb = B; g.C = grads[0]->W1; g.ldc = d0;
    g.M = d1; g.N = d0; g.K = B; g.S = 1;
    g.sumsq = sumsq[0] ? sumsq[0] + (d2 / 128) * (d1 / 128) : nullptr;
    return launch_gemm(g, s);
}

// What every entry point checks, and the carving. flags: the gemm_bf16 bits of a mixed-precision call.
int tower_call(TowerCall& c, int nt, const float* const* x, const nsvd_tower_params* const* p, int B, int d0, int d1,
               int d2, float slope, int update_running, bool mixed, int flags, void* const* ws, size_t ws_bytes,
               void* stream) {
    memset(&c, 0, sizeof(c));
    if (!tower_shape_ok(B, d0, d1, d2)) return NSVD_EINVAL;
    for (int t = 0; t < nt; ++t) {
        if (!x[t] || !ws[t] || !nsvd_tower_fields_ok(p[t], update_running != 0)) return NSVD_EINVAL;
        c.x[t] = x[t];
        c.p[t] = p[t];
        c.w[t] = carve_tower(B, d0, d1, d2, ws[t]);
        c.v[t] = views16(c.w[t]);
        if (!nsvd_ws_ok(ws[t], ws_bytes, c.w[t].bytes)) return NSVD_EINVAL;
    }
    if (mixed && !tower16_shape_ok(B, d0, d1, d2)) return NSVD_EUNSUPPORTED;
    c.nt = nt; c.B = B; c.d0 = d0; c.d1 = d1; c.d2 = d2;
    c.slope = slope; c.update_running = update_running; c.flags = flags;
    c.mixed = mixed;
    c.wide_only = mixed && (flags & NSVD_TOWER16_WIDE_ONLY);
    c.fused = mixed && tower16_fused(B, d0, d1, d2, slope);
    c.f16 = (flags & NSVD_TOWER16_F16) ? 1 : 0;
    c.S = mixed ? fwd2_slices16(nt, B, d1, d2) : fwd2_slices(B, d1, d2);
    c.s = (hipStream_t)stream;
    return 0;
}

// z[t]: where tower t's output goes (unused in phase 1 and behind NSVD_TOWER16_WIDE_ONLY)
int tower_forward(TowerCall& c, float eps, float momentum, int phase, float* const* z) {
    if (phase < 0 || phase > 2) return NSVD_EINVAL;
    const bool need_z = phase == 2 || (phase == 0 && !c.wide_only);
    for (int t = 0; t < c.nt; ++t) {
        if (!z[t] && need_z) return NSVD_EINVAL;
        c.z[t] = z[t];
    }
    c.eps = eps; c.momentum = momentum; c.phase = phase;
    if (phase == 2) return c.forward_narrow_end();
    return c.mixed ? c.forward16() : c.forward32();
}

// dz[t]: unused behind NSVD_TOWER16_WIDE_ONLY (the caller has written dY2h); sumsq: null, or per tower
// nsvd_tower_sumsq_count partials (dW2's tiles, then dW1's)
int tower_backward(TowerCall& c, const float* const* dz, const nsvd_tower_params* const* grads, float* const* sumsq) {
    for (int t = 0; t < c.nt; ++t) {
        if ((!dz[t] && !c.wide_only) || !nsvd_tower_fields_ok(grads[t], false)) return NSVD_EINVAL;
        c.dz[t] = dz[t];
        c.grads[t] = grads[t];
        c.sumsq[t] = sumsq ? sumsq[t] : nullptr;
    }
    return c.mixed ? c.backward16() : c.backward32();
}

}  // namespace

// Are these tower parameters (or gradient targets: need_running = false) usable - every tensor a kernel addresses
// through the struct there, and the running statistics when they are to be updated?
bool nsvd_tower_fields_ok(const nsvd_tower_params* t, bool need_running) {
    if (!t) return false;
    for (float* nsvd_tower_params::*f : NSVD_TOWER_FIELDS)
        if (!(t->*f)) return false;
    return !need_running || (t->rm1 && t->rv1 && t->rm2 && t->rv2);
}

extern "C" {

size_t nsvd_tower_workspace_bytes(int B, int d0, int d1, int d2) {
    if (!tower_shape_ok(B, d0, d1, d2)) return 0;
    return carve_tower(B, d0, d1, d2, nullptr).bytes;
}

size_t nsvd_tower_y2_offset(int B, int d0, int d1, int d2) {
    if (!tower_shape_ok(B, d0, d1, d2)) return 0;
    const TowerWs w = carve_tower(B, d0, d1, d2, nullptr);
    return (size_t)((char*)w.Y2 - (char*)nullptr);
}

int nsvd_tower_forward(const float* x, const nsvd_tower_params* p, int B, int d0, int d1, int d2, float slope,
                       float eps, float momentum, int update_running, int gemm_bf16, float* z, void* ws,
                       size_t ws_bytes, void* stream) {
    return nsvd_tower_forward_phase(x, p, B, d0, d1, d2, slope, eps, momentum, update_running, gemm_bf16, 0, z, ws,
                                    ws_bytes, stream);
}

int nsvd_tower_forward_phase(const float* x, const nsvd_tower_params* p, int B, int d0, int d1, int d2, float slope,
                             float eps, float momentum, int update_running, int gemm_bf16, int phase, float* z,
                             void* ws, size_t ws_bytes, void* stream) {
    TowerCall c;
    const int rc = tower_call(c, 1, &x, &p, B, d0, d1, d2, slope, update_running, gemm_bf16 != 0, gemm_bf16, &ws,
                              ws_bytes, stream);
    return rc ? rc : tower_forward(c, eps, momentum, phase, &z);
}

int nsvd_tower_backward(const float* x, const nsvd_tower_params* p, const float* dz, int B, int d0, int d1, int d2,
                        float slope, int gemm_bf16, const nsvd_tower_params* grads, void* ws, size_t ws_bytes,
                        void* stream) {
    return nsvd_tower_backward_sumsq(x, p, dz, B, d0, d1, d2, slope, gemm_bf16, grads, ws, ws_bytes, nullptr, stream);
}

int nsvd_tower_mixed_supported(int B, int d0, int d1, int d2) { return tower16_shape_ok(B, d0, d1, d2) ? 1 : 0; }

int nsvd_tower_mixed_fused(int B, int d0, int d1, int d2, float slope) {
    return tower16_shape_ok(B, d0, d1, d2) && tower16_fused(B, d0, d1, d2, slope) ? 1 : 0;
}

}  // extern "C"

// nsvd_tower_backward that also leaves, per workgroup of the two weight-gradient contractions, the sum of squares of
// its tile: sumsq[0 .. nsvd_tower_sumsq_count) (dW2's tiles, then dW1's), or nothing when sumsq is null
int nsvd_tower_sumsq_count(int d0, int d1, int d2, int gemm_bf16) {
    if (gemm_bf16) return sumsq_count16(d0, d1, d2);
    return (d2 / 128) * (d1 / 128) + (d1 / 128) * (d0 / 128);
}

int nsvd_tower_backward_sumsq(const float* x, const nsvd_tower_params* p, const float* dz, int B, int d0, int d1,
                              int d2, float slope, int gemm_bf16, const nsvd_tower_params* grads, void* ws,
                              size_t ws_bytes, float* sumsq, void* stream) {
    TowerCall c;  // (of the flag bits the single-tower backward takes the half type alone)
    const int rc = tower_call(c, 1, &x, &p, B, d0, d1, d2, slope, 0, gemm_bf16 != 0, gemm_bf16 & NSVD_TOWER16_F16, &ws,
                              ws_bytes, stream);
    return rc ? rc : tower_backward(c, &dz, &grads, sumsq ? &sumsq : nullptr);
}

// both towers of a mixed-precision CDK step through every launch together (cdk_step.hip); flags: the gemm_bf16 bits
int nsvd_tower16_forward_pair(const float* const* x, const nsvd_tower_params* const* p, int B, int d0, int d1, int d2,
                              float slope, float eps, float momentum, int update_running, int flags, float* const* z,
                              void* const* ws, size_t ws_bytes, hipStream_t s) {
    TowerCall c;
    const int rc = tower_call(c, 2, x, p, B, d0, d1, d2, slope, update_running, true, flags, ws, ws_bytes, s);
    return rc ? rc : tower_forward(c, eps, momentum, 0, z);
}

int nsvd_tower16_backward_pair(const float* const* x, const nsvd_tower_params* const* p, const float* const* dz, int B,
                               int d0, int d1, int d2, float slope, const nsvd_tower_params* const* grads,
                               void* const* ws, size_t ws_bytes, float* const* sumsq, hipStream_t s, int flags) {
    TowerCall c;
    const int rc = tower_call(c, 2, x, p, B, d0, d1, d2, slope, 0, true, flags, ws, ws_bytes, s);
    return rc ? rc : tower_backward(c, dz, grads, sumsq);
}

// what cdk_step.hip addresses inside a mixed-precision tower's workspace (it asks once per tower, when it carves its own)
NsvdTower16Views nsvd_tower16_views(int nt, int B, int d0, int d1, int d2, void* ws) {
    const TowerWs w = carve_tower(B, d0, d1, d2, ws);
    const Tower16 h = views16(w);
    NsvdTower16Views v;
    v.Y2p = w.Y2p; v.Y2 = w.Y2; v.mean2 = w.mean2; v.inv2 = w.inv2; v.dY2h = h.dY2h; v.W1h = h.W1h; v.W2h = h.W2h;
    v.S = fwd2_slices16(nt, B, d1, d2);
    v.slice_stride = (size_t)B * d2;
    return v;
}
