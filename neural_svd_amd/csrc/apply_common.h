// What the matrix-free kernel products share (rbf_apply.hip, dot_apply.hip, rbf_apply_pair.hip, dot_apply_pair.hip;
// the slice rule and the tile store also serve kernel_apply.hip, the barrier kernel_apply_pair.hip): the padding rule,
// the prep kernel (pad coordinates, row norms, transposes), the reduce of partial copies, the maps of the kernel kinds
// and the pieces of tile_nt.h's layout that every main kernel repeats. What only the two-sided products share is
// pair_common.h, on top of this header. Everything has internal linkage: each file gets its own.
#pragma once
#include <float.h>
#include <math.h>
#include <initializer_list>
#include "nsvd_kernels.h"
#include "tile_nt.h"

constexpr int APPLY_MAX_D = 64;  // the model kernels' own input limit

// ---- host: shapes, workspace -----------------------------------------------------------------------------------------
struct ApplyPad {
    int B1p, B2p, Dp, Lp;
};

// rows and heads to whole 64 x 64 tiles, D to the file's granule (4: float4 reads of a row, 8: one b128 per MFMA group)
static inline ApplyPad apply_pad(int B1, int B2, int D, int L, int granule) {
    return {nsvd_cdiv(B1, NSVD_TNT_T) * NSVD_TNT_T, nsvd_cdiv(B2, NSVD_TNT_KC) * NSVD_TNT_KC,
            nsvd_cdiv(D, granule) * granule, nsvd_cdiv(L, NSVD_TNT_T) * NSVD_TNT_T};
}

// slices of the contraction range of a one-sided product: enough workgroups for two per CU, at least 8 chunks per slice
static inline int apply_slices(long tiles, int chunks) {
    int S = 1;
    while (tiles * S < 512 && chunks / (2 * S) >= 8) S *= 2;
    return S;
}

static inline bool apply_shape_ok(int B1, int B2, int D, int L) { return B1 > 0 && B2 > 0 && L > 0 && D > 0; }

static inline bool apply_args_ok(std::initializer_list<const void*> ptrs, int B1, int B2, int D, int L) {
    for (const void* p : ptrs)
        if (!p) return false;
    return apply_shape_ok(B1, B2, D, L);
}

// do the float arrays at a (na elements) and b (nb elements) share a byte?
static inline bool apply_overlap(const float* a, size_t na, const float* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb * sizeof(float) && pb < pa + na * sizeof(float);
}

// the exponent's constant of the radial kinds, log2 e / (2 ell^2) (Gaussian) or log2 e / ell (exponential), in double
// and kept finite: a tiny ell gives exp2(-0 * FLT_MAX) = 1 on the diagonal and 0 elsewhere
static inline float apply_radial_cexp(int kind, float ell) {
    const double le = 1.4426950408889634;
    double cd = kind == NSVD_RBF_GAUSSIAN ? le / (2.0 * (double)ell * (double)ell) : le / (double)ell;
    if (!(cd < (double)FLT_MAX)) cd = (double)FLT_MAX;
    return (float)cd;
}

// the deep ReLU kinds of the dot-product products (NNGP and NTK: apply_relu_deep)
constexpr __host__ __device__ bool apply_is_relu(int kind) {
    return kind == NSVD_DOT_RELU_NNGP || kind == NSVD_DOT_RELU_NTK;
}

// nsvd_dot_apply and nsvd_dot_apply_pair: is `kind` one they serve, with parameters in its range? (the arc-cosine kind
// reads none of the three; the deep ReLU kinds read the depth from the degree slot)
static inline bool apply_dot_kind_ok(int kind, float gamma, float coef0, int degree) {
    if (kind == NSVD_DOT_POLYNOMIAL) return degree >= 1 && degree <= 8 && isfinite(gamma) && isfinite(coef0);
    if (apply_is_relu(kind))
        return degree >= 1 && degree <= 8 && isfinite(gamma) && gamma > 0.f && isfinite(coef0) && coef0 >= 0.f;
    return kind == NSVD_DOT_ARCCOS1;
}

// ---- prep ------------------------------------------------------------------------------------------------------------
// One side of a product: `rows` coordinate rows c (rows, D) and a matrix m (rows, L) that is contracted over them.
// cP = c zero padded to (ld, Dp), cN = the row norms (0 for padded rows), mT = m^T zero padded to (Lp, ld).
// c == nullptr: no coordinates to pad; cN == nullptr: no norms. ld == 0: no such side.
struct ApplyPrepSide {
    const float* c;
    float* cP;
    float* cN;
    const float* m;
    float* mT;
    int rows, ld;
};

struct ApplyPrep {
    ApplyPrepSide s[2];
    int D, Dp, L, Lp;
    int rooted;  // norms as |c| (1) or |c|^2 (0)
};

// grid: (s[0].ld / 64 + s[1].ld / 64, Lp / 64 + 1). The first s[0].ld / 64 columns of blocks serve side 0, the others
// side 1; the last row of blocks pads the coordinates and writes the norms (fmaf over d ascending), the others
// transpose through a 64 x 64 LDS tile.
// (the kernels of this header are templates so that a file's code object holds only the ones it launches)
template <int = 0>
static __global__ void __launch_bounds__(256) apply_prep_kernel(ApplyPrep p) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x;
    const int nb0 = p.s[0].ld / 64;
    const bool is0 = (int)blockIdx.x < nb0;
    const ApplyPrepSide sd = is0 ? p.s[0] : p.s[1];
    const int j0 = (is0 ? (int)blockIdx.x : (int)blockIdx.x - nb0) * 64;
    if ((int)blockIdx.y == p.Lp / 64) {
        if (!sd.c) return;
        for (int e = t; e < 64 * p.Dp; e += 256) {
            const int j = j0 + e / p.Dp, d = e % p.Dp;
            sd.cP[(size_t)j * p.Dp + d] = (j < sd.rows && d < p.D) ? sd.c[(size_t)j * p.D + d] : 0.f;
        }
        if (sd.cN && t < 64) {
            const int j = j0 + t;
            float s = 0.f;
            if (j < sd.rows)
                for (int d = 0; d < p.D; ++d) {
                    const float v = sd.c[(size_t)j * p.D + d];
                    s = fmaf(v, v, s);
                }
            sd.cN[j] = p.rooted ? __builtin_sqrtf(s) : s;
        }
        return;
    }
    const int l0 = blockIdx.y * 64;
    for (int e = t; e < 4096; e += 256) {
        const int jj = e >> 6, ll = e & 63;  // consecutive threads: consecutive heads of one row
        tile[jj][ll] = (j0 + jj < sd.rows && l0 + ll < p.L) ? sd.m[(size_t)(j0 + jj) * p.L + l0 + ll] : 0.f;
    }
    __syncthreads();
    for (int e = t; e < 4096; e += 256) {
        const int ll = e >> 6, jj = e & 63;
        sd.mT[(size_t)(l0 + ll) * sd.ld + j0 + jj] = tile[jj][ll];
    }
}

template <int = 0>
static inline void apply_prep_launch(const ApplyPrep& p, hipStream_t s) {
    apply_prep_kernel<><<<dim3(p.s[0].ld / 64 + p.s[1].ld / 64, p.Lp / 64 + 1), 256, 0, s>>>(p);
}

// ---- reduce ----------------------------------------------------------------------------------------------------------
// out[i] = scale * (sum of the n partial copies of a (Bp, Lp) matrix at element i of its (B, L) corner), in copy order:
// no atomics, bit-reproducible
__device__ __forceinline__ void apply_reduce_one(const float* __restrict__ part, int n, int Bp, int Lp, int L, size_t i,
                                                 float scale, float* __restrict__ out) {
    const size_t b = i / L, l = i - b * L;
    float s = 0.f;
    for (int c = 0; c < n; ++c) s += part[((size_t)c * Bp + b) * Lp + l];
    out[i] = scale * s;
}

template <int = 0>
static __global__ void __launch_bounds__(256) apply_reduce_kernel(const float* __restrict__ part, int S, int B1p, int Lp,
                                                                  int B1, int L, float scale, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B1 * L) apply_reduce_one(part, S, B1p, Lp, L, i, scale, out);
}

// ---- device: the pieces of a main kernel -----------------------------------------------------------------------------
// Workgroup barrier that orders LDS only: __syncthreads() would also wait for the global loads in flight (the staging
// loads that every main kernel issues just before it), and an asm barrier with a memory clobber makes the compiler give
// up the scalar loads of y (rbf_apply.hip, rbf_apply_pair.hip).
__device__ __forceinline__ void apply_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// 32 MFMAs of one wave on LDS buffer `b` (A chunk then B chunk, rows of LDT floats): tile_nt.h's read pattern
__device__ __forceinline__ void apply_chunk_mfma(const float* __restrict__ b, int ra, int rb, int kq, nsvd_f32x16& a0,
                                                 nsvd_f32x16& a1, nsvd_f32x16& a2, nsvd_f32x16& a3) {
    constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;
    const float* la = b + ra * LDT + kq;
    const float* lb = b + T * LDT + rb * LDT + kq;
    float4 av = *(const float4*)la, bv = *(const float4*)lb;
#pragma unroll
    for (int s = 0; s < KC / 8; ++s) {
        float4 an = av, bn = bv;
        if (s + 1 < KC / 8) {
            an = *(const float4*)(la + (s + 1) * 8);
            bn = *(const float4*)(lb + (s + 1) * 8);
        }
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, a2, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, a3, 0, 0, 0);
        av = an;
        bv = bn;
    }
}

// the radial kinds from a squared distance: ONE v_exp_f32 per pair (cexp: apply_radial_cexp)
template <int KIND>
__device__ __forceinline__ float apply_radial(float d2, float cexp) {
    const float r = KIND == NSVD_RBF_GAUSSIAN ? d2 : __builtin_sqrtf(d2);
    return __builtin_amdgcn_exp2f(-(r * cexp));
}

// (gamma s + coef0)^degree, the power by multiplication: one wave-uniform loop over the degree, 16 independent products
// inside
__device__ __forceinline__ nsvd_f32x16 apply_poly(const nsvd_f32x16& sv, float gamma, float coef0, int degree) {
    nsvd_f32x16 u, pw;
#pragma unroll
    for (int r = 0; r < 16; ++r) u[r] = fmaf(gamma, sv[r], coef0);
    pw = u;
    for (int d = 1; d < degree; ++d) pw *= u;
    return pw;
}

// the arc-cosine map of s = x.y. nx = |x_i| of this lane's row, ny = |y_j|.
__device__ __forceinline__ float apply_arccos1(float s, float nx, float ny) {
    const float p = nx * ny;
    float c = s / p;
    c = fminf(fmaxf(c, -1.f), 1.f);
    // sin t and pi - t = acos(-c) from the SAME c (the bracket is stationary at t = 0), neither through t near pi
    const float sn = __builtin_sqrtf((1.f - c) * (1.f + c));
    const float br = fmaxf(fmaf(acosf(-c), c, sn), 0.f);
    const float k = p * (br * 0.318309886183790671538f);
    return p > 0.f ? k : 0.f;  // a zero row on either side (also c = NaN from 0 / 0)
}

// the deep ReLU kinds (NNGP: k = S_depth; NTK: k = T_depth, a second chain beside S) of a lane's 16 values s = x.y.
// nx2 = |x_i|^2 of the lane's row, ny2 = the 16 |y_j|^2. Level l maps S_{l-1} to S_l = gamma p A1(c) + coef0 with
// p = sqrt(q_{l-1}(x) q_{l-1}(y)), c = S_{l-1} / p, and T_l = S_l + gamma T_{l-1} A0(c). q_l(v) = gl |v|^2 + bl with the
// wave-uniform gl = gamma^l, bl = gamma bl + coef0: one FMA per pair and level, nothing carried. p = 0 (a zero row at
// level 1; at every level when coef0 = 0) gives S_l = T_l = coef0. sin t and pi - t come from the SAME clamped c, as in
// apply_arccos1; with gamma = 1, coef0 = 0, depth = 1 the values are apply_arccos1's up to the rounding of p and of c
// (p = sqrt(|x|^2 |y|^2) and a corrected reciprocal here, |x| |y| and a division there). A0 = acos(-c) / pi has an unbounded slope at c = +-1: the rounding of c there (the diagonal of a Gram,
// near-parallel rows, every pair at D = 1) reaches the NTK value as sqrt(2 delta) / pi per level, and is left there.
template <bool NTK>
__device__ __forceinline__ void apply_relu_deep(const nsvd_f32x16& sv, float nx2, const float (&ny2)[16], float gamma,
                                                float coef0, int depth, float (&kv)[16]) {
    constexpr float inv_pi = 0.318309886183790671538f;
    float S[16], Tn[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = Tn[r] = sv[r];
    float gl = 1.f, bl = 0.f;
    for (int l = 0; l < depth; ++l) {
        const float qx = fmaf(gl, nx2, bl);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // ONE root: where x_i meets itself qx = qy and p = qx to the bit. c = S / p by the reciprocal and one
            // correction step (S = p then gives c = 1 exactly, where A0 cannot afford the reciprocal's ulp)
            const float p = __builtin_sqrtf(qx * fmaf(gl, ny2[r], bl));
            const float rp = __builtin_amdgcn_rcpf(p);
            float c = S[r] * rp;
            c = fmaf(fmaf(-c, p, S[r]), rp, c);
            c = fminf(fmaxf(c, -1.f), 1.f);  // (also c = NaN where p = 0)
            const float sn = __builtin_sqrtf((1.f - c) * (1.f + c));
            const float ac = acosf(-c);
            const float br = fmaxf(fmaf(ac, c, sn), 0.f);
            const float s1 = fmaf(gamma * p, br * inv_pi, coef0);
            if (NTK) Tn[r] = p > 0.f ? fmaf(gamma * (ac * inv_pi), Tn[r], s1) : coef0;
            S[r] = p > 0.f ? s1 : coef0;
        }
        bl = fmaf(gamma, bl, coef0);
        gl *= gamma;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) kv[r] = NTK ? Tn[r] : S[r];
}

// Partial-tile store: element r (value v) of a wave's 32 x 32 accumulator, MFMA 32x32 layout, to rows row0.., column
// col of a matrix with Lp columns. The kernel keeps the unrolled loop over r = 0 .. 15 and reads acc[r] itself: handed
// the whole accumulator, the compiler keeps the sum of the four chains a vector and rebuilds the main kernel around it.
__device__ __forceinline__ void apply_store_acc(float* out, int Lp, int row0, int col, int lane, int r, float v) {
    const int row = row0 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
    out[(size_t)row * Lp + col] = v;
}
