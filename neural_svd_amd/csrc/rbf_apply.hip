// Matrix-free radial kernel operator on coordinate batches:
//     out[i][l] = scale * sum_j k(|x_i - y_j|) f[j][l],        i < B1, j < B2, l < L
//     NSVD_RBF_GAUSSIAN: k(d) = exp(-d^2 / (2 ell^2)),    NSVD_RBF_EXPONENTIAL: k(d) = exp(-d / ell)
// - the (Kf, f) producer of NestedLoRA.compute_loss_kernel's `get_approx_kernel_op(x)(model, x, importance)` contract
// (methods/nestedlora.py:230-252) for a kernel given by a formula on coordinates drawn fresh every step; restated in
// float64 by oracle/nsvd_oracle.py:gaussian_kernel_apply. The (B1, B2) kernel matrix never exists in memory: a
// workgroup owns 64 rows of x and 64 heads, walks its slice of the reference rows in chunks of 64, and per chunk
//   1. forms the 64 x 64 squared distances by DIRECT DIFFERENCES on the VALU (sum_d (x_id - y_jd)^2: translation
//      invariant, a few ulp of d^2 whatever the offset of the data, never negative - the Gram form |x|^2 + |y|^2 - 2 x.y
//      loses u (|x|^2 + |y|^2) / ell^2 in the exponent and is useless for points far from the origin).
//      Lane = row of x (its coordinates come from LDS, four at a time), the 16 reference rows of a wave are WAVE-UNIFORM:
//      their coordinates are read through the scalar cache and cost no LDS bandwidth;
//   2. applies the exponential as ONE v_exp_f32 per pair (exp2 with log2 e / (2 ell^2), or log2 e / ell, folded in);
//   3. writes the chunk into LDS as the A operand in tile_nt.h's layout (rows of 64 + 4 floats: conflict-free b128);
//   4. accumulates against the matching chunk of f^T (K-contiguous after apply_prep_kernel's transpose, staged like
//      tile_nt.h's B operand) on v_mfma_f32_32x32x2_f32, four accumulation chains as in tile_nt.h.
// tile_nt.h's routine itself stages BOTH operands from global memory, which is exactly what must not happen to the
// kernel matrix; its LDS layout, wave-to-tile map and MFMA read pattern are kept so that the two stay comparable.
// The reference rows are split into slices so that the grid fills the chip at small B1; partial tiles are reduced in
// slice order by apply_reduce_kernel: no atomics, bit-reproducible. What this file shares with dot_apply.hip and the two
// *_apply_pair.hip (padding and arena, slice rule, prep and reduce kernels, LDS-only barrier, chunk MFMAs, the radial
// map) is apply_common.h's.
#include "apply_common.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;

struct RbfWs {
    float* yP;    // (B2p, Dp) reference coordinates, zero padded (padded coordinates add 0 to every distance)
    float* fT;    // (Lp, B2p) f transposed, zero padded (padded reference rows contribute k * 0)
    float* part;  // (S, B1p, Lp) partial tiles
    int B1p, B2p, Dp, Lp, S;
    size_t bytes;
};

RbfWs carve(void* base, int B1, int B2, int D, int L) {
    const ApplyPad pd = apply_pad(B1, B2, D, L, 4);
    RbfWs w;
    w.B1p = pd.B1p, w.B2p = pd.B2p, w.Dp = pd.Dp, w.Lp = pd.Lp;
    w.S = apply_slices((long)(w.B1p / T) * (w.Lp / T), w.B2p / KC);
    NsvdArena a(base);
    w.yP = a.take((size_t)w.B2p * w.Dp);
    w.fT = a.take((size_t)w.Lp * w.B2p);
    w.part = a.take((size_t)w.S * w.B1p * w.Lp);
    w.bytes = a.off;
    return w;
}

// tile (tb, tl) x slice. LDS: two buffers of [A chunk | B chunk] (NSVD_TNT_FLOATS), then the x tile (64, Dp + 4).
// cexp: log2 e / (2 ell^2) (Gaussian) or log2 e / ell (exponential)
template <int KIND>
__global__ void __launch_bounds__(256, 2) rbf_main_kernel(const float* __restrict__ x, int B1, int D, RbfWs w, float cexp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* xs = lds + NSVD_TNT_FLOATS;
    const int tb = blockIdx.x, tl = blockIdx.y, slice = blockIdx.z;
    const int chunks = w.B2p / KC;
    const int c0 = (int)((long)chunks * slice / w.S), c1 = (int)((long)chunks * (slice + 1) / w.S);
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);  // (uniform by construction; tells the compiler so)
    const int Dp = w.Dp, Dq = Dp >> 2, xld = Dp + 4;
    for (int e = t; e < 64 * Dp; e += 256) {
        const int i = e / Dp, d = e - i * Dp;
        const int r = tb * T + i;
        xs[i * xld + d] = (r < B1 && d < D) ? x[(size_t)r * D + d] : 0.f;
    }
    __syncthreads();
    const int ra = (wv & 1) * 32 + (lane & 31), rb = (wv >> 1) * 32 + (lane & 31), kq = (lane >> 5) * 4;
    const int lr0 = t >> 4, lc = (t & 15) * 4;
    const float* fp = w.fT + ((size_t)tl * T + lr0) * w.B2p + lc;
    const float4* xq = (const float4*)(xs + lane * xld);
    nsvd_f32x16 acc0 = {0}, acc1 = {0}, acc2 = {0}, acc3 = {0};
    // the chunk of f^T runs one chunk ahead in registers: requested before the barrier of the chunk before (the barrier
    // below leaves global loads in flight, as tile_nt.h's), consumed after the distances of its own chunk
    // (named registers: hipcc demotes a float4 array rewritten inside the loop to scratch, as tile_nt.h found)
    const size_t fr = (size_t)16 * w.B2p;
    const float* fc = fp + (size_t)c0 * KC;
    float4 fb0 = *(const float4*)fc, fb1 = *(const float4*)(fc + fr), fb2 = *(const float4*)(fc + 2 * fr),
           fb3 = *(const float4*)(fc + 3 * fr);
    for (int c = c0; c < c1; ++c) {
        float* buf = lds + ((c - c0) & 1) * NSVD_TNT_BUF;
        // squared distances of row `lane` of the tile to the 16 reference rows of this wave
        const float4* yq = (const float4*)w.yP + ((size_t)c * KC + 16 * wv) * Dq;
        float d2[16];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) d2[jj] = 0.f;
        for (int q = 0; q < Dq; ++q) {
            const float4 xv = xq[q];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const float4 yv = yq[(size_t)jj * Dq + q];
                const float e0 = xv.x - yv.x, e1 = xv.y - yv.y, e2 = xv.z - yv.z, e3 = xv.w - yv.w;
                d2[jj] = fmaf(e0, e0, d2[jj]);
                d2[jj] = fmaf(e1, e1, d2[jj]);
                d2[jj] = fmaf(e2, e2, d2[jj]);
                d2[jj] = fmaf(e3, e3, d2[jj]);
            }
        }
        float kv[16];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) kv[jj] = apply_radial<KIND>(d2[jj], cexp);
        float* la = buf + lane * LDT + 16 * wv;
#pragma unroll
        for (int i = 0; i < 4; ++i) *(float4*)(la + 4 * i) = make_float4(kv[4 * i], kv[4 * i + 1], kv[4 * i + 2], kv[4 * i + 3]);
        float* lb = buf + T * LDT + lr0 * LDT + lc;
        *(float4*)(lb) = fb0;
        *(float4*)(lb + 16 * LDT) = fb1;
        *(float4*)(lb + 32 * LDT) = fb2;
        *(float4*)(lb + 48 * LDT) = fb3;
        const int cn = min(c + 1, c1 - 1);  // (past the end: the last chunk again, never consumed)
        fc = fp + (size_t)cn * KC;
        fb0 = *(const float4*)fc;
        fb1 = *(const float4*)(fc + fr);
        fb2 = *(const float4*)(fc + 2 * fr);
        fb3 = *(const float4*)(fc + 3 * fr);
        // one barrier per chunk: the buffer written next is the one every wave finished reading before THIS barrier
        // (LDS only: the global loads just issued stay in flight)
        apply_lds_barrier();
        apply_chunk_mfma(buf, ra, rb, kq, acc0, acc1, acc2, acc3);
    }
    const nsvd_f32x16 acc = (acc0 + acc1) + (acc2 + acc3);
    float* out = w.part + (size_t)slice * w.B1p * w.Lp;
    const int row0 = tb * T + (wv & 1) * 32, col = tl * T + (wv >> 1) * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) apply_store_acc(out, w.Lp, row0, col, lane, r, acc[r]);
}

size_t rbf_lds_bytes(int Dp) { return (size_t)(NSVD_TNT_FLOATS + 64 * (Dp + 4)) * sizeof(float); }

}  // namespace

extern "C" size_t nsvd_rbf_apply_workspace_bytes(int B1, int B2, int D, int L) {
    if (!apply_shape_ok(B1, B2, D, L) || D > APPLY_MAX_D) return 0;
    return carve(nullptr, B1, B2, D, L).bytes;
}

extern "C" int nsvd_rbf_apply(const float* x, int B1, const float* y, int B2, int D, const float* f, int L, int kind,
                              float ell, float scale, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!apply_args_ok({x, y, f, out, ws}, B1, B2, D, L)) return NSVD_EINVAL;
    if (kind != NSVD_RBF_GAUSSIAN && kind != NSVD_RBF_EXPONENTIAL) return NSVD_EINVAL;
    if (!(ell > 0.f)) return NSVD_EINVAL;  // (also NaN)
    if (D > APPLY_MAX_D) return NSVD_EUNSUPPORTED;
    const RbfWs w = carve(ws, B1, B2, D, L);
    if (!nsvd_ws_ok(ws, ws_bytes, w.bytes)) return NSVD_EINVAL;
    const float cexp = apply_radial_cexp(kind, ell);
    hipStream_t s = (hipStream_t)stream;
    ApplyPrep pr = {};
    pr.s[0] = {y, w.yP, nullptr, f, w.fT, B2, w.B2p};
    pr.D = D, pr.Dp = w.Dp, pr.L = L, pr.Lp = w.Lp;
    apply_prep_launch(pr, s);
    NSVD_CHECK_LAUNCH();
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)rbf_main_kernel<NSVD_RBF_GAUSSIAN>,
                                                    (const void*)rbf_main_kernel<NSVD_RBF_EXPONENTIAL>},
                                                   rbf_lds_bytes(APPLY_MAX_D)))
        return rc;
    const dim3 grid(w.B1p / T, w.Lp / T, w.S);
    nsvd_prof_begin(s);
    if (kind == NSVD_RBF_GAUSSIAN)
        rbf_main_kernel<NSVD_RBF_GAUSSIAN><<<grid, 256, rbf_lds_bytes(w.Dp), s>>>(x, B1, D, w, cexp);
    else
        rbf_main_kernel<NSVD_RBF_EXPONENTIAL><<<grid, 256, rbf_lds_bytes(w.Dp), s>>>(x, B1, D, w, cexp);
    nsvd_prof_end(s);
    NSVD_CHECK_LAUNCH();
    const size_t n = (size_t)B1 * L;
    apply_reduce_kernel<><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(w.part, w.S, w.B1p, w.Lp, B1, L, scale, out);
    NSVD_CHECK_LAUNCH();
    return 0;
}
