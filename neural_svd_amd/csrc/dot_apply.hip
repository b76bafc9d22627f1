// Matrix-free dot-product kernel operator on coordinate batches:
//     out[i][l] = scale * sum_j k(x_i, y_j) f[j][l],        i < B1, j < B2, l < L
//     NSVD_DOT_POLYNOMIAL: k = (gamma x.y + coef0)^degree, integer degree 1..8, the power by multiplication
//     NSVD_DOT_ARCCOS1:    k = |x||y| / pi (sin t + (pi - t) cos t), cos t = x.y / (|x||y|)   (Cho & Saul, order 1)
//     NSVD_DOT_RELU_NNGP:  k = S_depth, NSVD_DOT_RELU_NTK: k = T_depth of a ReLU network `depth` layers deep (weight
//                          variance gamma, bias variance coef0, depth in the degree slot): apply_relu_deep's recursion
// - the sibling of rbf_apply.hip for kernels of the inner product. An inner product has no cancellation to protect
// (rbf_apply.hip forms distances by direct differences on the VALU for that reason), so x.y goes on the matrix pipe: two
// contractions back to back, like an attention forward. A workgroup owns 64 rows of x and 64 heads, walks its slice of
// the reference rows in chunks of 64 (rbf_apply.hip's shape; slice rule, prep and reduce kernels: apply_common.h), and
// per chunk
//   1. forms S^T = Y_chunk X_tile^T (64 x 64 x Dp) on v_mfma_f32_32x32x2_f32: the y chunk is staged in LDS (two
//      buffers, its global loads two chunks ahead in registers), the x operand of a wave (32 rows, this lane's half of
//      every 8 coordinates) is loop invariant and lives in registers, loaded once per workgroup;
//   2. applies the map (apply_poly, apply_arccos1, apply_relu_deep) to the accumulators in registers. S^T, not S: a lane
//      then owns ONE row i of x (one |x_i|, held in a register) and 4 runs of 4 consecutive reference rows j, which are 4
//      ds_write_b128 into the A operand of the second contraction - S would leave it 16 ds_write_b32;
//   3. accumulates against the matching chunk of f^T exactly as rbf_apply.hip does (tile_nt.h's LDS layout and MFMA
//      read pattern in apply_chunk_mfma, f^T one chunk ahead in registers, one apply_lds_barrier per chunk).
// D is padded to a multiple of 8 (one ds_read_b128 per lane feeds 4 MFMAs of k = 2) and the first contraction issues
// Dp / 2 MFMAs per wave and chunk: 4 at D <= 8, 32 at D = 64, beside the 32 of the second.
#include "apply_common.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;

struct DotWs {
    float* yP;    // (B2p, Dp) reference coordinates, zero padded
    float* yN;    // (B2p) |y_j|^2, 0 for padded rows
    float* fT;    // (Lp, B2p) f transposed, zero padded
    float* part;  // (S, B1p, Lp) partial tiles
    int B1p, B2p, Dp, Lp, S;
    size_t bytes;
};

DotWs carve(void* base, int B1, int B2, int D, int L) {
    const ApplyPad pd = apply_pad(B1, B2, D, L, 8);
    DotWs w;
    w.B1p = pd.B1p, w.B2p = pd.B2p, w.Dp = pd.Dp, w.Lp = pd.Lp;
    w.S = apply_slices((long)(w.B1p / T) * (w.Lp / T), w.B2p / KC);
    NsvdArena a(base);
    w.yP = a.take((size_t)w.B2p * w.Dp);
    w.yN = a.take((size_t)w.B2p);
    w.fT = a.take((size_t)w.Lp * w.B2p);
    w.part = a.take((size_t)w.S * w.B1p * w.Lp);
    w.bytes = a.off;
    return w;
}

struct DotMap {
    float gamma, coef0;
    int degree;
};

// the ds_read_b128 of the y operand for step s of the first contraction, and its 4 MFMAs on two chains
#define DOT_S_STEP(s)                                                                          \
    if ((s) < nq) {                                                                            \
        const float4 yv = *(const float4*)(yr + (s) * 8);                                      \
        s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.x, xr##s.x, s0, 0, 0, 0);                 \
        s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.y, xr##s.y, s1, 0, 0, 0);                 \
        s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.z, xr##s.z, s0, 0, 0, 0);                 \
        s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.w, xr##s.w, s1, 0, 0, 0);                 \
    }
#define DOT_X_LOAD(s)                                                                          \
    float4 xr##s = make_float4(0.f, 0.f, 0.f, 0.f);                                            \
    if ((s) < nq && xrow < B1) {                                                               \
        const float* xp_ = x + (size_t)xrow * D;                                               \
        const int d_ = (s) * 8 + kq;                                                           \
        xr##s.x = d_ < D ? xp_[d_] : 0.f;                                                      \
        xr##s.y = d_ + 1 < D ? xp_[d_ + 1] : 0.f;                                              \
        xr##s.z = d_ + 2 < D ? xp_[d_ + 2] : 0.f;                                              \
        xr##s.w = d_ + 3 < D ? xp_[d_ + 3] : 0.f;                                              \
    }                                                                                          \
    nx2 = fmaf(xr##s.x, xr##s.x, nx2);                                                         \
    nx2 = fmaf(xr##s.y, xr##s.y, nx2);                                                         \
    nx2 = fmaf(xr##s.z, xr##s.z, nx2);                                                         \
    nx2 = fmaf(xr##s.w, xr##s.w, nx2);
// the y chunk's staging: thread t moves the float4s t + 256 i < 16 Dp of the chunk's contiguous (64, Dp) block
#define DOT_Y_LOAD(cc)                                                                         \
    {                                                                                          \
        const float4* yc_ = (const float4*)(w.yP + (size_t)(cc) * KC * Dp) + t;                \
        if (t < nv) yb0 = yc_[0];                                                              \
        if (t + 256 < nv) yb1 = yc_[256];                                                      \
        if (t + 512 < nv) yb2 = yc_[512];                                                      \
        if (t + 768 < nv) yb3 = yc_[768];                                                      \
        if (KIND != NSVD_DOT_POLYNOMIAL && t < KC) ynb = w.yN[(size_t)(cc) * KC + t];          \
    }
#define DOT_Y_PUT(b)                                                                           \
    {                                                                                          \
        float* yd_ = ys + (b) * ybuf;                                                          \
        if (t < nv) *(float4*)(yd_ + yo0) = yb0;                                               \
        if (t + 256 < nv) *(float4*)(yd_ + yo1) = yb1;                                         \
        if (t + 512 < nv) *(float4*)(yd_ + yo2) = yb2;                                         \
        if (t + 768 < nv) *(float4*)(yd_ + yo3) = yb3;                                         \
        if (KIND == NSVD_DOT_ARCCOS1 && t < KC) yd_[64 * yld + t] = __builtin_sqrtf(ynb);      \
        if (apply_is_relu(KIND) && t < KC) yd_[64 * yld + t] = ynb;                            \
    }

// tile (tb, tl) x slice. LDS: two buffers of [A chunk | B chunk] (NSVD_TNT_FLOATS), then two buffers of
// [y chunk (64, Dp + 4) | |y_j| (64)] (the deep ReLU kinds: |y_j|^2).
template <int KIND>
__global__ void __launch_bounds__(256, 2) dot_main_kernel(const float* __restrict__ x, int B1, int B2, int D, DotWs w,
                                                          DotMap mp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ys = lds + NSVD_TNT_FLOATS;
    const int tb = blockIdx.x, tl = blockIdx.y, slice = blockIdx.z;
    const int chunks = w.B2p / KC;
    const int c0 = (int)((long)chunks * slice / w.S), c1 = (int)((long)chunks * (slice + 1) / w.S);
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);  // (uniform by construction; tells the compiler so)
    const int Dp = w.Dp, nq = Dp >> 3, yld = Dp + 4, ybuf = 64 * yld + 64, nv = 16 * Dp;
    const int ra = (wv & 1) * 32 + (lane & 31), rb = (wv >> 1) * 32 + (lane & 31), kq = (lane >> 5) * 4;
    const int lr0 = t >> 4, lc = (t & 15) * 4;
    // first contraction: wave wv forms reference rows 32 (wv & 1) .. x rows 32 (wv >> 1) .. of S^T
    const int jb = (wv & 1) * 32, ib = (wv >> 1) * 32;
    const int xrow = tb * T + ib + (lane & 31);
    float nx2 = 0.f;
    DOT_X_LOAD(0) DOT_X_LOAD(1) DOT_X_LOAD(2) DOT_X_LOAD(3) DOT_X_LOAD(4) DOT_X_LOAD(5) DOT_X_LOAD(6) DOT_X_LOAD(7)
    nx2 += __shfl_xor(nx2, 32);  // the other half of every 8 coordinates
    const float nx = __builtin_sqrtf(nx2);
    if (apply_is_relu(KIND)) {
        // |x_i|^2 summed as the prep kernel sums |y_j|^2 (d ascending): equal rows give equal bits, and sqrt(q q) = q
        nx2 = 0.f;
        if (xrow < B1)
            for (int d = 0; d < D; ++d) {
                const float v = x[(size_t)xrow * D + d];
                nx2 = fmaf(v, v, nx2);
            }
    }
    // LDS offsets of this thread's float4s of a y chunk
    const int Dq = Dp >> 2;
    const int yo0 = (t / Dq) * yld + (t % Dq) * 4, yo1 = ((t + 256) / Dq) * yld + ((t + 256) % Dq) * 4,
              yo2 = ((t + 512) / Dq) * yld + ((t + 512) % Dq) * 4, yo3 = ((t + 768) / Dq) * yld + ((t + 768) % Dq) * 4;
    const float* fp = w.fT + ((size_t)tl * T + lr0) * w.B2p + lc;
    nsvd_f32x16 acc0 = {0}, acc1 = {0}, acc2 = {0}, acc3 = {0};
    // f^T runs one chunk ahead in registers, the y chunk two (one in LDS, one in registers): requested before the barrier
    // of the chunk before, which leaves global loads in flight (named registers: hipcc demotes a float4 array rewritten
    // inside the loop to scratch, as tile_nt.h found)
    const size_t fr = (size_t)16 * w.B2p;
    const float* fc = fp + (size_t)c0 * KC;
    float4 fb0 = *(const float4*)fc, fb1 = *(const float4*)(fc + fr), fb2 = *(const float4*)(fc + 2 * fr),
           fb3 = *(const float4*)(fc + 3 * fr);
    float4 yb0 = make_float4(0.f, 0.f, 0.f, 0.f), yb1 = yb0, yb2 = yb0, yb3 = yb0;
    float ynb = 0.f;
    DOT_Y_LOAD(c0)
    DOT_Y_PUT(0)
    DOT_Y_LOAD(min(c0 + 1, c1 - 1))
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
        const int par = (c - c0) & 1;
        float* buf = lds + par * NSVD_TNT_BUF;
        const float* yb = ys + par * ybuf;
        const float* yr = yb + (jb + (lane & 31)) * yld + kq;
        nsvd_f32x16 s0 = {0}, s1 = {0};
        DOT_S_STEP(0) DOT_S_STEP(1) DOT_S_STEP(2) DOT_S_STEP(3) DOT_S_STEP(4) DOT_S_STEP(5) DOT_S_STEP(6) DOT_S_STEP(7)
        const nsvd_f32x16 sv = s0 + s1;
        // sv[r] = x_i . y_j, i = ib + (lane & 31), j = jb + 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
        float kv[16];
        if (KIND == NSVD_DOT_POLYNOMIAL) {
            const nsvd_f32x16 pw = apply_poly(sv, mp.gamma, mp.coef0, mp.degree);
#pragma unroll
            for (int r = 0; r < 16; ++r) kv[r] = pw[r];
        } else if (apply_is_relu(KIND)) {
            float ny2[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 ny = *(const float4*)(yb + 64 * yld + jb + 8 * g + kq);
                ny2[4 * g] = ny.x, ny2[4 * g + 1] = ny.y, ny2[4 * g + 2] = ny.z, ny2[4 * g + 3] = ny.w;
            }
            apply_relu_deep<KIND == NSVD_DOT_RELU_NTK>(sv, nx2, ny2, mp.gamma, mp.coef0, mp.degree, kv);
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 ny = *(const float4*)(yb + 64 * yld + jb + 8 * g + kq);
                kv[4 * g] = apply_arccos1(sv[4 * g], nx, ny.x);
                kv[4 * g + 1] = apply_arccos1(sv[4 * g + 1], nx, ny.y);
                kv[4 * g + 2] = apply_arccos1(sv[4 * g + 2], nx, ny.z);
                kv[4 * g + 3] = apply_arccos1(sv[4 * g + 3], nx, ny.w);
            }
        }
        if (c == chunks - 1) {
            // padded reference rows: f^T is 0 there, but k (coef0^degree of a huge coef0) need not be finite (and the deep
            // ReLU kinds give a padded zero row k = coef0-derived values: 0 * k is right only while k is finite)
            const int jg = c * KC + jb + kq;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (jg + 8 * (r >> 2) + (r & 3) >= B2) kv[r] = 0.f;
        }
        float* la = buf + (ib + (lane & 31)) * LDT + jb + kq;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *(float4*)(la + 8 * g) = make_float4(kv[4 * g], kv[4 * g + 1], kv[4 * g + 2], kv[4 * g + 3]);
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
        // the y buffer written here was last read in the first contraction of chunk c - 1: before the barrier of c - 1
        DOT_Y_PUT(par ^ 1)
        DOT_Y_LOAD(min(c + 2, c1 - 1))
        // one barrier per chunk, ordering LDS only: the loads just issued stay in flight
        apply_lds_barrier();
        apply_chunk_mfma(buf, ra, rb, kq, acc0, acc1, acc2, acc3);
    }
    const nsvd_f32x16 acc = (acc0 + acc1) + (acc2 + acc3);
    float* out = w.part + (size_t)slice * w.B1p * w.Lp;
    const int row0 = tb * T + (wv & 1) * 32, col = tl * T + (wv >> 1) * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) apply_store_acc(out, w.Lp, row0, col, lane, r, acc[r]);
}
#undef DOT_S_STEP
#undef DOT_X_LOAD
#undef DOT_Y_LOAD
#undef DOT_Y_PUT

size_t dot_lds_bytes(int Dp) { return (size_t)(NSVD_TNT_FLOATS + 2 * (64 * (Dp + 4) + 64)) * sizeof(float); }

}  // namespace

extern "C" size_t nsvd_dot_apply_workspace_bytes(int B1, int B2, int D, int L) {
    if (!apply_shape_ok(B1, B2, D, L) || D > APPLY_MAX_D) return 0;
    return carve(nullptr, B1, B2, D, L).bytes;
}

extern "C" int nsvd_dot_apply(const float* x, int B1, const float* y, int B2, int D, const float* f, int L, int kind,
                              float gamma, float coef0, int degree, float scale, float* out, void* ws, size_t ws_bytes,
                              void* stream) {
    if (!apply_args_ok({x, y, f, out, ws}, B1, B2, D, L)) return NSVD_EINVAL;
    if (!apply_dot_kind_ok(kind, gamma, coef0, degree)) return NSVD_EINVAL;
    if (D > APPLY_MAX_D) return NSVD_EUNSUPPORTED;
    const DotWs w = carve(ws, B1, B2, D, L);
    if (!nsvd_ws_ok(ws, ws_bytes, w.bytes)) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ApplyPrep pr = {};
    pr.s[0] = {y, w.yP, w.yN, f, w.fT, B2, w.B2p};  // (|y|^2: the main kernel takes the root at staging)
    pr.D = D, pr.Dp = w.Dp, pr.L = L, pr.Lp = w.Lp;
    apply_prep_launch(pr, s);
    NSVD_CHECK_LAUNCH();
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)dot_main_kernel<NSVD_DOT_POLYNOMIAL>,
                                                    (const void*)dot_main_kernel<NSVD_DOT_ARCCOS1>,
                                                    (const void*)dot_main_kernel<NSVD_DOT_RELU_NNGP>,
                                                    (const void*)dot_main_kernel<NSVD_DOT_RELU_NTK>},
                                                   dot_lds_bytes(APPLY_MAX_D)))
        return rc;
    const dim3 grid(w.B1p / T, w.Lp / T, w.S);
    const DotMap mp = {gamma, coef0, degree};
    nsvd_prof_begin(s);
    if (kind == NSVD_DOT_POLYNOMIAL)
        dot_main_kernel<NSVD_DOT_POLYNOMIAL><<<grid, 256, dot_lds_bytes(w.Dp), s>>>(x, B1, B2, D, w, mp);
    else if (kind == NSVD_DOT_ARCCOS1)
        dot_main_kernel<NSVD_DOT_ARCCOS1><<<grid, 256, dot_lds_bytes(w.Dp), s>>>(x, B1, B2, D, w, mp);
    else if (kind == NSVD_DOT_RELU_NNGP)
        dot_main_kernel<NSVD_DOT_RELU_NNGP><<<grid, 256, dot_lds_bytes(w.Dp), s>>>(x, B1, B2, D, w, mp);
    else
        dot_main_kernel<NSVD_DOT_RELU_NTK><<<grid, 256, dot_lds_bytes(w.Dp), s>>>(x, B1, B2, D, w, mp);
    nsvd_prof_end(s);
    NSVD_CHECK_LAUNCH();
    const size_t n = (size_t)B1 * L;
    apply_reduce_kernel<><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(w.part, w.S, w.B1p, w.Lp, B1, L, scale, out);
    NSVD_CHECK_LAUNCH();
    return 0;
}
