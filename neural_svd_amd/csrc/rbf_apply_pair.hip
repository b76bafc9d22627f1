// Two-sided matrix-free radial kernel operator on coordinate batches - both halves of a kernel SVD step in one pass:
//     out_x[i][l] = scale_g * sum_j k(|x_i - y_j|) g[j][l]        (B1, L)   "K g"
//     out_y[j][l] = scale_f * sum_i k(|x_i - y_j|) f[i][l]        (B2, L)   "K^T f"
// - the (Tg, Tadjf) producer of NestedLoRALossFunctionSVD(f, Tg, g, Tadjf) (methods/nestedlora.py:100-156) for a
// cross-domain kernel k(x, y), x ~ p_x, y ~ p_y; restated in float64 by tests/_pair_oracle.py. Two nsvd_rbf_apply calls
// with swapped arguments evaluate every k(x_i, y_j) twice, and the distances (VALU) are what bounds that kernel above
// D = 16. Here each kernel value is evaluated ONCE per 64-head tile and feeds both contractions.
//
// The workgroup, its runs of x tiles and slices, the walk over them, the two-sided contraction, the partial copies and
// their reduce are pair_common.h's (pair_walk). What is particular here: per (x tile, chunk) a step
//   1. forms the 64 x 64 kernel values exactly as rbf_main_kernel does (direct differences, lane = x row, the wave's 16
//      y rows wave-uniform through scalar loads, one v_exp_f32 per pair, the same exponent constant);
//   2. writes them ONCE into LDS, x-row major (tile_nt.h's A layout), beside the g^T chunk that ran one chunk ahead in
//      registers, the f^T tile (first chunk of an x tile) and the next x tile (last chunk), and contracts (pair_contract).
// LDS is single-buffered (kernel chunk, g^T chunk, f^T tile, x tile: 68 KB at D = 64) so that two workgroups share a CU
// and one's distances run under the other's MFMAs; two LDS-only barriers per chunk, none for the x tile or the f^T tile
// (they are rewritten between the two barriers of a chunk, when no wave can be reading them).
#include "pair_common.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;

struct PairWs : PairParts {
    float* yP;  // (B2p, Dp) y coordinates, zero padded (padded coordinates add 0 to every distance)
    float* gT;  // (Lp, B2p) g transposed, zero padded (padded y rows contribute k * 0 to K g)
    float* fT;  // (Lp, B1p) f transposed, zero padded (padded x rows contribute k * 0 to K^T f)
    int Dp;
    size_t bytes;
};

PairWs carve(void* base, int B1, int B2, int D, int L) {
    const ApplyPad pd = apply_pad(B1, B2, D, L, 4);
    PairWs w;
    w.Dp = pd.Dp;
    NsvdArena a(base);
    w.yP = a.take((size_t)pd.B2p * pd.Dp);
    w.gT = a.take((size_t)pd.Lp * pd.B2p);
    w.fT = a.take((size_t)pd.Lp * pd.B1p);
    static_cast<PairParts&>(w) = pair_parts(a, pd.B1p, pd.B2p, pd.Lp);
    w.bytes = a.off;
    return w;
}

// rows row0 .. row0 + 63 of x into the x tile (rows of Dp + 4 floats), zero padded
__device__ __forceinline__ void pair_stage_x(float* __restrict__ xs, const float* __restrict__ x, int B1, int D, int Dp,
                                             int row0) {
    for (int e = threadIdx.x; e < 64 * Dp; e += 256) {
        const int i = e / Dp, d = e - i * Dp;
        const int r = row0 + i;
        xs[i * (Dp + 4) + d] = (r < B1 && d < D) ? x[(size_t)r * D + d] : 0.f;
    }
}

// kv[jj] = k(|x_lane - y_jj|) for row `lane` of the x tile and the 16 y rows at yq (wave-uniform: scalar loads), formed
// exactly as rbf_main_kernel forms them: direct differences, one v_exp_f32 per pair, the same exponent constant
template <int KIND>
__device__ __forceinline__ void pair_values(const float* __restrict__ xs, int lane, int Dp,
                                            const float4* __restrict__ yq, float cexp, float (&kv)[16]) {
    const int Dq = Dp >> 2;
    const float4* xq = (const float4*)(xs + lane * (Dp + 4));
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
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) kv[jj] = apply_radial<KIND>(d2[jj], cexp);
}

// grid (RG, Lp / 64, CG). LDS: kernel chunk [x row][y row] | g^T chunk [head][y row] | f^T tile [head][x row]
// (PAIR_TILE floats each) | x tile (64, Dp + 4). cexp: log2 e / (2 ell^2) (Gaussian) or log2 e / ell (exponential)
template <int KIND>
__global__ void __launch_bounds__(256, 2) rbf_pair_main_kernel(const float* __restrict__ x, int B1, int D, PairWs w,
                                                               float cexp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ks = lds, *gs = lds + PAIR_TILE, *fs = lds + 2 * PAIR_TILE, *xs = lds + 3 * PAIR_TILE;
    const PairLane p = pair_lane(threadIdx.x);
    const int tl = blockIdx.y, Dp = w.Dp, so = p.lr0 * LDT + p.lc;
    // this thread's first float4 of a g^T chunk / an f^T tile at column 0; its other three are 16 rows further each
    const size_t gr = (size_t)16 * w.B2p, fr = (size_t)16 * w.B1p;
    const float* gp = w.gT + ((size_t)tl * T + p.lr0) * w.B2p + p.lc;
    const float* fp = w.fT + ((size_t)tl * T + p.lr0) * w.B1p + p.lc;
    const size_t ystep = (size_t)KC * (Dp >> 2);
    PairQuad gb, fb;     // the g^T chunk of the coming step; the f^T tile of the x tile under way
    const float* gc;     // the slice's first chunk of g^T
    const float4* yq;    // ... and of y: the 16 rows of this wave
    int xnext;           // first row of the next x tile, staged by the last step of a tile that has a successor
    bool more;
    pair_walk(
        p, w, tl,
        [&](int cb, int xt0) {
            // the first x tile of the run (the steps stage every later one under a chunk's barriers)
            __syncthreads();
            pair_stage_x(xs, x, B1, D, Dp, xt0 * T);
            __syncthreads();
            gc = gp + (size_t)cb * KC;
            gb = pair_load(gc, gr);
            yq = (const float4*)w.yP + ((size_t)cb * KC + 16 * p.wv) * (Dp >> 2);
        },
        [&](int xt, bool more_) {
            fb = pair_load(fp + (size_t)xt * T, fr);
            xnext = (xt + 1) * T, more = more_;
        },
        [&](int q, int qn, bool last, nsvd_f32x16& ax0, nsvd_f32x16& ax1, nsvd_f32x16& ay) {
            float kv[16];
            pair_values<KIND>(xs, p.lane, Dp, yq + q * ystep, cexp, kv);
            // every wave is done with the previous step's kernel chunk, g^T chunk and f^T tile, and with this step's x
            // tile
            apply_lds_barrier();
            float* la = ks + p.lane * LDT + 16 * p.wv;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *(float4*)(la + 4 * i) = make_float4(kv[4 * i], kv[4 * i + 1], kv[4 * i + 2], kv[4 * i + 3]);
            pair_put(gs + so, gb);
            gb = pair_load(gc + qn * KC, gr);
            // (no barrier of their own for the f^T tile and the x tile: they are rewritten between the two barriers of
            // a chunk, when no wave can be reading them)
            if (q == 0) pair_put(fs + so, fb);
            if (more && last) pair_stage_x(xs, x, B1, D, Dp, xnext);
            apply_lds_barrier();
            pair_contract(p, ks, gs, fs, ax0, ax1, ay);
        });
}

size_t pair_lds_bytes(int Dp) { return (size_t)(3 * PAIR_TILE + 64 * (Dp + 4)) * sizeof(float); }

}  // namespace

extern "C" size_t nsvd_rbf_apply_pair_workspace_bytes(int B1, int B2, int D, int L) {
    if (!apply_shape_ok(B1, B2, D, L) || D > APPLY_MAX_D) return 0;
    return carve(nullptr, B1, B2, D, L).bytes;
}

extern "C" int nsvd_rbf_apply_pair_partition(int B1, int B2, int D, int L, int* row_groups, int* col_slices) {
    return pair_partition(apply_shape_ok(B1, B2, D, L), D <= APPLY_MAX_D, row_groups, col_slices,
                          [&] { return carve(nullptr, B1, B2, D, L); });
}

extern "C" int nsvd_rbf_apply_pair(const float* x, int B1, const float* y, int B2, int D, const float* g, const float* f,
                                   int L, int kind, float ell, float scale_g, float scale_f, float* out_x, float* out_y,
                                   void* ws, size_t ws_bytes, void* stream) {
    if (!apply_args_ok({x, y, g, f, out_x, out_y, ws}, B1, B2, D, L)) return NSVD_EINVAL;
    if (kind != NSVD_RBF_GAUSSIAN && kind != NSVD_RBF_EXPONENTIAL) return NSVD_EINVAL;
    if (!(ell > 0.f)) return NSVD_EINVAL;  // (also NaN)
    if (D > APPLY_MAX_D) return NSVD_EUNSUPPORTED;
    const PairWs w = carve(ws, B1, B2, D, L);
    if (!nsvd_ws_ok(ws, ws_bytes, w.bytes)) return NSVD_EINVAL;
    const float cexp = apply_radial_cexp(kind, ell);
    hipStream_t s = (hipStream_t)stream;
    ApplyPrep pr = {};
    pr.s[0] = {y, w.yP, nullptr, g, w.gT, B2, w.B2p};
    pr.s[1] = {nullptr, nullptr, nullptr, f, w.fT, B1, w.B1p};  // (the main kernel stages x itself)
    pr.D = D, pr.Dp = w.Dp, pr.L = L, pr.Lp = w.Lp;
    apply_prep_launch(pr, s);
    NSVD_CHECK_LAUNCH();
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)rbf_pair_main_kernel<NSVD_RBF_GAUSSIAN>,
                                                    (const void*)rbf_pair_main_kernel<NSVD_RBF_EXPONENTIAL>},
                                                   pair_lds_bytes(APPLY_MAX_D)))
        return rc;
    const dim3 grid(w.RG, w.Lp / T, w.CG);
    nsvd_prof_begin(s);
    if (kind == NSVD_RBF_GAUSSIAN)
        rbf_pair_main_kernel<NSVD_RBF_GAUSSIAN><<<grid, 256, pair_lds_bytes(w.Dp), s>>>(x, B1, D, w, cexp);
    else
        rbf_pair_main_kernel<NSVD_RBF_EXPONENTIAL><<<grid, 256, pair_lds_bytes(w.Dp), s>>>(x, B1, D, w, cexp);
    nsvd_prof_end(s);
    NSVD_CHECK_LAUNCH();
    pair_reduce_launch(w, B1, B2, L, scale_g, scale_f, out_x, out_y, s);
    NSVD_CHECK_LAUNCH();
    return 0;
}
