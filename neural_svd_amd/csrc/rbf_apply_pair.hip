// Two-sided matrix-free radial kernel operator on coordinate batches - both halves of a kernel SVD step in one pass:
//     out_x[i][l] = scale_g * sum_j k(|x_i - y_j|) g[j][l]        (B1, L)   "K g"
//     out_y[j][l] = scale_f * sum_i k(|x_i - y_j|) f[i][l]        (B2, L)   "K^T f"
// - the (Tg, Tadjf) producer of NestedLoRALossFunctionSVD(f, Tg, g, Tadjf) (methods/nestedlora.py:100-156) for a
// cross-domain kernel k(x, y), x ~ p_x, y ~ p_y; restated in float64 by tests/_pair_oracle.py. Two nsvd_rbf_apply calls
// with swapped arguments evaluate every k(x_i, y_j) twice, and the distances (VALU) are what bounds that kernel above
// D = 16. Here each kernel value is evaluated ONCE per 64-head tile and feeds both contractions.
//
// A workgroup (row group, head tile, column group) owns a run of 64-row x tiles and a run of SLICES of at most four
// 64-row y chunks. Per slice it walks its x tiles; per (x tile, chunk) it
//   1. forms the 64 x 64 kernel values exactly as rbf_main_kernel does (direct differences, lane = x row, the wave's 16
//      y rows wave-uniform through scalar loads, one v_exp_f32 per pair, the same exponent constant);
//   2. writes them ONCE into LDS, x-row major (tile_nt.h's A layout);
//   3. contracts them with the g^T chunk into the K g accumulators of the x tile (b128 reads, as rbf_main_kernel), and
//   4. reads the SAME copy column-wise (32-bit reads, which the compiler pairs into ds_read2_b32: 32 consecutive y rows
//      of one x row are 32 consecutive banks)
//      against the f^T tile of the x rows into the K^T f accumulators of the chunk. Those (4 chunks x 16 registers) stay
//      in registers over the whole run of x tiles.
// K g tiles are flushed per x tile into the partial copy of the workgroup's column group (added to what the SAME thread
// stored for its previous slice: memory only this workgroup touches), K^T f tiles once per slice into the partial copy of
// its row group. apply_pair_reduce_kernel (apply_common.h) adds the copies in group order: no atomics, bit-reproducible, at most
// PAIR_MAX_GROUPS copies of either output whatever the shape.
// LDS is single-buffered (kernel chunk, g^T chunk, f^T tile, x tile: 68 KB at D = 64) so that two workgroups share a CU
// and one's distances run under the other's MFMAs; two LDS-only barriers per chunk, none for the x tile or the f^T tile
// (they are rewritten between the two barriers of a chunk, when no wave can be reading them).
#include "apply_common.h"
#include "pair_split.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;
constexpr int PAIR_TILE = T * LDT;   // one 64 x 64 LDS tile with padded rows

struct PairWs {
    float* yP;     // (B2p, Dp) y coordinates, zero padded (padded coordinates add 0 to every distance)
    float* gT;     // (Lp, B2p) g transposed, zero padded (padded y rows contribute k * 0 to K g)
    float* fT;     // (Lp, B1p) f transposed, zero padded (padded x rows contribute k * 0 to K^T f)
    float* partX;  // (CG, B1p, Lp) partial K g
    float* partY;  // (RG, B2p, Lp) partial K^T f
    int B1p, B2p, Dp, Lp, RG, CG;
    size_t bytes;
};

PairWs carve(void* base, int B1, int B2, int D, int L) {
    const ApplyPad pd = apply_pad(B1, B2, D, L, 4);
    PairWs w;
    w.B1p = pd.B1p, w.B2p = pd.B2p, w.Dp = pd.Dp, w.Lp = pd.Lp;
    pair_split(w.B1p / T, nsvd_cdiv(w.B2p / KC, PAIR_SLICE), w.Lp / T, &w.RG, &w.CG);
    NsvdArena a(base);
    w.yP = a.take((size_t)w.B2p * w.Dp);
    w.gT = a.take((size_t)w.Lp * w.B2p);
    w.fT = a.take((size_t)w.Lp * w.B1p);
    w.partX = a.take((size_t)w.CG * w.B1p * w.Lp);
    w.partY = a.take((size_t)w.RG * w.B2p * w.Lp);
    w.bytes = a.off;
    return w;
}

struct PairLane {
    int lane, wv, ra, rb, kq, lr0, lc, Dq, xld;
};

// One (x tile, chunk) step. ks: kernel chunk [x row][y row]; gs: g^T chunk [head][y row]; fs: f^T tile [head][x row];
// xs: x tile. gb*: the g^T chunk of THIS step in registers on entry, the one at gnext on exit. fb (first chunk of an x
// tile only, stage_f): the f^T tile to stage. stage_x (last chunk of an x tile that has a successor): stage the x tile
// of rows xrow0.. for the next tile.
template <int KIND>
__device__ __forceinline__ void pair_step(const PairLane& p, float* __restrict__ ks, float* __restrict__ gs,
                                          float* __restrict__ fs, float* __restrict__ xs,
                                          const float4* __restrict__ yq, float cexp, float4& gb0, float4& gb1,
                                          float4& gb2, float4& gb3, const float* __restrict__ gnext, size_t gr,
                                          bool stage_f, const float4& fb0, const float4& fb1, const float4& fb2,
                                          const float4& fb3, const float* __restrict__ x, int B1, int D, int Dp,
                                          int xrow0, bool stage_x, nsvd_f32x16& ax0, nsvd_f32x16& ax1,
                                          nsvd_f32x16& ay) {
    // squared distances of row `lane` of the x tile to the 16 y rows of this wave
    const float4* xq = (const float4*)(xs + p.lane * p.xld);
    float d2[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) d2[jj] = 0.f;
    for (int q = 0; q < p.Dq; ++q) {
        const float4 xv = xq[q];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const float4 yv = yq[(size_t)jj * p.Dq + q];
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
    // every wave is done with the previous step's kernel chunk, g^T chunk and f^T tile, and with this step's x tile
    apply_lds_barrier();
    float* la = ks + p.lane * LDT + 16 * p.wv;
#pragma unroll
    for (int i = 0; i < 4; ++i) *(float4*)(la + 4 * i) = make_float4(kv[4 * i], kv[4 * i + 1], kv[4 * i + 2], kv[4 * i + 3]);
    float* lb = gs + p.lr0 * LDT + p.lc;
    *(float4*)(lb) = gb0;
    *(float4*)(lb + 16 * LDT) = gb1;
    *(float4*)(lb + 32 * LDT) = gb2;
    *(float4*)(lb + 48 * LDT) = gb3;
    gb0 = *(const float4*)gnext;
    gb1 = *(const float4*)(gnext + gr);
    gb2 = *(const float4*)(gnext + 2 * gr);
    gb3 = *(const float4*)(gnext + 3 * gr);
    if (stage_f) {
        float* lf = fs + p.lr0 * LDT + p.lc;
        *(float4*)(lf) = fb0;
        *(float4*)(lf + 16 * LDT) = fb1;
        *(float4*)(lf + 32 * LDT) = fb2;
        *(float4*)(lf + 48 * LDT) = fb3;
    }
    if (stage_x) {
        for (int e = threadIdx.x; e < 64 * Dp; e += 256) {
            const int i = e / Dp, d = e - i * Dp;
            const int r = xrow0 + i;
            xs[i * p.xld + d] = (r < B1 && d < D) ? x[(size_t)r * D + d] : 0.f;
        }
    }
    apply_lds_barrier();
    // K g: rows = x rows (b128 along y), columns = heads of g^T;  K^T f: rows = y rows (b32 down the x rows of the same
    // copy), columns = heads of f^T. MFMA e of group s contracts k = 8 s + e (lanes 0-31) and 8 s + 4 + e (lanes 32-63).
    const float* pa = ks + p.ra * LDT + p.kq;
    const float* pg = gs + p.rb * LDT + p.kq;
    const float* pt = ks + p.kq * LDT + p.ra;
    const float* pf = fs + p.rb * LDT + p.kq;
#pragma unroll
    for (int s = 0; s < KC / 8; ++s) {
        const float4 av = *(const float4*)(pa + s * 8), gv = *(const float4*)(pg + s * 8);
        const float4 fv = *(const float4*)(pf + s * 8);
        const float t0 = pt[(s * 8 + 0) * LDT], t1 = pt[(s * 8 + 1) * LDT], t2 = pt[(s * 8 + 2) * LDT],
                    t3 = pt[(s * 8 + 3) * LDT];
        ax0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, gv.x, ax0, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t0, fv.x, ay, 0, 0, 0);
        ax1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, gv.y, ax1, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t1, fv.y, ay, 0, 0, 0);
        ax0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, gv.z, ax0, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t2, fv.z, ay, 0, 0, 0);
        ax1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, gv.w, ax1, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t3, fv.w, ay, 0, 0, 0);
    }
}

// store (first == true) or add-and-store the wave's 32 x 32 tile at rows row0.., column col of a (rows, Lp) partial copy
__device__ __forceinline__ void pair_flush(float* __restrict__ part, int Lp, int row0, int col, int lane,
                                           const nsvd_f32x16& acc, bool first) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
        float* q = part + (size_t)row * Lp + col;
        *q = first ? acc[r] : *q + acc[r];
    }
}

// grid (RG, Lp / 64, CG). LDS: kernel chunk | g^T chunk | f^T tile (PAIR_TILE floats each) | x tile (64, Dp + 4).
// cexp: log2 e / (2 ell^2) (Gaussian) or log2 e / ell (exponential)
template <int KIND>
__global__ void __launch_bounds__(256, 2) rbf_pair_main_kernel(const float* __restrict__ x, int B1, int D, PairWs w,
                                                               float cexp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ks = lds, *gs = lds + PAIR_TILE, *fs = lds + 2 * PAIR_TILE, *xs = lds + 3 * PAIR_TILE;
    const int rg = blockIdx.x, tl = blockIdx.y, cg = blockIdx.z;
    const int xtiles = w.B1p / T, chunks = w.B2p / KC, slices = (chunks + PAIR_SLICE - 1) / PAIR_SLICE;
    const int xt0 = (int)((long)xtiles * rg / w.RG), xt1 = (int)((long)xtiles * (rg + 1) / w.RG);
    const int s0 = (int)((long)slices * cg / w.CG), s1 = (int)((long)slices * (cg + 1) / w.CG);
    const int t = threadIdx.x;
    PairLane p;
    p.lane = t & 63;
    p.wv = __builtin_amdgcn_readfirstlane(t >> 6);  // (uniform by construction; tells the compiler so)
    p.ra = (p.wv & 1) * 32 + (p.lane & 31);
    p.rb = (p.wv >> 1) * 32 + (p.lane & 31);
    p.kq = (p.lane >> 5) * 4;
    p.lr0 = t >> 4;
    p.lc = (t & 15) * 4;
    const int Dp = w.Dp;
    p.Dq = Dp >> 2;
    p.xld = Dp + 4;
    const size_t gr = (size_t)16 * w.B2p, fr = (size_t)16 * w.B1p;
    const float* gp = w.gT + ((size_t)tl * T + p.lr0) * w.B2p + p.lc;
    const float* fp = w.fT + ((size_t)tl * T + p.lr0) * w.B1p + p.lc;
    const int col = tl * T + (p.wv >> 1) * 32 + (p.lane & 31), rsub = (p.wv & 1) * 32;
    float* px = w.partX + (size_t)cg * w.B1p * w.Lp;
    float* py = w.partY + (size_t)rg * w.B2p * w.Lp;
    for (int sl = s0; sl < s1; ++sl) {
        const int cb = sl * PAIR_SLICE;
        const int nc = min(PAIR_SLICE, chunks - cb);
        nsvd_f32x16 ay0 = {0}, ay1 = {0}, ay2 = {0}, ay3 = {0};  // one chain each: the K g MFMAs run between
        // the first x tile of the run (the loop below stages every later one under a chunk's barriers)
        __syncthreads();
        for (int e = t; e < 64 * Dp; e += 256) {
            const int i = e / Dp, d = e - i * Dp;
            const int r = xt0 * T + i;
            xs[i * p.xld + d] = (r < B1 && d < D) ? x[(size_t)r * D + d] : 0.f;
        }
        __syncthreads();
        const float* gc = gp + (size_t)cb * KC;
        float4 gb0 = *(const float4*)gc, gb1 = *(const float4*)(gc + gr), gb2 = *(const float4*)(gc + 2 * gr),
               gb3 = *(const float4*)(gc + 3 * gr);
        for (int xt = xt0; xt < xt1; ++xt) {
            const float* fc = fp + (size_t)xt * T;
            const float4 fb0 = *(const float4*)fc, fb1 = *(const float4*)(fc + fr), fb2 = *(const float4*)(fc + 2 * fr),
                         fb3 = *(const float4*)(fc + 3 * fr);
            nsvd_f32x16 ax0 = {0}, ax1 = {0};
            const bool more = xt + 1 < xt1;
            const int xn = (xt + 1) * T;
            const float4* yq = (const float4*)w.yP + ((size_t)cb * KC + 16 * p.wv) * p.Dq;
            const size_t ystep = (size_t)KC * p.Dq;
            // (g^T runs one chunk ahead: after the slice's last chunk comes its first again, for the next x tile)
            pair_step<KIND>(p, ks, gs, fs, xs, yq, cexp, gb0, gb1, gb2, gb3, gc + (nc > 1 ? KC : 0), gr, true, fb0, fb1,
                            fb2, fb3, x, B1, D, Dp, xn, more && nc == 1, ax0, ax1, ay0);
            if (nc > 1)
                pair_step<KIND>(p, ks, gs, fs, xs, yq + ystep, cexp, gb0, gb1, gb2, gb3, gc + (nc > 2 ? 2 * KC : 0), gr,
                                false, fb0, fb1, fb2, fb3, x, B1, D, Dp, xn, more && nc == 2, ax0, ax1, ay1);
            if (nc > 2)
                pair_step<KIND>(p, ks, gs, fs, xs, yq + 2 * ystep, cexp, gb0, gb1, gb2, gb3, gc + (nc > 3 ? 3 * KC : 0),
                                gr, false, fb0, fb1, fb2, fb3, x, B1, D, Dp, xn, more && nc == 3, ax0, ax1, ay2);
            if (nc > 3)
                pair_step<KIND>(p, ks, gs, fs, xs, yq + 3 * ystep, cexp, gb0, gb1, gb2, gb3, gc, gr, false, fb0, fb1, fb2,
                                fb3, x, B1, D, Dp, xn, more, ax0, ax1, ay3);
            pair_flush(px, w.Lp, xt * T + rsub, col, p.lane, ax0 + ax1, sl == s0);
        }
        const int yrow = cb * KC + rsub;
        pair_flush(py, w.Lp, yrow, col, p.lane, ay0, true);
        if (nc > 1) pair_flush(py, w.Lp, yrow + KC, col, p.lane, ay1, true);
        if (nc > 2) pair_flush(py, w.Lp, yrow + 2 * KC, col, p.lane, ay2, true);
        if (nc > 3) pair_flush(py, w.Lp, yrow + 3 * KC, col, p.lane, ay3, true);
    }
}

size_t pair_lds_bytes(int Dp) { return (size_t)(3 * PAIR_TILE + 64 * (Dp + 4)) * sizeof(float); }

}  // namespace

extern "C" size_t nsvd_rbf_apply_pair_workspace_bytes(int B1, int B2, int D, int L) {
    if (!apply_shape_ok(B1, B2, D, L) || D > APPLY_MAX_D) return 0;
    return carve(nullptr, B1, B2, D, L).bytes;
}

extern "C" int nsvd_rbf_apply_pair_partition(int B1, int B2, int D, int L, int* row_groups, int* col_slices) {
    return apply_pair_partition(carve, B1, B2, D, L, row_groups, col_slices);
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
    const size_t n = (size_t)(B1 + (size_t)B2) * L;
    apply_pair_reduce_kernel<><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(
        w.partX, w.CG, w.B1p, w.partY, w.RG, w.B2p, w.Lp, B1, B2, L, scale_g, scale_f, out_x, out_y);
    NSVD_CHECK_LAUNCH();
    return 0;
}
