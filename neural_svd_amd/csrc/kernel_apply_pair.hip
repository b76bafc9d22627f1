// Two-sided dense operator on index batches - both halves of an SVD step on a STORED (N1 x N2) matrix in one pass:
//     out_x[i][l] = scale_g * sum_k A[rows_i][cols_k] g[k][l]        (B1, L)   "A g"
//     out_y[k][l] = scale_f * sum_i A[rows_i][cols_k] f[i][l]        (B2, L)   "A^T f"
// - the (Tg, Tadjf) producer of NestedLoRALossFunctionSVD(f, Tg, g, Tadjf) (methods/nestedlora.py:100-156) for a matrix
// the caller holds (rectangular, not symmetric); restated in float64 by tests/_dense_pair_oracle.py. Two nsvd_kernel_apply
// calls would need a transposed copy of A and stream the gathered rows twice; here there is no transpose anywhere.
// Form used, as kernel_apply.hip: g is scattered into the column index space, Sg^T[l][j] = sum_{k: cols_k = j} g[k][l]
// (scatter_blocks.h: no atomics, duplicates added in batch order), so that
//     A g      = A[rows, :] Sg                  (B1 x N2p) . (N2p x L)
//     A^T f    = gather_cols(U),  U = A[rows, :]^T f      (N2p x B1) . (B1 x L)
// are two contractions over the SAME gathered rows of A. f^T is staged zero padded, rows whose index is out of range
// zeroed (such a row is read from row 0 of A and must add nothing to U).
//
// The main kernel is rbf_apply_pair.hip's with the kernel values read instead of computed. A workgroup (row group, head
// tile, column group) owns a run of 64-row tiles of gathered rows and a run of SLICES of at most four 64-column chunks
// of [0, N2p). Per slice it walks its row tiles; per (row tile, chunk) it
//   1. writes the 64 x 64 block of A ONCE into LDS, row major (tile_nt.h's A layout), from registers that were loaded one
//      step ahead (a thread holds 4 float4: rows (t >> 4) + 16 i, columns 4 (t & 15) .. +3 of the chunk);
//   2. contracts it row-wise with the Sg^T chunk into the A g accumulators of the row tile (b128 reads), and
//   3. reads the SAME copy column-wise (32-bit reads: 32 consecutive columns of one row are 32 consecutive banks)
//      against the f^T tile of the rows into the U accumulators of the chunk. Those (4 chunks x 16 registers) stay in
//      registers over the whole run of row tiles.
// A g tiles are flushed per row tile into the partial copy of the workgroup's column group (added to what the SAME thread
// stored for its previous slice), U tiles once per slice into the partial copy of its row group. kap_reduce_kernel adds
// the copies in group order and gathers out_y[k] = scale_f U[cols_k]: no atomics, bit-reproducible, at most
// PAIR_MAX_GROUPS copies of either product whatever the shape.
// LDS is single-buffered (A block, Sg^T chunk, f^T tile: 51 KB) so that two workgroups share a CU and one's staging runs
// under the other's MFMAs; two LDS-only barriers per chunk.
// All index arithmetic into A is 64-bit.
// Built into libnsvd_dense.so on its own (include/nsvd_dense.h): everything it shares with libnsvd_hip.so is in headers.
#include "../../include/nsvd_dense.h"
#include "apply_common.h"
#include "pair_split.h"
#include "scatter_blocks.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;
constexpr int PAIR_TILE = T * LDT;   // one 64 x 64 LDS tile with padded rows

struct KapWs {
    float* SgT;    // (Lp, N2p) g scattered into the column index space, zero padded
    float* fT;     // (Lp, B1p) f transposed, zero padded, rows with an index outside [0, N1) zeroed
    float* partX;  // (CG, B1p, Lp) partial A g
    float* partY;  // (RG, N2p, Lp) partial U = A[rows, :]^T f
    int B1p, N2p, Lp, RG, CG;
    size_t bytes;
};

KapWs carve(void* base, int N2, int B1, int L) {
    KapWs w;
    w.B1p = nsvd_cdiv(B1, T) * T;
    w.N2p = nsvd_cdiv(N2, KC) * KC;
    w.Lp = nsvd_cdiv(L, T) * T;
    pair_split(w.B1p / T, nsvd_cdiv(w.N2p / KC, PAIR_SLICE), w.Lp / T, &w.RG, &w.CG);
    NsvdArena a(base);
    w.SgT = a.take((size_t)w.Lp * w.N2p);
    w.fT = a.take((size_t)w.Lp * w.B1p);
    w.partX = a.take((size_t)w.CG * w.B1p * w.Lp);
    w.partY = a.take((size_t)w.RG * w.N2p * w.Lp);
    w.bytes = a.off;
    return w;
}

bool shape_ok(int N1, int N2, int B1, int B2, int L) { return N1 > 0 && N2 > 0 && B1 > 0 && B2 > 0 && L > 0; }

// fT[l][r] = f[r][l] where rows[r] is a row of A, 0 elsewhere (and in the padding): grid (B1p / 64, Lp / 64)
__global__ void __launch_bounds__(256) kap_stage_f_kernel(const float* __restrict__ f, const long long* __restrict__ rows,
                                                          int N1, int B1, int L, float* __restrict__ fT, int B1p) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x, r0 = blockIdx.x * 64, l0 = blockIdx.y * 64;
    for (int e = t; e < 4096; e += 256) {
        const int rr = e >> 6, ll = e & 63;  // consecutive threads: consecutive heads of one row
        const int r = r0 + rr;
        bool ok = r < B1 && l0 + ll < L;
        if (ok) {
            const long long g = rows[r];
            ok = g >= 0 && g < N1;
        }
        tile[rr][ll] = ok ? f[(size_t)r * L + l0 + ll] : 0.f;
    }
    __syncthreads();
    for (int e = t; e < 4096; e += 256) {
        const int ll = e >> 6, rr = e & 63;
        fT[(size_t)(l0 + ll) * B1p + r0 + rr] = tile[rr][ll];
    }
}

// what a thread stages of a 64 x 64 operand block: rows (t >> 4) + 16 i, 4 consecutive floats each
struct Quad {
    float4 a, b, c, d;
};
struct Rows {
    const float *a, *b, *c, *d;
};
__device__ __forceinline__ Quad kap_load(const Rows& r, size_t off) {
    Quad q;
    q.a = *(const float4*)(r.a + off);
    q.b = *(const float4*)(r.b + off);
    q.c = *(const float4*)(r.c + off);
    q.d = *(const float4*)(r.d + off);
    return q;
}
__device__ __forceinline__ void kap_put(float* __restrict__ l, const Quad& q) {
    *(float4*)(l) = q.a;
    *(float4*)(l + 16 * LDT) = q.b;
    *(float4*)(l + 32 * LDT) = q.c;
    *(float4*)(l + 48 * LDT) = q.d;
}
__device__ __forceinline__ Rows kap_strided(const float* p, size_t stride16) {
    return {p, p + stride16, p + 2 * stride16, p + 3 * stride16};
}
// the four rows of A that this thread stages for the row tile at batch row r0 (its own row offset included), at its 4
// columns of chunk 0. Rows that only pad the tile and rows with an index outside [0, N1) read row 0 of A: their f^T is
// zero and their A g is never used.
__device__ __forceinline__ Rows kap_gather(const float* __restrict__ A, size_t lda, int N1,
                                           const long long* __restrict__ rows, int B1, int r0, int lc) {
    const float* p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + 16 * i;
        long long g = r < B1 ? rows[r] : 0;
        if (g < 0 || g >= N1) g = 0;
        p[i] = A + (size_t)g * lda + lc;
    }
    return {p[0], p[1], p[2], p[3]};
}

struct KapLane {
    int lane, wv, ra, rb, kq, lr0, lc;
};

// One (row tile, chunk) step. ks: block of A [row][column]; gs: Sg^T chunk [head][column]; fs: f^T tile [head][row].
// ab / gb: the operands of THIS step in registers on entry, those of the next step (read at anext + aoff / gnext) on
// exit. fb (first chunk of a row tile only, stage_f): the f^T tile to stage.
__device__ __forceinline__ void kap_step(const KapLane& p, float* __restrict__ ks, float* __restrict__ gs,
                                         float* __restrict__ fs, Quad& ab, const Rows& anext, size_t aoff, Quad& gb,
                                         const Rows& gnext, size_t goff, bool stage_f, const Quad& fb,
                                         nsvd_f32x16& ax0, nsvd_f32x16& ax1, nsvd_f32x16& ay) {
    // every wave is done with the previous step's block, Sg^T chunk and f^T tile
    apply_lds_barrier();
    const int so = p.lr0 * LDT + p.lc;
    kap_put(ks + so, ab);
    kap_put(gs + so, gb);
    ab = kap_load(anext, aoff);
    gb = kap_load(gnext, goff);
    if (stage_f) kap_put(fs + so, fb);
    apply_lds_barrier();
    // A g: rows = rows of the block (b128 along the columns), columns = heads of Sg^T;  U: rows = columns of the block
    // (b32 down the rows of the same copy), columns = heads of f^T. MFMA e of group s contracts k = 8 s + e (lanes
    // 0-31) and 8 s + 4 + e (lanes 32-63).
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
__device__ __forceinline__ void kap_flush(float* __restrict__ part, int Lp, int row0, int col, int lane,
                                          const nsvd_f32x16& acc, bool first) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
        float* q = part + (size_t)row * Lp + col;
        *q = first ? acc[r] : *q + acc[r];
    }
}

// grid (RG, Lp / 64, CG). LDS: block of A | Sg^T chunk | f^T tile (PAIR_TILE floats each)
__global__ void __launch_bounds__(256, 2) kap_main_kernel(const float* __restrict__ A, size_t lda, int N1,
                                                          const long long* __restrict__ rows, int B1, KapWs w) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ks = lds, *gs = lds + PAIR_TILE, *fs = lds + 2 * PAIR_TILE;
    const int rg = blockIdx.x, tl = blockIdx.y, cg = blockIdx.z;
    const int xtiles = w.B1p / T, chunks = w.N2p / KC, slices = (chunks + PAIR_SLICE - 1) / PAIR_SLICE;
    const int xt0 = (int)((long)xtiles * rg / w.RG), xt1 = (int)((long)xtiles * (rg + 1) / w.RG);
    const int s0 = (int)((long)slices * cg / w.CG), s1 = (int)((long)slices * (cg + 1) / w.CG);
    const int t = threadIdx.x;
    KapLane p;
    p.lane = t & 63;
    p.wv = __builtin_amdgcn_readfirstlane(t >> 6);  // (uniform by construction; tells the compiler so)
    p.ra = (p.wv & 1) * 32 + (p.lane & 31);
    p.rb = (p.wv >> 1) * 32 + (p.lane & 31);
    p.kq = (p.lane >> 5) * 4;
    p.lr0 = t >> 4;
    p.lc = (t & 15) * 4;
    const Rows gR = kap_strided(w.SgT + ((size_t)tl * T + p.lr0) * w.N2p + p.lc, (size_t)16 * w.N2p);
    const Rows fR = kap_strided(w.fT + ((size_t)tl * T + p.lr0) * w.B1p + p.lc, (size_t)16 * w.B1p);
    const int col = tl * T + (p.wv >> 1) * 32 + (p.lane & 31), rsub = (p.wv & 1) * 32;
    float* px = w.partX + (size_t)cg * w.B1p * w.Lp;
    float* py = w.partY + (size_t)rg * w.N2p * w.Lp;
    for (int sl = s0; sl < s1; ++sl) {
        const int cb = sl * PAIR_SLICE;
        const int nc = min(PAIR_SLICE, chunks - cb);
        const size_t c0 = (size_t)cb * KC;  // first column of the slice
        nsvd_f32x16 ay0 = {0}, ay1 = {0}, ay2 = {0}, ay3 = {0};  // one chain each: the A g MFMAs run between
        Rows ar = kap_gather(A, lda, N1, rows, B1, xt0 * T + p.lr0, p.lc);
        Quad ab = kap_load(ar, c0), gb = kap_load(gR, c0);
        for (int xt = xt0; xt < xt1; ++xt) {
            const Quad fb = kap_load(fR, (size_t)xt * T);
            // the rows of the NEXT tile: their indices are requested now and used behind the tile's last chunk (the last
            // tile of the run reads its own first chunk again; that copy is never consumed)
            const Rows an = xt + 1 < xt1 ? kap_gather(A, lda, N1, rows, B1, (xt + 1) * T + p.lr0, p.lc) : ar;
            nsvd_f32x16 ax0 = {0}, ax1 = {0};
            // (Sg^T runs one chunk ahead: after the slice's last chunk comes its first again, for the next row tile)
            kap_step(p, ks, gs, fs, ab, nc > 1 ? ar : an, nc > 1 ? c0 + KC : c0, gb, gR, nc > 1 ? c0 + KC : c0, true, fb,
                     ax0, ax1, ay0);
            if (nc > 1)
                kap_step(p, ks, gs, fs, ab, nc > 2 ? ar : an, nc > 2 ? c0 + 2 * KC : c0, gb, gR,
                         nc > 2 ? c0 + 2 * KC : c0, false, fb, ax0, ax1, ay1);
            if (nc > 2)
                kap_step(p, ks, gs, fs, ab, nc > 3 ? ar : an, nc > 3 ? c0 + 3 * KC : c0, gb, gR,
                         nc > 3 ? c0 + 3 * KC : c0, false, fb, ax0, ax1, ay2);
            if (nc > 3) kap_step(p, ks, gs, fs, ab, an, c0, gb, gR, c0, false, fb, ax0, ax1, ay3);
            kap_flush(px, w.Lp, xt * T + rsub, col, p.lane, ax0 + ax1, sl == s0);
            ar = an;
        }
        const int yrow = cb * KC + rsub;
        kap_flush(py, w.Lp, yrow, col, p.lane, ay0, true);
        if (nc > 1) kap_flush(py, w.Lp, yrow + KC, col, p.lane, ay1, true);
        if (nc > 2) kap_flush(py, w.Lp, yrow + 2 * KC, col, p.lane, ay2, true);
        if (nc > 3) kap_flush(py, w.Lp, yrow + 3 * KC, col, p.lane, ay3, true);
    }
}

// out_x[i] = scale_g * (sum of the CG copies of A g at row i), out_y[k] = scale_f * (sum of the RG copies of U at row
// cols_k), in copy order; a zero row where the index is outside its range
__global__ void __launch_bounds__(256) kap_reduce_kernel(KapWs w, const long long* __restrict__ rows, int N1,
                                                         const long long* __restrict__ cols, int N2, int B1, int B2,
                                                         int L, float scale_g, float scale_f, float* __restrict__ out_x,
                                                         float* __restrict__ out_y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nx = (size_t)B1 * L, ny = (size_t)B2 * L;
    if (i >= nx + ny) return;
    const bool isx = i < nx;
    const size_t e = isx ? i : i - nx;
    const size_t b = e / L, l = e - b * L;
    const long long g = isx ? rows[b] : cols[b];
    float* out = isx ? out_x : out_y;
    if (g < 0 || g >= (isx ? N1 : N2)) {
        out[e] = 0.f;
        return;
    }
    const float* part = isx ? w.partX : w.partY;
    const size_t Bp = isx ? w.B1p : w.N2p, pr = isx ? b : (size_t)g;
    const int n = isx ? w.CG : w.RG;
    float s = 0.f;
    for (int c = 0; c < n; ++c) s += part[((size_t)c * Bp + pr) * w.Lp + l];
    out[e] = (isx ? scale_g : scale_f) * s;
}

constexpr size_t KAP_LDS_BYTES = 3 * PAIR_TILE * sizeof(float);
static_assert(KAP_LDS_BYTES <= NSVD_LDS_MAX, "LDS of gfx950");

}  // namespace

extern "C" size_t nsvd_kernel_apply_pair_workspace_bytes(int N1, int N2, int B1, int B2, int L) {
    if (!shape_ok(N1, N2, B1, B2, L)) return 0;
    return carve(nullptr, N2, B1, L).bytes;
}

extern "C" int nsvd_kernel_apply_pair_partition(int N1, int N2, int B1, int B2, int L, int* row_groups,
                                                int* col_groups) {
    if (!row_groups || !col_groups || !shape_ok(N1, N2, B1, B2, L)) return NSVD_EINVAL;
    const KapWs w = carve(nullptr, N2, B1, L);
    *row_groups = w.RG;
    *col_groups = w.CG;
    return 0;
}

extern "C" int nsvd_kernel_apply_pair(const float* A, size_t lda, int N1, int N2, const long long* rows, int B1,
                                      const long long* cols, int B2, const float* g, const float* f, int L,
                                      float scale_g, float scale_f, float* out_x, float* out_y, void* ws,
                                      size_t ws_bytes, void* stream) {
    if (!A || !rows || !cols || !g || !f || !out_x || !out_y || !ws || !shape_ok(N1, N2, B1, B2, L))
        return NSVD_EINVAL;
    const KapWs w = carve(ws, N2, B1, L);
    // whole 64-float chunks of a row are read: the leading dimension must cover the padded width
    if (lda < (size_t)w.N2p || (lda & 3) != 0 || ((uintptr_t)A & 15) != 0) return NSVD_EINVAL;
    if (!nsvd_ws_ok(ws, ws_bytes, w.bytes)) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)kap_main_kernel}, KAP_LDS_BYTES)) return rc;
    ka_scatter_blocks_kernel<><<<dim3(w.N2p / KS_PB, w.Lp / 64), 256, 0, s>>>(g, cols, B2, L, N2, w.SgT, w.N2p);
    NSVD_CHECK_LAUNCH();
    kap_stage_f_kernel<<<dim3(w.B1p / 64, w.Lp / 64), 256, 0, s>>>(f, rows, N1, B1, L, w.fT, w.B1p);
    NSVD_CHECK_LAUNCH();
    kap_main_kernel<<<dim3(w.RG, w.Lp / T, w.CG), 256, KAP_LDS_BYTES, s>>>(A, lda, N1, rows, B1, w);
    NSVD_CHECK_LAUNCH();
    const size_t n = ((size_t)B1 + (size_t)B2) * L;
    kap_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(w, rows, N1, cols, N2, B1, B2, L, scale_g, scale_f,
                                                                  out_x, out_y);
    NSVD_CHECK_LAUNCH();
    return 0;
}
