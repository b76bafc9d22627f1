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
// The workgroup, its runs of row tiles and slices, the walk over them, the two-sided contraction and the partial copies
// are pair_common.h's (pair_walk), with the kernel values read instead of computed: a slice is at most four 64-column
// chunks of [0, N2p), and per (row tile, chunk) a step writes the 64 x 64 block of A ONCE into LDS, row major (tile_nt.h's
// A layout), from registers that were loaded one step ahead (a thread holds 4 float4: rows (t >> 4) + 16 i, columns
// 4 (t & 15) .. +3 of the chunk), beside the Sg^T chunk and, at the first chunk of a row tile, the f^T tile, and contracts
// (pair_contract: A g row-wise, U column-wise from the same copy).
// kap_reduce_kernel adds the partial copies in group order and gathers out_y[k] = scale_f U[cols_k]: no atomics,
// bit-reproducible, at most PAIR_MAX_GROUPS copies of either product whatever the shape.
// LDS is single-buffered (A block, Sg^T chunk, f^T tile: 51 KB) so that two workgroups share a CU and one's staging runs
// under the other's MFMAs; two LDS-only barriers per chunk.
// All index arithmetic into A is 64-bit.
// Built into libnsvd_dense.so on its own (include/nsvd_dense.h): everything it shares with libnsvd_hip.so is in headers.
#include "../../include/nsvd_dense.h"
#include "pair_common.h"
#include "scatter_blocks.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;

// (PairParts' B2p is N2p here: the padded columns of A stand in the place of the y rows)
struct KapWs : PairParts {
    float* SgT;  // (Lp, N2p) g scattered into the column index space, zero padded
    float* fT;   // (Lp, B1p) f transposed, zero padded, rows with an index outside [0, N1) zeroed
    size_t bytes;
};

KapWs carve(void* base, int N2, int B1, int L) {
    const int B1p = nsvd_cdiv(B1, T) * T, N2p = nsvd_cdiv(N2, KC) * KC, Lp = nsvd_cdiv(L, T) * T;
    KapWs w;
    NsvdArena a(base);
    w.SgT = a.take((size_t)Lp * N2p);
    w.fT = a.take((size_t)Lp * B1p);
    static_cast<PairParts&>(w) = pair_parts(a, B1p, N2p, Lp);
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

// the four rows of A that this thread stages for the row tile at batch row r0 (its own row offset included), at its 4
// columns of chunk 0. Rows that only pad the tile and rows with an index outside [0, N1) read row 0 of A: their f^T is
// zero and their A g is never used.
__device__ __forceinline__ PairRows kap_gather(const float* __restrict__ A, size_t lda, int N1,
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

// grid (RG, Lp / 64, CG). LDS: block of A [row][column] | Sg^T chunk [head][column] | f^T tile [head][row] (PAIR_TILE
// floats each)
__global__ void __launch_bounds__(256, 2) kap_main_kernel(const float* __restrict__ A, size_t lda, int N1,
                                                          const long long* __restrict__ rows, int B1, KapWs w) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ks = lds, *gs = lds + PAIR_TILE, *fs = lds + 2 * PAIR_TILE;
    const PairLane p = pair_lane(threadIdx.x);
    const int tl = blockIdx.y, so = p.lr0 * LDT + p.lc;
    const PairRows gR = pair_strided(w.SgT + ((size_t)tl * T + p.lr0) * w.B2p + p.lc, (size_t)16 * w.B2p);
    const PairRows fR = pair_strided(w.fT + ((size_t)tl * T + p.lr0) * w.B1p + p.lc, (size_t)16 * w.B1p);
    PairRows ar, an;  // this thread's rows of A for the row tile under way and for the next one
    PairQuad ab, gb;  // the block of A and the Sg^T chunk of the coming step, loaded one step ahead
    PairQuad fb;      // the f^T tile of the row tile under way
    size_t c0;        // first column of the slice
    pair_walk(
        p, w, tl,
        [&](int cb, int xt0) {
            c0 = (size_t)cb * KC;
            an = kap_gather(A, lda, N1, rows, B1, xt0 * T + p.lr0, p.lc);
            ab = pair_load(an, c0), gb = pair_load(gR, c0);
        },
        [&](int xt, bool more) {
            ar = an;
            fb = pair_load(fR, (size_t)xt * T);
            // the rows of the NEXT tile: their indices are requested now and used behind the tile's last chunk (the last
            // tile of the run reads its own first chunk again; that copy is never consumed)
            if (more) an = kap_gather(A, lda, N1, rows, B1, (xt + 1) * T + p.lr0, p.lc);
        },
        [&](int q, int qn, bool last, nsvd_f32x16& ax0, nsvd_f32x16& ax1, nsvd_f32x16& ay) {
            // every wave is done with the previous step's block, Sg^T chunk and f^T tile
            apply_lds_barrier();
            pair_put(ks + so, ab);
            pair_put(gs + so, gb);
            ab = pair_load(last ? an : ar, c0 + qn * KC);
            gb = pair_load(gR, c0 + qn * KC);
            if (q == 0) pair_put(fs + so, fb);
            apply_lds_barrier();
            pair_contract(p, ks, gs, fs, ax0, ax1, ay);
        });
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
    const size_t Bp = isx ? w.B1p : w.B2p, pr = isx ? b : (size_t)g;
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
    return pair_partition(shape_ok(N1, N2, B1, B2, L), true, row_groups, col_groups,
                          [&] { return carve(nullptr, N2, B1, L); });
}

extern "C" int nsvd_kernel_apply_pair(const float* A, size_t lda, int N1, int N2, const long long* rows, int B1,
                                      const long long* cols, int B2, const float* g, const float* f, int L,
                                      float scale_g, float scale_f, float* out_x, float* out_y, void* ws,
                                      size_t ws_bytes, void* stream) {
    if (!A || !rows || !cols || !g || !f || !out_x || !out_y || !ws || !shape_ok(N1, N2, B1, B2, L))
        return NSVD_EINVAL;
    const KapWs w = carve(ws, N2, B1, L);
    // whole 64-float chunks of a row are read: the leading dimension must cover the padded width
    if (lda < (size_t)w.B2p || (lda & 3) != 0 || ((uintptr_t)A & 15) != 0) return NSVD_EINVAL;
    if (!nsvd_ws_ok(ws, ws_bytes, w.bytes)) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)kap_main_kernel}, KAP_LDS_BYTES)) return rc;
    ka_scatter_blocks_kernel<><<<dim3(w.B2p / KS_PB, w.Lp / 64), 256, 0, s>>>(g, cols, B2, L, N2, w.SgT, w.B2p);
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
