// What the two-sided products share (rbf_apply_pair.hip, dot_apply_pair.hip, kernel_apply_pair.hip): both halves of an
// SVD step, "K g" (B1, L) and "K^T f" (B2, L), from ONE pass over the 64 x 64 blocks of kernel values. Here, once: the
// partition rule, the partial copies and their reduce, a thread's tile coordinates, the runs of a workgroup, the
// two-sided contraction, the flush of a wave's tile, the four-row staging of an operand block and the slice walk.
// A file keeps its workspace, how a step obtains its kernel values and stages its operands, and its entry points.
// Everything has internal linkage, as in apply_common.h: each file gets its own.
//
// A workgroup (row group, head tile, column group) owns a run of 64-row x tiles and a run of SLICES of at most
// PAIR_SLICE 64-row y chunks. Per slice it walks its x tiles; per (x tile, chunk) a STEP writes the block of kernel
// values once into LDS, x-row major, and contracts it both ways (pair_contract). The K^T f accumulators of the slice's
// chunks (4 x 16 registers) stay in registers over the whole run of x tiles. K g tiles are flushed per x tile into the
// partial copy of the workgroup's column group (added to what the SAME thread stored for its previous slice: memory
// only this workgroup touches), K^T f tiles once per slice into the partial copy of its row group. The reduce adds the
// copies in group order: no atomics, bit-reproducible, at most PAIR_MAX_GROUPS copies of either output.
#pragma once
#include "apply_common.h"

constexpr int PAIR_SLICE = 4;        // y chunks per slice (K^T f accumulator tiles per wave)
constexpr int PAIR_MAX_GROUPS = 32;  // partial copies of either output
constexpr int PAIR_FILL = 512;       // workgroups wanted: two per CU
constexpr int PAIR_TILE = NSVD_TNT_T * NSVD_TNT_LDT;  // one 64 x 64 LDS tile with padded rows

// ---- host: partition, partial copies, reduce -------------------------------------------------------------------------
// RG row groups of x tiles, CG column groups of slices: split whichever side has more work per group until the grid
// fills the chip or both sides are at one item per group / PAIR_MAX_GROUPS. Restated by tests/_pair_oracle.py:pair_split.
static inline void pair_split(int xtiles, int slices, int ltiles, int* RG, int* CG) {
    int rg = 1, cg = 1;
    const int rmax = xtiles < PAIR_MAX_GROUPS ? xtiles : PAIR_MAX_GROUPS;
    const int cmax = slices < PAIR_MAX_GROUPS ? slices : PAIR_MAX_GROUPS;
    while ((long)ltiles * rg * cg < PAIR_FILL) {
        const bool can_r = 2 * rg <= rmax, can_c = 2 * cg <= cmax;
        if (!can_r && !can_c) break;
        if (can_r && (!can_c || (long)xtiles * cg >= (long)slices * rg)) rg *= 2;
        else cg *= 2;
    }
    *RG = rg;
    *CG = cg;
}

// the tail of every two-sided workspace: the partial copies and the partition they belong to
struct PairParts {
    float* partX;  // (CG, B1p, Lp) partial K g
    float* partY;  // (RG, B2p, Lp) partial K^T f
    int B1p, B2p, Lp, RG, CG;
};

static inline PairParts pair_parts(NsvdArena& a, int B1p, int B2p, int Lp) {
    PairParts q;
    q.B1p = B1p, q.B2p = B2p, q.Lp = Lp;
    pair_split(B1p / NSVD_TNT_T, nsvd_cdiv(B2p / NSVD_TNT_KC, PAIR_SLICE), Lp / NSVD_TNT_T, &q.RG, &q.CG);
    q.partX = a.take((size_t)q.CG * B1p * Lp);
    q.partY = a.take((size_t)q.RG * B2p * Lp);
    return q;
}

// nsvd_*_apply_pair_partition: the shape rules and carve (a callable that measures the workspace) are the file's own
template <class Carve>
static inline int pair_partition(bool shape_ok, bool supported, int* row_groups, int* col_groups, Carve carve) {
    if (!row_groups || !col_groups || !shape_ok) return NSVD_EINVAL;
    if (!supported) return NSVD_EUNSUPPORTED;
    const PairParts w = carve();
    *row_groups = w.RG;
    *col_groups = w.CG;
    return 0;
}

// both outputs in one launch: out_x from the CG copies partX, then out_y from the RG copies partY
// (kernel_apply_pair.hip keeps a reduce of its own: it checks two index arrays and gathers out_y through one, which
// would put four arguments and two branches that the coordinate products never use into this kernel)
template <int = 0>
static __global__ void __launch_bounds__(256)
apply_pair_reduce_kernel(const float* __restrict__ partX, int CG, int B1p, const float* __restrict__ partY, int RG, int B2p,
                         int Lp, int B1, int B2, int L, float scale_g, float scale_f, float* __restrict__ out_x,
                         float* __restrict__ out_y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nx = (size_t)B1 * L, ny = (size_t)B2 * L;
    if (i < nx)
        apply_reduce_one(partX, CG, B1p, Lp, L, i, scale_g, out_x);
    else if (i - nx < ny)
        apply_reduce_one(partY, RG, B2p, Lp, L, i - nx, scale_f, out_y);
}

template <int = 0>
static inline void pair_reduce_launch(const PairParts& w, int B1, int B2, int L, float scale_g, float scale_f,
                                      float* out_x, float* out_y, hipStream_t s) {
    const size_t n = ((size_t)B1 + (size_t)B2) * L;
    apply_pair_reduce_kernel<><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(w.partX, w.CG, w.B1p, w.partY, w.RG, w.B2p, w.Lp,
                                                                          B1, B2, L, scale_g, scale_f, out_x, out_y);
}

// ---- device: a thread's coordinates, a workgroup's runs ---------------------------------------------------------------
// lane, wave; the rows of an MFMA operand this lane reads (ra: wave & 1 half, rb: wave >> 1 half) and its k offset;
// the row (+ 16 i) and column of the float4s it stages of a 64 x 64 block
struct PairLane {
    int lane, wv, ra, rb, kq, lr0, lc;
};

__device__ __forceinline__ PairLane pair_lane(int t) {
    PairLane p;
    p.lane = t & 63;
    p.wv = __builtin_amdgcn_readfirstlane(t >> 6);  // (uniform by construction; tells the compiler so)
    p.ra = (p.wv & 1) * 32 + (p.lane & 31);
    p.rb = (p.wv >> 1) * 32 + (p.lane & 31);
    p.kq = (p.lane >> 5) * 4;
    p.lr0 = t >> 4;
    p.lc = (t & 15) * 4;
    return p;
}

// the x tiles [xt0, xt1) of row group blockIdx.x and the slices [s0, s1) of column group blockIdx.z
struct PairRuns {
    int chunks, xt0, xt1, s0, s1;
};

__device__ __forceinline__ PairRuns pair_runs(int B1p, int B2p, int RG, int CG) {
    const int rg = blockIdx.x, cg = blockIdx.z;
    const int xtiles = B1p / NSVD_TNT_T, chunks = B2p / NSVD_TNT_KC, slices = (chunks + PAIR_SLICE - 1) / PAIR_SLICE;
    PairRuns r;
    r.chunks = chunks;
    r.xt0 = (int)((long)xtiles * rg / RG), r.xt1 = (int)((long)xtiles * (rg + 1) / RG);
    r.s0 = (int)((long)slices * cg / CG), r.s1 = (int)((long)slices * (cg + 1) / CG);
    return r;
}

// ---- device: operand staging -----------------------------------------------------------------------------------------
// what a thread stages of a 64 x 64 operand block: rows (t >> 4) + 16 i, 4 consecutive floats each. pair_load returns
// the record by value: filled through a reference, the compiler leaves one of its float4s in scratch.
struct PairQuad {
    float4 a, b, c, d;
};
struct PairRows {
    const float *a, *b, *c, *d;
};
__device__ __forceinline__ PairRows pair_strided(const float* p, size_t stride16) {
    return {p, p + stride16, p + 2 * stride16, p + 3 * stride16};
}
__device__ __forceinline__ PairQuad pair_load(const PairRows& r, size_t off) {
    PairQuad q;
    q.a = *(const float4*)(r.a + off);
    q.b = *(const float4*)(r.b + off);
    q.c = *(const float4*)(r.c + off);
    q.d = *(const float4*)(r.d + off);
    return q;
}
// (rows given by the first and the distance of 16 rows in floats)
__device__ __forceinline__ PairQuad pair_load(const float* p, size_t stride16) {
    return pair_load(pair_strided(p, stride16), 0);
}
// l: the LDS tile at this thread's (lr0, lc)
__device__ __forceinline__ void pair_put(float* __restrict__ l, const PairQuad& q) {
    *(float4*)(l) = q.a;
    *(float4*)(l + 16 * NSVD_TNT_LDT) = q.b;
    *(float4*)(l + 32 * NSVD_TNT_LDT) = q.c;
    *(float4*)(l + 48 * NSVD_TNT_LDT) = q.d;
}

// ---- device: contraction and flush -----------------------------------------------------------------------------------
// The 32 interleaved MFMAs of a step on its three LDS tiles. ks: kernel values [x row][y row]; gs: g^T chunk [head][y
// row]; fs: f^T tile [head][x row].
//   K g:   rows = x rows (b128 reads along y), columns = heads of g^T;
//   K^T f: rows = y rows (b32 reads down the x rows of the SAME copy, which the compiler pairs into ds_read2_b32: 32
//          consecutive y rows of one x row are 32 consecutive banks), columns = heads of f^T.
// MFMA e of group s contracts k = 8 s + e (lanes 0-31) and 8 s + 4 + e (lanes 32-63).
// K g runs in two chains (ax0 + ax1 is the tile), K^T f in one: the other product's MFMAs run between dependent ones.
// A caller with ONE K g chain passes the same accumulator twice; FIRST then starts that chain here (its value on entry
// is not read: the first MFMA takes an inline zero, no registers).
template <bool FIRST = false>
__device__ __forceinline__ void pair_contract(const PairLane& p, const float* __restrict__ ks,
                                              const float* __restrict__ gs, const float* __restrict__ fs,
                                              nsvd_f32x16& ax0, nsvd_f32x16& ax1, nsvd_f32x16& ay) {
    constexpr int KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;
    const nsvd_f32x16 zero = {0};
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
        ax0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, gv.x, FIRST && s == 0 ? zero : ax0, 0, 0, 0);
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

// ---- device: the slice walk ------------------------------------------------------------------------------------------
// The walk of workgroup (blockIdx.x, head tile tl, blockIdx.z) over its runs. It owns the K^T f chains of a slice's
// chunks, the two K g chains of an x tile and every flush. The file's side of it are three callables (lambdas of its
// main kernel, which keep what is staged in the kernel's own variables):
//   slice(cb, xt0)     a slice begins at chunk cb, its first x tile is xt0: stage what the first step finds staged;
//   tile(xt, more)     x tile xt begins; more: it has a successor in the run;
//   step(q, qn, last, ax0, ax1, ay)   chunk q of the slice against the tile: consume what is staged, stage chunk qn
//                      (operands run one chunk ahead: after the slice's last chunk comes its first again, for the next
//                      x tile; last: this is that last chunk) and contract (pair_contract).
// q, qn and last are constants at each of the four call sites once nc is known, as the unrolled ladder needs: a loop
// over the chunks would index the four K^T f accumulators dynamically.
template <class Slice, class Tile, class Step>
__device__ __forceinline__ void pair_walk(const PairLane& p, const PairParts& w, int tl, Slice slice, Tile tile,
                                          Step step) {
    constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC;
    const PairRuns r = pair_runs(w.B1p, w.B2p, w.RG, w.CG);
    const int col = tl * T + (p.wv >> 1) * 32 + (p.lane & 31), rsub = (p.wv & 1) * 32;
    float* px = w.partX + (size_t)blockIdx.z * w.B1p * w.Lp;
    float* py = w.partY + (size_t)blockIdx.x * w.B2p * w.Lp;
    for (int sl = r.s0; sl < r.s1; ++sl) {
        const int cb = sl * PAIR_SLICE;
        const int nc = min(PAIR_SLICE, r.chunks - cb);
        nsvd_f32x16 ay0 = {0}, ay1 = {0}, ay2 = {0}, ay3 = {0};  // one chain each: the K g MFMAs run between
        slice(cb, r.xt0);
        for (int xt = r.xt0; xt < r.xt1; ++xt) {
            tile(xt, xt + 1 < r.xt1);
            nsvd_f32x16 ax0 = {0}, ax1 = {0};
            step(0, nc > 1 ? 1 : 0, nc == 1, ax0, ax1, ay0);
            if (nc > 1) step(1, nc > 2 ? 2 : 0, nc == 2, ax0, ax1, ay1);
            if (nc > 2) step(2, nc > 3 ? 3 : 0, nc == 3, ax0, ax1, ay2);
            if (nc > 3) step(3, 0, true, ax0, ax1, ay3);
            pair_flush(px, w.Lp, xt * T + rsub, col, p.lane, ax0 + ax1, sl == r.s0);
        }
        const int yrow = cb * KC + rsub;
        pair_flush(py, w.Lp, yrow, col, p.lane, ay0, true);
        if (nc > 1) pair_flush(py, w.Lp, yrow + KC, col, p.lane, ay1, true);
        if (nc > 2) pair_flush(py, w.Lp, yrow + 2 * KC, col, p.lane, ay2, true);
        if (nc > 3) pair_flush(py, w.Lp, yrow + 3 * KC, col, p.lane, ay3, true);
    }
}
