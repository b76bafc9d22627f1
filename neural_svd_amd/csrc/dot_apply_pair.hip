// Two-sided matrix-free dot-product kernel operator on coordinate batches - both halves of a kernel SVD step in one pass:
//     out_x[i][l] = scale_g * sum_j k(x_i, y_j) g[j][l]        (B1, L)   "K g"
//     out_y[j][l] = scale_f * sum_i k(x_i, y_j) f[i][l]        (B2, L)   "K^T f"
// with the kinds and numerical rules of dot_apply.hip (polynomial by multiplication, order-1 arc-cosine with its clamps,
// the deep ReLU NNGP and NTK recursions: apply_poly, apply_arccos1 and apply_relu_deep of apply_common.h).
// Two nsvd_dot_apply calls with swapped arguments form every x_i . y_j twice on the matrix pipe and run the map twice;
// here each kernel value is formed ONCE per 64-head tile and feeds both contractions.
//
// The workgroup, its runs, the partial copies, the reduce and the two-sided contraction are pair_common.h's (the prep
// kernel: apply_common.h): a workgroup (row group, head tile, column group) owns a run of 64-row x tiles and a run of
// slices of at most four 64-row y chunks; per slice it walks its x tiles, the K^T f accumulators of the slice's chunks
// (4 x 16 registers) staying in registers over the run. The kernel values are dot_apply.hip's: per (x tile, chunk) a step
//   1. forms S^T = Y_chunk X_tile^T (64 x 64 x Dp) on v_mfma_f32_32x32x2_f32 from the x tile and the y chunk in LDS
//      (rows of Dp + 4 floats, b128 reads; the x operand is not loop invariant here, so it cannot live in registers);
//   2. applies the map in registers - a lane owns ONE x row (|x_i| read from the tile's norms) and 4 runs of 4
//      consecutive y rows (|y_j| rides with the chunk) - and forces the values of padded x rows AND padded y rows to 0:
//      both now take part in a sum, and coef0^degree need not be finite;
//   3. writes them ONCE into LDS, x-row major (4 ds_write_b128 per lane), with the g^T chunk, the next y chunk and, where
//      due, the f^T tile (first chunk of an x tile) and the next x tile (last chunk), between the step's two LDS-only
//      barriers;
//   4. contracts the copy with the g^T chunk into the K g accumulators (b128 reads) and reads the SAME copy column-wise
//      (32-bit reads) against the f^T tile into the K^T f accumulators (pair_contract).
// g^T runs one chunk ahead in registers; the next y chunk is requested after the map and staged under the barriers, the
// f^T tile and the x tile are requested between them (once per tile). Every buffer is single: LDS is 3 tiles + x tile +
// y chunk = 57.5 KB at D <= 8, 77.5 KB at D = 48 (two workgroups per CU), 85.5 KB at D = 64 (one). 174 / 190 VGPRs, no
// scratch - by three rules the source keeps: staging loads are unconditional, lane offsets of global
// addresses are opaque to the compiler (dpair_opaque), and a chain's first MFMA takes an inline zero. They bind what
// this kernel takes from pair_common.h, and they are why three pieces stay here: the walk (one K g chain that FIRST
// starts), the flush (wave-uniform addresses, one lane offset) and the registers of a coordinate block (named float4s;
// kept in a struct they cost the polynomial kernel two registers).
#include "pair_common.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;

struct DPairWs : PairParts {
    float* xP;  // (B1p, Dp) x coordinates, zero padded
    float* xN;  // (B1p) |x_i| (the deep ReLU kinds: |x_i|^2), 0 for padded rows
    float* yP;  // (B2p, Dp) y coordinates, zero padded
    float* yN;  // (B2p) |y_j| (the deep ReLU kinds: |y_j|^2), 0 for padded rows
    float* gT;  // (Lp, B2p) g transposed, zero padded
    float* fT;  // (Lp, B1p) f transposed, zero padded
    int Dp;
    size_t bytes;
};

DPairWs carve(void* base, int B1, int B2, int D, int L) {
    const ApplyPad pd = apply_pad(B1, B2, D, L, 8);
    DPairWs w;
    w.Dp = pd.Dp;
    NsvdArena a(base);
    w.xP = a.take((size_t)pd.B1p * pd.Dp);
    w.xN = a.take((size_t)pd.B1p);
    w.yP = a.take((size_t)pd.B2p * pd.Dp);
    w.yN = a.take((size_t)pd.B2p);
    w.gT = a.take((size_t)pd.Lp * pd.B2p);
    w.fT = a.take((size_t)pd.Lp * pd.B1p);
    static_cast<PairParts&>(w) = pair_parts(a, pd.B1p, pd.B2p, pd.Lp);
    w.bytes = a.off;
    return w;
}

struct DPairMap {
    float gamma, coef0;
    int degree;
};

// The value, opaque to the compiler: what is computed from it is computed where it is used. Every step of this kernel
// is inlined four times with loop-invariant operands, and the compiler otherwise forms each lane's 64-bit addresses and
// each mask of every variant before the loops and carries them - about 60 vector and 130 scalar registers - through
// all of them, spilling both kinds.
__device__ __forceinline__ unsigned dpair_opaque(unsigned v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ size_t dpair_opaque(size_t v) {
    asm volatile("" : "+v"(v));
    return v;
}

struct DPairLane : PairLane {
    int t, nq, xld, nv;
    int so0, so1, so2, so3;  // LDS offsets of this thread's float4s of a staged (64, Dp) block
    unsigned bo0, bo1, bo2, bo3, bon;  // byte offsets of the same float4s in the workspace block, and of a norm
    size_t go, fo;  // byte offset of this thread's first float4 in a g^T chunk / an f^T tile
    size_t gr, fr;  // floats between the 4 rows it stages
};

// a (64, Dp) block of padded coordinates and its 64 norms, contiguous in the workspace (wave-uniform addresses)
struct DPairBlock {
    const float *c, *n;
};

// ... into a thread's registers: thread t moves the float4s t + 256 i < 16 Dp (named registers: hipcc demotes a float4
// array rewritten inside the loop to scratch, and a struct of them written through a reference likewise)
template <int KIND>
__device__ __forceinline__ void dpair_load(const DPairLane& p, const DPairBlock& blk, float4& b0, float4& b1,
                                           float4& b2, float4& b3, float& nb) {
    // Unconditional: a float4 past the block's end re-reads its last one and is not stored (a load under a condition
    // makes every staging register a value the compiler carries, and spills, between the steps).
    // Addresses are the wave-uniform base plus this lane's byte offset, opaque (dpair_opaque's note).
    const char* s = (const char*)blk.c;
    b0 = *(const float4*)(s + dpair_opaque(p.bo0));
    b1 = *(const float4*)(s + dpair_opaque(p.bo1));
    b2 = *(const float4*)(s + dpair_opaque(p.bo2));
    b3 = *(const float4*)(s + dpair_opaque(p.bo3));
    if (KIND != NSVD_DOT_POLYNOMIAL) nb = *(const float*)((const char*)blk.n + dpair_opaque(p.bon));
}

template <int KIND>
__device__ __forceinline__ void dpair_put(const DPairLane& p, float* __restrict__ dst, const float4& b0,
                                          const float4& b1, const float4& b2, const float4& b3, float nb) {
    if (p.t < p.nv) *(float4*)(dst + p.so0) = b0;
    if (p.t + 256 < p.nv) *(float4*)(dst + p.so1) = b1;
    if (p.t + 512 < p.nv) *(float4*)(dst + p.so2) = b2;
    if (p.t + 768 < p.nv) *(float4*)(dst + p.so3) = b3;
    if (KIND != NSVD_DOT_POLYNOMIAL && p.t < 64) dst[64 * p.xld + p.t] = nb;
}

// this thread's four float4s of a g^T chunk / an f^T tile whose first row starts at `base` (wave-uniform): rows 16
// apart (stride16 floats), the lane's byte offset `off` opaque and added last
__device__ __forceinline__ PairQuad dpair_load_rows(const float* base, size_t stride16, size_t off) {
    const size_t o = dpair_opaque(off);
    PairQuad q;
    q.a = *(const float4*)((const char*)base + o);
    q.b = *(const float4*)((const char*)(base + stride16) + o);
    q.c = *(const float4*)((const char*)(base + 2 * stride16) + o);
    q.d = *(const float4*)((const char*)(base + 3 * stride16) + o);
    return q;
}

// the LDS of a workgroup. ks: kernel chunk [x row][y row]; gs: g^T chunk [head][y row]; fs: f^T tile [head][x row];
// xs, ys: x tile and y chunk, rows of xld floats, then their 64 norms
struct DPairLds {
    float *ks, *gs, *fs, *xs, *ys;
};

// One (x tile, chunk) step. xvalid, yvalid: how many rows of the tile and of the chunk exist (>= 64: all). gb: the g^T
// chunk of THIS step in registers on entry, the one at gnext on exit.
// FIRST: the first chunk of an x tile - the K g accumulator ax starts here (its value on entry is not read) and the
// f^T tile at fc is staged. ynext: the y chunk of the NEXT step, staged here. stage_x (last chunk of an x tile that has
// a successor): stage the x tile xnext. Pointers are wave-uniform.
template <int KIND, bool FIRST>
__device__ __forceinline__ void pair_step(const DPairLane& p, const DPairLds& l, const DPairMap& mp, int xvalid,
                                          int yvalid, PairQuad& gb, const float* __restrict__ gnext,
                                          const DPairBlock& ynext, const float* __restrict__ fc, bool stage_x,
                                          const DPairBlock& xnext, nsvd_f32x16& ax, nsvd_f32x16& ay) {
    float *const ks = l.ks, *const gs = l.gs, *const fs = l.fs, *const xs = l.xs, *const ys = l.ys;
    // S^T: this wave forms y rows jb .. jb + 31 against x rows ib .. ib + 31; jb + (lane & 31) = ra, ib + (lane & 31) = rb
    const int jb = (p.wv & 1) * 32;
    const float* yr = ys + p.ra * p.xld + p.kq;
    const float* xr = xs + p.rb * p.xld + p.kq;
    // (one accumulation chain: the other workgroup of the CU fills the pipe between dependent MFMAs)
    const nsvd_f32x16 zero = {0};  // (as the C operand of a chain's first MFMA: an inline constant, no registers)
    nsvd_f32x16 sv;
    {
        const float4 yv = *(const float4*)yr, xv = *(const float4*)xr;
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.x, xv.x, zero, 0, 0, 0);
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.y, xv.y, sv, 0, 0, 0);
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.z, xv.z, sv, 0, 0, 0);
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.w, xv.w, sv, 0, 0, 0);
    }
    for (int s = 1; s < p.nq; ++s) {
        const float4 yv = *(const float4*)(yr + s * 8), xv = *(const float4*)(xr + s * 8);
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.x, xv.x, sv, 0, 0, 0);
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.y, xv.y, sv, 0, 0, 0);
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.z, xv.z, sv, 0, 0, 0);
        sv = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.w, xv.w, sv, 0, 0, 0);
    }
    // sv[r] = x_i . y_j, i = rb, j = jb + 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
    float kv[16];
    if (KIND == NSVD_DOT_POLYNOMIAL) {
        const nsvd_f32x16 pw = apply_poly(sv, mp.gamma, mp.coef0, mp.degree);
#pragma unroll
        for (int r = 0; r < 16; ++r) kv[r] = pw[r];
    } else if (apply_is_relu(KIND)) {
        const float nx2 = xs[64 * p.xld + p.rb];  // (these kinds stage the SQUARED norms: the prep call's `rooted`)
        float ny2[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 ny = *(const float4*)(ys + 64 * p.xld + jb + 8 * g + p.kq);
            ny2[4 * g] = ny.x, ny2[4 * g + 1] = ny.y, ny2[4 * g + 2] = ny.z, ny2[4 * g + 3] = ny.w;
        }
        apply_relu_deep<KIND == NSVD_DOT_RELU_NTK>(sv, nx2, ny2, mp.gamma, mp.coef0, mp.degree, kv);
    } else {
        const float nx = xs[64 * p.xld + p.rb];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 ny = *(const float4*)(ys + 64 * p.xld + jb + 8 * g + p.kq);
            kv[4 * g] = apply_arccos1(sv[4 * g], nx, ny.x);
            kv[4 * g + 1] = apply_arccos1(sv[4 * g + 1], nx, ny.y);
            kv[4 * g + 2] = apply_arccos1(sv[4 * g + 2], nx, ny.z);
            kv[4 * g + 3] = apply_arccos1(sv[4 * g + 3], nx, ny.w);
        }
    }
    if (xvalid < T || yvalid < KC) {
        // padded rows of EITHER side: f^T and g^T are 0 there, but k (coef0^degree of a huge coef0) need not be finite
        // (the deep ReLU kinds: coef0-derived values there)
        const bool xpad = p.rb >= xvalid;
        // (rows left from this lane's first y row on, against constants: the 16 row numbers themselves are loop invariant,
        // and the compiler would carry them in 16 registers through the whole kernel)
        const int left = yvalid - (int)dpair_opaque((unsigned)(jb + p.kq));
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (xpad || 8 * (r >> 2) + (r & 3) >= left) kv[r] = 0.f;
    }
    // the next step's y chunk, requested once the map's registers are free; it lands under the barrier and the other
    // LDS writes
    float4 yb0, yb1, yb2, yb3;  // (no initial value: dpair_put reads exactly what dpair_load wrote)
    float ynb;
    dpair_load<KIND>(p, ynext, yb0, yb1, yb2, yb3, ynb);
    // every wave is done with the previous step's kernel chunk, g^T chunk and f^T tile, and with this step's x tile and
    // y chunk
    apply_lds_barrier();
    float* la = ks + p.rb * LDT + jb + p.kq;
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *(float4*)(la + 8 * g) = make_float4(kv[4 * g], kv[4 * g + 1], kv[4 * g + 2], kv[4 * g + 3]);
    const int so = p.lr0 * LDT + p.lc;
    pair_put(gs + so, gb);
    gb = dpair_load_rows(gnext, p.gr, p.go);
    dpair_put<KIND>(p, ys, yb0, yb1, yb2, yb3, ynb);
    if (FIRST) pair_put(fs + so, dpair_load_rows(fc, p.fr, p.fo));  // (requested here, once per x tile, not a step ahead)
    if (stage_x) {
        float4 x0, x1, x2, x3;
        float xn;
        dpair_load<KIND>(p, xnext, x0, x1, x2, x3, xn);
        dpair_put<KIND>(p, xs, x0, x1, x2, x3, xn);
    }
    apply_lds_barrier();
    // (one K g chain: the K^T f MFMAs run between, and the other workgroup of the CU fills the rest. ax is passed as
    // BOTH K g accumulators on purpose: the two references name one object, which makes pair_contract's two chains one)
    pair_contract<FIRST>(p, ks, gs, fs, ax, ax, ay);
}

// store (first == true) or add-and-store the wave's 32 x 32 tile whose first element is at `tile` (wave-uniform) in a
// (rows, Lp) partial copy; po: this lane's offset in the tile's first row group, (lane >> 5) * 4 * Lp + (lane & 31)
__device__ __forceinline__ void dpair_flush(float* __restrict__ tile, size_t Lp, size_t po, const nsvd_f32x16& acc,
                                            bool first) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float* q = (tile + (size_t)((r >> 2) * 8 + (r & 3)) * Lp) + po;
        *q = first ? acc[r] : *q + acc[r];
    }
}

// grid (RG, Lp / 64, CG). LDS: kernel chunk | g^T chunk | f^T tile (PAIR_TILE floats each) | x tile | y chunk
// ((64, Dp + 4) + 64 norms each).
// The walk is pair_walk's, written out: here the K g chain is ONE, started by the inline zero of the tile's first step
// (FIRST is a template argument, and a zeroed second chain would be added to the tile: 16 more registers and a sum
// that turns -0 into +0), and the flushes go through wave-uniform addresses with one opaque lane offset.
template <int KIND>
__global__ void __launch_bounds__(256, 2) dot_pair_main_kernel(int B1, int B2, DPairWs w, DPairMap mp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Dp = w.Dp;
    DPairLane p;
    p.t = threadIdx.x;
    static_cast<PairLane&>(p) = pair_lane(p.t);
    p.nq = Dp >> 3;
    p.xld = Dp + 4;
    p.nv = 16 * Dp;
    const int Dq = Dp >> 2;
    p.so0 = (p.t / Dq) * p.xld + (p.t % Dq) * 4;
    p.so1 = ((p.t + 256) / Dq) * p.xld + ((p.t + 256) % Dq) * 4;
    p.so2 = ((p.t + 512) / Dq) * p.xld + ((p.t + 512) % Dq) * 4;
    p.so3 = ((p.t + 768) / Dq) * p.xld + ((p.t + 768) % Dq) * 4;
    const int cblk = 64 * p.xld + 64;  // a staged coordinate block and its norms
    const DPairLds l = {lds, lds + PAIR_TILE, lds + 2 * PAIR_TILE, lds + 3 * PAIR_TILE, lds + 3 * PAIR_TILE + cblk};
    const int rg = blockIdx.x, tl = blockIdx.y, cg = blockIdx.z;
    const PairRuns r = pair_runs(w.B1p, w.B2p, w.RG, w.CG);
    {
        const unsigned last = (unsigned)p.nv - 1u, u = (unsigned)p.t;
        p.bo0 = 16u * min(u, last);
        p.bo1 = 16u * min(u + 256u, last);
        p.bo2 = 16u * min(u + 512u, last);
        p.bo3 = 16u * min(u + 768u, last);
        p.bon = 4u * (u & 63u);
    }
    p.go = 4 * ((size_t)p.lr0 * w.B2p + p.lc);
    p.gr = (size_t)16 * w.B2p;
    p.fo = 4 * ((size_t)p.lr0 * w.B1p + p.lc);
    p.fr = (size_t)16 * w.B1p;
    const float* gp = w.gT + (size_t)tl * T * w.B2p;  // wave-uniform: the head tile's first row
    const float* fp = w.fT + (size_t)tl * T * w.B1p;
    // the wave's tiles in the partial copies of this workgroup: wave-uniform addresses, one lane offset
    const size_t Lp = (size_t)w.Lp, po = (size_t)((p.lane >> 5) * 4) * Lp + (size_t)(p.lane & 31);
    const int col0 = tl * T + (p.wv >> 1) * 32, rsub = (p.wv & 1) * 32;
    float* px = w.partX + ((size_t)cg * w.B1p + rsub) * Lp + col0;
    float* py = w.partY + ((size_t)rg * w.B2p + rsub) * Lp + col0;
    const size_t cstep = (size_t)KC * Dp;  // floats of one padded (64, Dp) coordinate block
    // x tile b: its padded coordinates and norms
    const auto xblock = [&](int b) { return DPairBlock{w.xP + (size_t)b * cstep, w.xN + (size_t)b * T}; };
    for (int sl = r.s0; sl < r.s1; ++sl) {
        const int cb = sl * PAIR_SLICE;
        const int nc = min(PAIR_SLICE, r.chunks - cb);
        // chunk q of the slice: its padded coordinates and norms
        const DPairBlock y0 = {w.yP + (size_t)cb * cstep, w.yN + (size_t)cb * KC};
        const auto ychunk = [&](int q) { return DPairBlock{y0.c + q * cstep, y0.n + q * KC}; };
        // chunk q of the slice is followed by chunk (q + 1) % nc: the walk starts over for the next x tile
        const int q1 = 1 % nc, q2 = 2 % nc, q3 = 3 % nc, q4 = 4 % nc;
        // the first x tile of the run and the first y chunk (the steps below stage every later one between their barriers)
        __syncthreads();
        {
            float4 b0, b1, b2, b3;
            float nb;
            dpair_load<KIND>(p, xblock(r.xt0), b0, b1, b2, b3, nb);
            dpair_put<KIND>(p, l.xs, b0, b1, b2, b3, nb);
            dpair_load<KIND>(p, y0, b0, b1, b2, b3, nb);
            dpair_put<KIND>(p, l.ys, b0, b1, b2, b3, nb);
        }
        __syncthreads();
        nsvd_f32x16 ay0 = {0}, ay1 = {0}, ay2 = {0}, ay3 = {0};  // one chain each: the K g MFMAs run between
        const float* gc = gp + (size_t)cb * KC;
        PairQuad gb = dpair_load_rows(gc, p.gr, p.go);
        for (int xt = r.xt0; xt < r.xt1; ++xt) {
            const float* fc = fp + (size_t)xt * T;
            nsvd_f32x16 ax;  // one chain (the K^T f MFMAs run between), started by the tile's first step
            const bool more = xt + 1 < r.xt1;
            const DPairBlock xn = xblock(xt + 1);  // (read only where `more`)
            const int xv = B1 - xt * T, yv = B2 - cb * KC;
            // step q consumes chunk q (in LDS) and stages chunk (q + 1) % nc of y and of g^T
            pair_step<KIND, true>(p, l, mp, xv, yv, gb, gc + q1 * KC, ychunk(q1), fc, more && nc == 1, xn, ax, ay0);
            if (nc > 1)
                pair_step<KIND, false>(p, l, mp, xv, yv - KC, gb, gc + q2 * KC, ychunk(q2), fc, more && nc == 2, xn,
                                       ax, ay1);
            if (nc > 2)
                pair_step<KIND, false>(p, l, mp, xv, yv - 2 * KC, gb, gc + q3 * KC, ychunk(q3), fc, more && nc == 3,
                                       xn, ax, ay2);
            if (nc > 3)
                pair_step<KIND, false>(p, l, mp, xv, yv - 3 * KC, gb, gc + q4 * KC, ychunk(q4), fc, more, xn, ax,
                                       ay3);
            dpair_flush(px + (size_t)xt * T * Lp, Lp, po, ax, sl == r.s0);
        }
        float* pyc = py + (size_t)cb * KC * Lp;
        dpair_flush(pyc, Lp, po, ay0, true);
        if (nc > 1) dpair_flush(pyc + (size_t)KC * Lp, Lp, po, ay1, true);
        if (nc > 2) dpair_flush(pyc + (size_t)2 * KC * Lp, Lp, po, ay2, true);
        if (nc > 3) dpair_flush(pyc + (size_t)3 * KC * Lp, Lp, po, ay3, true);
    }
}

size_t dpair_lds_bytes(int Dp) { return (size_t)(3 * PAIR_TILE + 2 * (64 * (Dp + 4) + 64)) * sizeof(float); }

}  // namespace

extern "C" size_t nsvd_dot_apply_pair_workspace_bytes(int B1, int B2, int D, int L) {
    if (!apply_shape_ok(B1, B2, D, L) || D > APPLY_MAX_D) return 0;
    return carve(nullptr, B1, B2, D, L).bytes;
}

extern "C" int nsvd_dot_apply_pair_partition(int B1, int B2, int D, int L, int* row_groups, int* col_slices) {
    return pair_partition(apply_shape_ok(B1, B2, D, L), D <= APPLY_MAX_D, row_groups, col_slices,
                          [&] { return carve(nullptr, B1, B2, D, L); });
}

extern "C" int nsvd_dot_apply_pair(const float* x, int B1, const float* y, int B2, int D, const float* g, const float* f,
                                   int L, int kind, float gamma, float coef0, int degree, float scale_g, float scale_f,
                                   float* out_x, float* out_y, void* ws, size_t ws_bytes, void* stream) {
    if (!apply_args_ok({x, y, g, f, out_x, out_y, ws}, B1, B2, D, L)) return NSVD_EINVAL;
    if (!apply_dot_kind_ok(kind, gamma, coef0, degree)) return NSVD_EINVAL;
    const size_t nox = (size_t)B1 * L, noy = (size_t)B2 * L;
    if (apply_overlap(out_x, nox, out_y, noy)) return NSVD_EINVAL;
    for (float* o : {out_x, out_y}) {  // the outputs alias nothing
        const size_t no = o == out_x ? nox : noy;
        if (apply_overlap(o, no, x, (size_t)B1 * D) || apply_overlap(o, no, y, (size_t)B2 * D) ||
            apply_overlap(o, no, g, noy) || apply_overlap(o, no, f, nox))
            return NSVD_EINVAL;
    }
    if (D > APPLY_MAX_D) return NSVD_EUNSUPPORTED;
    const DPairWs w = carve(ws, B1, B2, D, L);
    if (!nsvd_ws_ok(ws, ws_bytes, w.bytes)) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ApplyPrep pr = {};
    pr.s[0] = {y, w.yP, w.yN, g, w.gT, B2, w.B2p};
    pr.s[1] = {x, w.xP, w.xN, f, w.fT, B1, w.B1p};
    pr.D = D, pr.Dp = w.Dp, pr.L = L, pr.Lp = w.Lp, pr.rooted = apply_is_relu(kind) ? 0 : 1;  // (|.|; the deep ReLU kinds: |.|^2)
    apply_prep_launch(pr, s);
    NSVD_CHECK_LAUNCH();
    static NsvdLdsOptIn lds_opt_in;
    if (const int rc = nsvd_lds_opt_in(lds_opt_in, {(const void*)dot_pair_main_kernel<NSVD_DOT_POLYNOMIAL>,
                                                    (const void*)dot_pair_main_kernel<NSVD_DOT_ARCCOS1>,
                                                    (const void*)dot_pair_main_kernel<NSVD_DOT_RELU_NNGP>,
                                                    (const void*)dot_pair_main_kernel<NSVD_DOT_RELU_NTK>},
                                                   dpair_lds_bytes(APPLY_MAX_D)))
        return rc;
    const dim3 grid(w.RG, w.Lp / T, w.CG);
    const DPairMap mp = {gamma, coef0, degree};
    nsvd_prof_begin(s);
    if (kind == NSVD_DOT_POLYNOMIAL)
        dot_pair_main_kernel<NSVD_DOT_POLYNOMIAL><<<grid, 256, dpair_lds_bytes(w.Dp), s>>>(B1, B2, w, mp);
    else if (kind == NSVD_DOT_ARCCOS1)
        dot_pair_main_kernel<NSVD_DOT_ARCCOS1><<<grid, 256, dpair_lds_bytes(w.Dp), s>>>(B1, B2, w, mp);
    else if (kind == NSVD_DOT_RELU_NNGP)
        dot_pair_main_kernel<NSVD_DOT_RELU_NNGP><<<grid, 256, dpair_lds_bytes(w.Dp), s>>>(B1, B2, w, mp);
    else
        dot_pair_main_kernel<NSVD_DOT_RELU_NTK><<<grid, 256, dpair_lds_bytes(w.Dp), s>>>(B1, B2, w, mp);
    nsvd_prof_end(s);
    NSVD_CHECK_LAUNCH();
    pair_reduce_launch(w, B1, B2, L, scale_g, scale_f, out_x, out_y, s);
    NSVD_CHECK_LAUNCH();
    return 0;
}
