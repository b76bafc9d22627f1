// Two-sided matrix-free dot-product kernel operator on coordinate batches - both halves of a kernel SVD step in one pass:
//     out_x[i][l] = scale_g * sum_j k(x_i, y_j) g[j][l]        (B1, L)   "K g"
//     out_y[j][l] = scale_f * sum_i k(x_i, y_j) f[i][l]        (B2, L)   "K^T f"
// with the kinds and numerical rules of dot_apply.hip (polynomial by multiplication, order-1 arc-cosine with its clamps,
// the deep ReLU NNGP and NTK recursions: apply_poly, apply_arccos1 and apply_relu_deep of apply_common.h).
// Two nsvd_dot_apply calls with swapped arguments form every x_i . y_j twice on the matrix pipe and run the map twice;
// here each kernel value is formed ONCE per 64-head tile and feeds both contractions.
//
// The workgroup, its runs and the partial copies are rbf_apply_pair.hip's (prep and reduce kernels: apply_common.h): a workgroup (row group,
// head tile, column group) owns a run of 64-row x tiles and a run of slices of at most four 64-row y chunks; per slice
// it walks its x tiles, the K^T f accumulators of the slice's chunks (4 x 16 registers) staying in registers over the
// run. The kernel values are dot_apply.hip's: per (x tile, chunk) a step
//   1. forms S^T = Y_chunk X_tile^T (64 x 64 x Dp) on v_mfma_f32_32x32x2_f32 from the x tile and the y chunk in LDS
//      (rows of Dp + 4 floats, b128 reads; the x operand is not loop invariant here, so it cannot live in registers);
//   2. applies the map in registers - a lane owns ONE x row (|x_i| read from the tile's norms) and 4 runs of 4
//      consecutive y rows (|y_j| rides with the chunk) - and forces the values of padded x rows AND padded y rows to 0:
//      both now take part in a sum, and coef0^degree need not be finite;
//   3. writes them ONCE into LDS, x-row major (4 ds_write_b128 per lane), with the g^T chunk, the next y chunk and, where
//      due, the f^T tile (first chunk of an x tile) and the next x tile (last chunk), between the step's two LDS-only
//      barriers;
//   4. contracts the copy with the g^T chunk into the K g accumulators (b128 reads) and reads the SAME copy column-wise
//      (32-bit reads) against the f^T tile into the K^T f accumulators, as rbf_apply_pair.hip does.
// g^T runs one chunk ahead in registers; the next y chunk is requested after the map and staged under the barriers, the
// f^T tile and the x tile are requested between them (once per tile). Every buffer is single: LDS is 3 tiles + x tile +
// y chunk = 57.5 KB at D <= 8, 77.5 KB at D = 48 (two workgroups per CU), 85.5 KB at D = 64 (one). 174 / 191 VGPRs, no
// scratch - by three rules the source keeps: staging loads are unconditional, lane offsets of global
// addresses are opaque to the compiler (dpair_opaque), and a chain's first MFMA takes an inline zero.
#include "apply_common.h"
#include "pair_split.h"

namespace {

constexpr int T = NSVD_TNT_T, KC = NSVD_TNT_KC, LDT = NSVD_TNT_LDT;
constexpr int DPAIR_TILE = T * LDT;   // one 64 x 64 LDS tile with padded rows

struct DPairWs {
    float* xP;     // (B1p, Dp) x coordinates, zero padded
    float* xN;     // (B1p) |x_i| (the deep ReLU kinds: |x_i|^2), 0 for padded rows
    float* yP;     // (B2p, Dp) y coordinates, zero padded
    float* yN;     // (B2p) |y_j| (the deep ReLU kinds: |y_j|^2), 0 for padded rows
    float* gT;     // (Lp, B2p) g transposed, zero padded
    float* fT;     // (Lp, B1p) f transposed, zero padded
    float* partX;  // (CG, B1p, Lp) partial K g
    float* partY;  // (RG, B2p, Lp) partial K^T f
    int B1p, B2p, Dp, Lp, RG, CG;
    size_t bytes;
};

DPairWs carve(void* base, int B1, int B2, int D, int L) {
    const ApplyPad pd = apply_pad(B1, B2, D, L, 8);
    DPairWs w;
    w.B1p = pd.B1p, w.B2p = pd.B2p, w.Dp = pd.Dp, w.Lp = pd.Lp;
    pair_split(w.B1p / T, nsvd_cdiv(w.B2p / KC, PAIR_SLICE), w.Lp / T, &w.RG, &w.CG);
    NsvdArena a(base);
    w.xP = a.take((size_t)w.B1p * w.Dp);
    w.xN = a.take((size_t)w.B1p);
    w.yP = a.take((size_t)w.B2p * w.Dp);
    w.yN = a.take((size_t)w.B2p);
    w.gT = a.take((size_t)w.Lp * w.B2p);
    w.fT = a.take((size_t)w.Lp * w.B1p);
    w.partX = a.take((size_t)w.CG * w.B1p * w.Lp);
    w.partY = a.take((size_t)w.RG * w.B2p * w.Lp);
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

struct DPairLane {
    int t, lane, wv, ra, rb, kq, lr0, lc, nq, xld, nv;
    int so0, so1, so2, so3;  // LDS offsets of this thread's float4s of a staged (64, Dp) block
    unsigned bo0, bo1, bo2, bo3, bon;  // byte offsets of the same float4s in the workspace block, and of a norm
    size_t go, fo;  // byte offset of this thread's first float4 in a g^T chunk / an f^T tile
    size_t gr, fr;  // floats between the 4 rows it stages
};

// a (64, Dp) block of padded coordinates (contiguous in the workspace, wave-uniform address) and its 64 norms: thread t
// moves the float4s t + 256 i < 16 Dp (named registers: hipcc demotes a float4 array rewritten inside the loop to scratch)
template <int KIND>
__device__ __forceinline__ void dpair_load(const DPairLane& p, const float* __restrict__ blk,
                                           const float* __restrict__ nrm, float4& b0, float4& b1, float4& b2,
                                           float4& b3, float& nb) {
    // Unconditional: a float4 past the block's end re-reads its last one and is not stored (a load under a condition
    // makes every staging register a value the compiler carries, and spills, between the steps).
    // Addresses are the wave-uniform base plus this lane's byte offset, opaque (dpair_opaque's note).
    const char* s = (const char*)blk;
    b0 = *(const float4*)(s + dpair_opaque(p.bo0));
    b1 = *(const float4*)(s + dpair_opaque(p.bo1));
    b2 = *(const float4*)(s + dpair_opaque(p.bo2));
    b3 = *(const float4*)(s + dpair_opaque(p.bo3));
    if (KIND != NSVD_DOT_POLYNOMIAL) nb = *(const float*)((const char*)nrm + dpair_opaque(p.bon));
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

// One (x tile, chunk) step. ks: kernel chunk [x row][y row]; gs: g^T chunk [head][y row]; fs: f^T tile [head][x row];
// xs, ys: x tile and y chunk, rows of xld floats, then their 64 norms. xvalid, yvalid: how many rows of the tile and of
// the chunk exist (>= 64: all). gb*: the g^T chunk of THIS step in registers on entry, the one at gnext on exit.
// FIRST: the first chunk of an x tile - the K g accumulator ax starts here (its value on entry is not read) and the
// f^T tile at fc is staged. (ynext, ynnext): the y chunk of the NEXT step and its norms, staged here. stage_x (last
// chunk of an x tile that has a successor): stage the x tile at (xnext, xnnext). Pointers are wave-uniform.
template <int KIND, bool FIRST>
__device__ __forceinline__ void dpair_step(const DPairLane& p, float* __restrict__ ks, float* __restrict__ gs,
                                           float* __restrict__ fs, float* __restrict__ xs, float* __restrict__ ys,
                                           const DPairMap& mp, int xvalid, int yvalid, float4& gb0, float4& gb1,
                                           float4& gb2, float4& gb3, const float* __restrict__ gnext,
                                           const float* __restrict__ ynext, const float* __restrict__ ynnext,
                                           const float* __restrict__ fc, bool stage_x, const float* __restrict__ xnext,
                                           const float* __restrict__ xnnext, nsvd_f32x16& ax, nsvd_f32x16& ay) {
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
    dpair_load<KIND>(p, ynext, ynnext, yb0, yb1, yb2, yb3, ynb);
    // every wave is done with the previous step's kernel chunk, g^T chunk and f^T tile, and with this step's x tile and
    // y chunk
    apply_lds_barrier();
    float* la = ks + p.rb * LDT + jb + p.kq;
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *(float4*)(la + 8 * g) = make_float4(kv[4 * g], kv[4 * g + 1], kv[4 * g + 2], kv[4 * g + 3]);
    float* lb = gs + p.lr0 * LDT + p.lc;
    *(float4*)(lb) = gb0;
    *(float4*)(lb + 16 * LDT) = gb1;
    *(float4*)(lb + 32 * LDT) = gb2;
    *(float4*)(lb + 48 * LDT) = gb3;
    const size_t go = dpair_opaque(p.go);
    gb0 = *(const float4*)((const char*)gnext + go);
    gb1 = *(const float4*)((const char*)(gnext + p.gr) + go);
    gb2 = *(const float4*)((const char*)(gnext + 2 * p.gr) + go);
    gb3 = *(const float4*)((const char*)(gnext + 3 * p.gr) + go);
    dpair_put<KIND>(p, ys, yb0, yb1, yb2, yb3, ynb);
    if (FIRST) {
        // (requested here, once per x tile, not a step ahead)
        const size_t fo = dpair_opaque(p.fo);
        const float4 fb0 = *(const float4*)((const char*)fc + fo), fb1 = *(const float4*)((const char*)(fc + p.fr) + fo),
                     fb2 = *(const float4*)((const char*)(fc + 2 * p.fr) + fo),
                     fb3 = *(const float4*)((const char*)(fc + 3 * p.fr) + fo);
        float* lf = fs + p.lr0 * LDT + p.lc;
        *(float4*)(lf) = fb0;
        *(float4*)(lf + 16 * LDT) = fb1;
        *(float4*)(lf + 32 * LDT) = fb2;
        *(float4*)(lf + 48 * LDT) = fb3;
    }
    if (stage_x) {
        float4 x0, x1, x2, x3;
        float xn;
        dpair_load<KIND>(p, xnext, xnnext, x0, x1, x2, x3, xn);
        dpair_put<KIND>(p, xs, x0, x1, x2, x3, xn);
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
        ax = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, gv.x, FIRST && s == 0 ? zero : ax, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t0, fv.x, ay, 0, 0, 0);
        ax = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, gv.y, ax, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t1, fv.y, ay, 0, 0, 0);
        ax = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, gv.z, ax, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t2, fv.z, ay, 0, 0, 0);
        ax = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, gv.w, ax, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f32_32x32x2f32(t3, fv.w, ay, 0, 0, 0);
    }
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

// grid (RG, Lp / 64, CG). LDS: kernel chunk | g^T chunk | f^T tile (DPAIR_TILE floats each) | x tile | y chunk
// ((64, Dp + 4) + 64 norms each).
template <int KIND>
__global__ void __launch_bounds__(256, 2) dot_pair_main_kernel(int B1, int B2, DPairWs w, DPairMap mp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Dp = w.Dp;
    DPairLane p;
    p.t = threadIdx.x;
    p.lane = p.t & 63;
    p.wv = __builtin_amdgcn_readfirstlane(p.t >> 6);  // (uniform by construction; tells the compiler so)
    p.ra = (p.wv & 1) * 32 + (p.lane & 31);
    p.rb = (p.wv >> 1) * 32 + (p.lane & 31);
    p.kq = (p.lane >> 5) * 4;
    p.lr0 = p.t >> 4;
    p.lc = (p.t & 15) * 4;
    p.nq = Dp >> 3;
    p.xld = Dp + 4;
    p.nv = 16 * Dp;
    const int Dq = Dp >> 2;
    p.so0 = (p.t / Dq) * p.xld + (p.t % Dq) * 4;
    p.so1 = ((p.t + 256) / Dq) * p.xld + ((p.t + 256) % Dq) * 4;
    p.so2 = ((p.t + 512) / Dq) * p.xld + ((p.t + 512) % Dq) * 4;
    p.so3 = ((p.t + 768) / Dq) * p.xld + ((p.t + 768) % Dq) * 4;
    const int cblk = 64 * p.xld + 64;  // a staged coordinate block and its norms
    float *ks = lds, *gs = lds + DPAIR_TILE, *fs = lds + 2 * DPAIR_TILE, *xs = lds + 3 * DPAIR_TILE, *ys = xs + cblk;
    const int rg = blockIdx.x, tl = blockIdx.y, cg = blockIdx.z;
    const int xtiles = w.B1p / T, chunks = w.B2p / KC, slices = (chunks + PAIR_SLICE - 1) / PAIR_SLICE;
    const int xt0 = (int)((long)xtiles * rg / w.RG), xt1 = (int)((long)xtiles * (rg + 1) / w.RG);
    const int sl0 = (int)((long)slices * cg / w.CG), sl1 = (int)((long)slices * (cg + 1) / w.CG);
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
    for (int sl = sl0; sl < sl1; ++sl) {
        const int cb = sl * PAIR_SLICE;
        const int nc = min(PAIR_SLICE, chunks - cb);
        const float* yc = w.yP + (size_t)cb * cstep;  // the slice's chunks: coordinates, norms
        const float* ync = w.yN + (size_t)cb * KC;
        // chunk q of the slice is followed by chunk (q + 1) % nc: the walk starts over for the next x tile
        const int q1 = 1 % nc, q2 = 2 % nc, q3 = 3 % nc, q4 = 4 % nc;
        // the first x tile of the run and the first y chunk (the steps below stage every later one between their barriers)
        __syncthreads();
        {
            float4 b0, b1, b2, b3;
            float nb;
            dpair_load<KIND>(p, w.xP + (size_t)xt0 * cstep, w.xN + (size_t)xt0 * T, b0, b1, b2, b3, nb);
            dpair_put<KIND>(p, xs, b0, b1, b2, b3, nb);
            dpair_load<KIND>(p, yc, ync, b0, b1, b2, b3, nb);
            dpair_put<KIND>(p, ys, b0, b1, b2, b3, nb);
        }
        __syncthreads();
        nsvd_f32x16 ay0 = {0}, ay1 = {0}, ay2 = {0}, ay3 = {0};  // one chain each: the K g MFMAs run between
        const float* gc = gp + (size_t)cb * KC;
        const size_t go = dpair_opaque(p.go);
        float4 gb0 = *(const float4*)((const char*)gc + go), gb1 = *(const float4*)((const char*)(gc + p.gr) + go),
               gb2 = *(const float4*)((const char*)(gc + 2 * p.gr) + go),
               gb3 = *(const float4*)((const char*)(gc + 3 * p.gr) + go);
        for (int xt = xt0; xt < xt1; ++xt) {
            const float* fc = fp + (size_t)xt * T;
            nsvd_f32x16 ax;  // one chain (the K^T f MFMAs run between), started by the tile's first step
            const bool more = xt + 1 < xt1;
            const float* xn = w.xP + (size_t)(xt + 1) * cstep;  // (read only where `more`)
            const float* xnn = w.xN + (size_t)(xt + 1) * T;
            const int xv = B1 - xt * T, yv = B2 - cb * KC;
            // step q consumes chunk q (in LDS) and stages chunk (q + 1) % nc of y and of g^T
            dpair_step<KIND, true>(p, ks, gs, fs, xs, ys, mp, xv, yv, gb0, gb1, gb2, gb3, gc + q1 * KC, yc + q1 * cstep,
                             ync + q1 * KC, fc, more && nc == 1, xn, xnn, ax, ay0);
            if (nc > 1)
                dpair_step<KIND, false>(p, ks, gs, fs, xs, ys, mp, xv, yv - KC, gb0, gb1, gb2, gb3, gc + q2 * KC,
                                 yc + q2 * cstep, ync + q2 * KC, fc, more && nc == 2, xn, xnn, ax, ay1);
            if (nc > 2)
                dpair_step<KIND, false>(p, ks, gs, fs, xs, ys, mp, xv, yv - 2 * KC, gb0, gb1, gb2, gb3, gc + q3 * KC,
                                 yc + q3 * cstep, ync + q3 * KC, fc, more && nc == 3, xn, xnn, ax, ay2);
            if (nc > 3)
                dpair_step<KIND, false>(p, ks, gs, fs, xs, ys, mp, xv, yv - 3 * KC, gb0, gb1, gb2, gb3, gc + q4 * KC,
                                 yc + q4 * cstep, ync + q4 * KC, fc, more, xn, xnn, ax, ay3);
            dpair_flush(px + (size_t)xt * T * Lp, Lp, po, ax, sl == sl0);
        }
        float* pyc = py + (size_t)cb * KC * Lp;
        dpair_flush(pyc, Lp, po, ay0, true);
        if (nc > 1) dpair_flush(pyc + (size_t)KC * Lp, Lp, po, ay1, true);
        if (nc > 2) dpair_flush(pyc + (size_t)2 * KC * Lp, Lp, po, ay2, true);
        if (nc > 3) dpair_flush(pyc + (size_t)3 * KC * Lp, Lp, po, ay3, true);
    }
}

size_t dpair_lds_bytes(int Dp) { return (size_t)(3 * DPAIR_TILE + 2 * (64 * (Dp + 4) + 64)) * sizeof(float); }

}  // namespace

extern "C" size_t nsvd_dot_apply_pair_workspace_bytes(int B1, int B2, int D, int L) {
    if (!apply_shape_ok(B1, B2, D, L) || D > APPLY_MAX_D) return 0;
    return carve(nullptr, B1, B2, D, L).bytes;
}

extern "C" int nsvd_dot_apply_pair_partition(int B1, int B2, int D, int L, int* row_groups, int* col_slices) {
    return apply_pair_partition(carve, B1, B2, D, L, row_groups, col_slices);
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
    const size_t n = (size_t)(B1 + (size_t)B2) * L;
    apply_pair_reduce_kernel<><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(
        w.partX, w.CG, w.B1p, w.partY, w.RG, w.B2p, w.Lp, B1, B2, L, scale_g, scale_f, out_x, out_y);
    NSVD_CHECK_LAUNCH();
    return 0;
}
