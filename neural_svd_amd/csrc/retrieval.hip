// Exact retrieval metrics for the CDK towers (examples/cdk/sketchy/retrieve.py): for every query the whole gallery
// ranked by descending key, ties by ascending gallery index; top-K indices and relevances, P@K, the three average
// precisions over the WHOLE ranking. DESIGN.md 3.11 has the choice and its cost model; in short, per query chunk:
//   1. retr_half_sqnorm_kernel (Euclidean only, once per call): |y_j|^2 / 2.
//   2. retr_score_kernel: keys s_ij = x_i . y_j [- |y_j|^2 / 2] on the fp32-input MFMA (64 x 128 x 16 LDS tiles, scalar
//      4-byte staging: the operands are column windows of a wider matrix, 4-byte aligned only), written as 64-bit
//      COMPOSITES (~ordered(key) << 32 | j): ascending composite order == descending key, ascending index. Composites are
//      unique, so the order is total and any correct sort gives the same answer.
//   3. retr_rank_kernel: one workgroup per query sorts the row's composites (bitonic; tiles of 16384 composites = 128 KiB
//      in the LDS, the strides above a tile through the workspace row, which only this workgroup touches) and reads
//      every output off the sorted row: relevance flags, block scans for the running relevant count and the suffix
//      maximum of the precision curve, float64 sums reduced in a fixed tree. No atomics anywhere: bit-reproducible.
#include <stdint.h>
#include "nsvd_common.h"

namespace {

constexpr int RT_MAX_GALLERY = 1 << 18;
constexpr int RT_MAX_D = 1024, RT_MAX_K = 2048;
constexpr int RT_TILE = 16384;                       // composites per LDS tile
constexpr size_t RT_WS_TARGET = (size_t)64 << 20;    // bytes of composite rows per query chunk (at least 64 rows)
constexpr int RT_MIN_ROWS = 64;
constexpr int TK = 16, PAD = 4, TM = 64, TN = 128;

__global__ void __launch_bounds__(256) retr_half_sqnorm_kernel(const float* __restrict__ zg, long ldg, int Ng, int d,
                                                               float* __restrict__ hn) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= Ng) return;
    const float* y = zg + (size_t)row * ldg;
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s = fmaf(y[k], y[k], s);
    s = nsvd_wave_sum(s);
    if (lane == 0) hn[row] = 0.5f * s;
}

// float bits -> unsigned with the same order (-0 was folded into +0 by the caller)
__device__ __forceinline__ uint32_t retr_ordered(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// comps[(i - q0) * Npad + j] for queries q0 <= i < q0 + nq, 0 <= j < Ng
__global__ void __launch_bounds__(256) retr_score_kernel(const float* __restrict__ zq, long ldq,
                                                         const float* __restrict__ zg, long ldg, int q0, int nq, int Ng,
                                                         int d, const float* __restrict__ hn,
                                                         unsigned long long* __restrict__ comps, int Npad) {
    __shared__ float As[2][TK][TM + PAD];
    __shared__ float Bs[2][TK][TN + PAD];
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int t = threadIdx.x;
    const int lane = t & 63, wv = t >> 6;
    const int li = lane & 31, hi = lane >> 5;
    const int wm = wv >> 1, wn = wv & 1;  // this wave: rows 32 wm .., columns 64 wn .. (two 32-column blocks)
    typedef float f32x16_t __attribute__((ext_vector_type(16)));
    f32x16_t acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
    const float* A = zq + (size_t)q0 * ldq;
    const int kk_t = t & 15, rr_t = t >> 4;  // staging: k fastest (both operands are k-contiguous)
    float ra[4], rb[8];
    auto request = [&](int k0) {
        const int gk = k0 + kk_t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + rr_t + 16 * i;
            ra[i] = (gm < nq && gk < d) ? A[(size_t)gm * ldq + gk] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gn = n0 + rr_t + 16 * i;
            rb[i] = (gn < Ng && gk < d) ? zg[(size_t)gn * ldg + gk] : 0.f;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) As[buf][kk_t][rr_t + 16 * i] = ra[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) Bs[buf][kk_t][rr_t + 16 * i] = rb[i];
    };
    request(0);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < d; k0 += TK) {
        const bool more = k0 + TK < d;
        if (more) request(k0 + TK);
#pragma unroll
        for (int kk = 0; kk < TK; kk += 2) {
            const float av = As[buf][kk + hi][32 * wm + li];
            const float b0 = Bs[buf][kk + hi][64 * wn + li], b1 = Bs[buf][kk + hi][64 * wn + 32 + li];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int gn = n0 + 64 * wn + 32 * blk + li;
        if (gn >= Ng) continue;
        const float h = hn ? hn[gn] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gm = m0 + 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (gm >= nq) continue;
            const float key = ((blk ? acc1[r] : acc0[r]) - h) + 0.f;  // + 0: -0 and +0 are one key
            comps[(size_t)gm * Npad + gn] = ((unsigned long long)(~retr_ordered(key)) << 32) | (unsigned)gn;
        }
    }
}

// one bitonic compare-exchange step (stride j of the merge of width k) on `n` composites at `a`; `base` is the global
// index of a[0] (the direction of a pair comes from its global position)
__device__ __forceinline__ void retr_bitonic_step(unsigned long long* a, int n, int base, int k, int j) {
    for (int p = threadIdx.x; p < (n >> 1); p += blockDim.x) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
        const unsigned long long x = a[i], y = a[l];
        const bool up = ((base + i) & k) == 0;
        if ((x > y) == up) {
            a[i] = y;
            a[l] = x;
        }
    }
    __syncthreads();
}

struct RetrOut {
    int32_t* topk_idx;
    uint8_t* topk_rel;
    float* prec_at_k;
    int32_t* hits_at_k;
    double* avg_prec;  // float64: ver 2 divides by the caller's n_relevant_items and is not bounded by 1
    int32_t* n_found;
};

__global__ void __launch_bounds__(1024) retr_rank_kernel(unsigned long long* __restrict__ comps, int Npad, int Ng, int q0,
                                                         int Nq, int K, const int32_t* __restrict__ q_cls,
                                                         const int32_t* __restrict__ g_cls,
                                                         const int32_t* __restrict__ n_relevant_items, RetrOut o) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long tile[];
    __shared__ int ish[1024];
    __shared__ double dsh[1024];
    __shared__ double dsh2[1024];
    const int t = threadIdx.x, T = blockDim.x;
    const int q = q0 + blockIdx.x;
    unsigned long long* row = comps + (size_t)blockIdx.x * Npad;
    const int TL = Npad < RT_TILE ? Npad : RT_TILE;
    const int ntiles = Npad / TL;
    const unsigned long long PADV = ~0ull;  // sorts behind every gallery row

    // ---- sort: every tile on its own, then the merges wider than a tile ----
    for (int tl = 0; tl < ntiles; ++tl) {
        const int base = tl * TL;
        for (int i = t; i < TL; i += T) tile[i] = (base + i < Ng) ? row[base + i] : PADV;
        __syncthreads();
        for (int k = 2; k <= TL; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) retr_bitonic_step(tile, TL, base, k, j);
        if (ntiles > 1) {
            for (int i = t; i < TL; i += T) row[base + i] = tile[i];
            __syncthreads();
        }
    }
    for (int k = TL << 1; k <= Npad; k <<= 1) {
        for (int j = k >> 1; j >= TL; j >>= 1) retr_bitonic_step(row, Npad, 0, k, j);
        for (int tl = 0; tl < ntiles; ++tl) {
            const int base = tl * TL;
            for (int i = t; i < TL; i += T) tile[i] = row[base + i];
            __syncthreads();
            for (int j = TL >> 1; j > 0; j >>= 1) retr_bitonic_step(tile, TL, base, k, j);
            for (int i = t; i < TL; i += T) row[base + i] = tile[i];
            __syncthreads();
        }
    }
    unsigned long long* sorted = ntiles > 1 ? row : tile;

    // ---- relevance flags (composite -> relevant << 32 | index), top K, the two counts ----
    const int32_t qc = q_cls[q];
    int cntK = 0, cntAll = 0;
    for (int p = t; p < Ng; p += T) {
        const unsigned idx = (unsigned)sorted[p];
        const int rel = g_cls[idx] == qc;
        sorted[p] = ((unsigned long long)rel << 32) | idx;
        cntAll += rel;
        if (p < K) {
            cntK += rel;
            if (o.topk_idx) o.topk_idx[(size_t)q * K + p] = (int32_t)idx;
            if (o.topk_rel) o.topk_rel[(size_t)q * K + p] = (uint8_t)rel;
        }
    }
    // (integer sums: any order gives the same value)
    ish[t] = cntK;
    __syncthreads();
    for (int s = T >> 1; s > 0; s >>= 1) {
        if (t < s) ish[t] += ish[t + s];
        __syncthreads();
    }
    if (t == 0) {
        o.prec_at_k[q] = (float)ish[0] / (float)K;
        if (o.hits_at_k) o.hits_at_k[q] = ish[0];
    }
    __syncthreads();
    if (!o.avg_prec) {
        if (o.n_found) {
            ish[t] = cntAll;
            __syncthreads();
            for (int s = T >> 1; s > 0; s >>= 1) {
                if (t < s) ish[t] += ish[t + s];
                __syncthreads();
            }
            if (t == 0) o.n_found[q] = ish[0];
        }
        return;
    }

    // ---- average precisions: thread t owns the ranks seg * t + 1 .. seg * (t + 1) ----
    const int seg = (Ng + T - 1) / T;
    const int p0 = min(Ng, t * seg), p1 = min(Ng, p0 + seg);
    int c = 0;
    for (int p = p0; p < p1; ++p) c += (int)(sorted[p] >> 32);
    ish[t] = c;
    __syncthreads();
    for (int s = 1; s < T; s <<= 1) {  // inclusive scan
        const int x = t >= s ? ish[t - s] : 0;
        __syncthreads();
        ish[t] += x;
        __syncthreads();
    }
    const int before = ish[t] - c, R = ish[T - 1];
    // forward: p_m = m / r_m at the relevant ranks; their sum (ver 2, 3) and this segment's maximum
    double s3 = 0.0, smax = 0.0;
    int m = before;
    for (int p = p0; p < p1; ++p) {
        if (sorted[p] >> 32) {
            ++m;
            const double pm = (double)m / (double)(p + 1);
            s3 += pm;
            smax = fmax(smax, pm);
        }
    }
    dsh[t] = smax;
    __syncthreads();
    for (int s = 1; s < T; s <<= 1) {  // inclusive suffix maximum
        const double x = t + s < T ? dsh[t + s] : 0.0;
        __syncthreads();
        dsh[t] = fmax(dsh[t], x);
        __syncthreads();
    }
    // backward: ver 1 sums the running maximum of p_m' over m' >= m
    double run = t + 1 < T ? dsh[t + 1] : 0.0, s1 = 0.0;
    m = before + c;
    for (int p = p1 - 1; p >= p0; --p) {
        if (sorted[p] >> 32) {
            run = fmax(run, (double)m / (double)(p + 1));
            s1 += run;
            --m;
        }
    }
    __syncthreads();
    dsh[t] = s1;
    dsh2[t] = s3;
    __syncthreads();
    for (int s = T >> 1; s > 0; s >>= 1) {  // fixed tree: the same bits every run
        if (t < s) {
            dsh[t] += dsh[t + s];
            dsh2[t] += dsh2[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double nri = (double)min(Ng, n_relevant_items[q]);
        o.avg_prec[q] = dsh[0] / (double)R;              // 0 / 0 = NaN when nothing is relevant
        o.avg_prec[(size_t)Nq + q] = dsh2[0] / nri;
        o.avg_prec[2 * (size_t)Nq + q] = dsh2[0] / (double)R;
        if (o.n_found) o.n_found[q] = R;
    }
}

int rt_npad(int Ng) {
    int n = 2;
    while (n < Ng) n <<= 1;
    return n;
}
int rt_chunk_rows(int Nq, int Npad) {
    size_t rows = RT_WS_TARGET / ((size_t)Npad * 8);
    if (rows < (size_t)RT_MIN_ROWS) rows = RT_MIN_ROWS;
    if (rows > 32768) rows = 32768;  // (one launch's grid: rows / 64 tiles in y, one rank workgroup per row)
    if (rows > (size_t)Nq) rows = (size_t)Nq;
    return (int)rows;
}
// 0: fine
int rt_validate(int Nq, int Ng, int d, int K) {
    if (Nq < 0 || Ng < 1 || d < 1 || d > RT_MAX_D || K < 1 || K > Ng || K > RT_MAX_K) return NSVD_EINVAL;
    if (Ng > RT_MAX_GALLERY) return NSVD_EUNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int nsvd_retrieval_max_gallery(void) { return RT_MAX_GALLERY; }
extern "C" int nsvd_retrieval_max_k(void) { return RT_MAX_K; }
extern "C" int nsvd_retrieval_max_d(void) { return RT_MAX_D; }

extern "C" size_t nsvd_retrieval_workspace_bytes(int Nq, int Ng, int d, int K) {
    if (rt_validate(Nq, Ng, d, K) != 0) return 0;
    const int Npad = rt_npad(Ng);
    return nsvd_align((size_t)Ng * sizeof(float)) + (size_t)rt_chunk_rows(Nq, Npad) * Npad * 8 + 256;
}

extern "C" int nsvd_retrieval_eval(const float* zq, long ldq, const float* zg, long ldg, int Nq, int Ng, int d,
                                   const int32_t* q_cls, const int32_t* g_cls, const int32_t* n_relevant_items,
                                   int metric, int K, int32_t* topk_idx, uint8_t* topk_rel, float* prec_at_k,
                                   int32_t* hits_at_k, double* avg_prec, int32_t* n_relevant_found, void* ws,
                                   size_t ws_bytes, void* stream) {
    const int rc = rt_validate(Nq, Ng, d, K);
    if (rc != 0) return rc;
    if (metric != NSVD_RETR_INNER_PRODUCT && metric != NSVD_RETR_EUCLIDEAN) return NSVD_EINVAL;
    if (Nq == 0) return 0;
    if (!zq || !zg || !q_cls || !g_cls || !prec_at_k || !ws || ldq < d || ldg < d) return NSVD_EINVAL;
    if (avg_prec && !n_relevant_items) return NSVD_EINVAL;
    if ((((uintptr_t)zq | (uintptr_t)zg) & 3) != 0) return NSVD_EINVAL;
    if (!nsvd_ws_ok(ws, ws_bytes, nsvd_retrieval_workspace_bytes(Nq, Ng, d, K))) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int Npad = rt_npad(Ng), rows = rt_chunk_rows(Nq, Npad);
    float* hn = (float*)ws;
    unsigned long long* comps = (unsigned long long*)((char*)ws + nsvd_align((size_t)Ng * sizeof(float)));
    const int TL = Npad < RT_TILE ? Npad : RT_TILE;
    const size_t lds = (size_t)TL * 8;
    static_assert((size_t)RT_TILE * 8 <= NSVD_LDS_MAX, "LDS of gfx950");
    static NsvdLdsOptIn lds_opt_in;
    if (const int e = nsvd_lds_opt_in(lds_opt_in, {(const void*)retr_rank_kernel}, (size_t)RT_TILE * 8)) return e;
    if (metric == NSVD_RETR_EUCLIDEAN) {
        hipLaunchKernelGGL(retr_half_sqnorm_kernel, dim3(nsvd_cdiv(Ng, 4)), dim3(256), 0, s, zg, ldg, Ng, d, hn);
        NSVD_CHECK_LAUNCH();
    }
    RetrOut o;
    o.topk_idx = topk_idx;
    o.topk_rel = topk_rel;
    o.prec_at_k = prec_at_k;
    o.hits_at_k = hits_at_k;
    o.avg_prec = avg_prec;
    o.n_found = n_relevant_found;
    const int threads = Npad > 4096 ? 1024 : 256;
    for (int q0 = 0; q0 < Nq; q0 += rows) {
        const int nq = Nq - q0 < rows ? Nq - q0 : rows;
        hipLaunchKernelGGL(retr_score_kernel, dim3(nsvd_cdiv(Ng, TN), nsvd_cdiv(nq, TM)), dim3(256), 0, s, zq, ldq, zg,
                           ldg, q0, nq, Ng, d, metric == NSVD_RETR_EUCLIDEAN ? hn : (const float*)nullptr, comps, Npad);
        NSVD_CHECK_LAUNCH();
        hipLaunchKernelGGL(retr_rank_kernel, dim3(nq), dim3(threads), lds, s, comps, Npad, Ng, q0, Nq, K, q_cls, g_cls,
                           n_relevant_items, o);
        NSVD_CHECK_LAUNCH();
    }
    return 0;
}
