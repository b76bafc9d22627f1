// The no-atomics scatter of a batch into the index space, S^T[l][j] = sum_{k: cols_k = j} f[k][l], shared by the dense
// products (kernel_apply.hip, kernel_apply_pair.hip). Internal linkage, a template so that a file's code object holds
// it only when the file launches it (as the kernels of apply_common.h and pair_common.h).
#pragma once
#include "nsvd_common.h"

// One workgroup owns 32 consecutive points and a block of 64 heads, scans the batch's column indices for hits (8
// consecutive k per thread, hits listed in k order through a prefix sum over the workgroup) and adds the hit rows of f in
// that order: S^T is bit-reproducible whatever the duplicates, every element is written exactly once (zeros included,
// also the columns N .. Np of the padding), and 0.5 M float atomics (28 us at configs[3]) become a 64 KB scan per
// workgroup. grid (Np / KS_PB, Lp / 64); indices outside [0, N) hit nothing.
constexpr int KS_PB = 32;      // points per workgroup
constexpr int KS_RK = 8192;    // batch entries per round (the hit list can hold them all)
constexpr int KS_PT = KS_RK / 256;  // consecutive entries per thread
template <int = 0>
static __global__ void __launch_bounds__(256) ka_scatter_blocks_kernel(const float* __restrict__ f,
                                                                       const long long* __restrict__ cols, int B2, int L,
                                                                       int N, float* __restrict__ ST, int Np) {
    __shared__ int hit_k[KS_RK];
    __shared__ unsigned char hit_j[KS_RK];
    __shared__ int wsum[4], total;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int j0 = blockIdx.x * KS_PB, l0 = blockIdx.y * 64;
    const int jj = t & 31, lq = t >> 5;  // this thread accumulates point j0 + jj, heads l0 + 8 lq .. + 7
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < B2; k0 += KS_RK) {
        // hits of this round, in k order (bit i of `mask`: entry k0 + KS_PT t + i hits point j0 + pj[i])
        unsigned mask = 0;
        unsigned char pj[KS_PT];
#pragma unroll
        for (int i = 0; i < KS_PT; ++i) {
            const int k = k0 + KS_PT * t + i;
            const long long c = k < B2 ? cols[k] : -1;
            const bool hit = c >= j0 && c < j0 + KS_PB && c < N;
            pj[i] = hit ? (unsigned char)(c - j0) : 0;
            mask |= hit ? (1u << i) : 0u;
        }
        const int cnt = __builtin_popcount(mask);
        int incl = cnt;  // inclusive prefix over the wave, then over the four waves
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int base = incl - cnt;
        for (int q = 0; q < wv; ++q) base += wsum[q];
        if (t == 255) total = base + cnt;
#pragma unroll
        for (int i = 0; i < KS_PT; ++i)
            if (mask & (1u << i)) {
                hit_k[base] = k0 + KS_PT * t + i;
                hit_j[base] = pj[i];
                ++base;
            }
        __syncthreads();
        // this thread's point: its hits are collected first (up to four at a time), their rows of f requested together -
        // one memory latency per pass instead of one per hit - and added in k order
        const int nh = total;
        int e = 0;
        while (e < nh) {
            int ks[4], n = 0;
            for (; e < nh && n < 4; ++e)
                if (hit_j[e] == jj) ks[n++] = hit_k[e];
            float4 v[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i][0] = v[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < n) {
                    const float* fr = f + (size_t)ks[i] * L + l0 + 8 * lq;
                    if (l0 + 8 * lq + 8 <= L && (L & 3) == 0) {
                        v[i][0] = *reinterpret_cast<const float4*>(fr);
                        v[i][1] = *reinterpret_cast<const float4*>(fr + 4);
                    } else {
                        float tmp[8];
                        for (int q = 0; q < 8; ++q) tmp[q] = l0 + 8 * lq + q < L ? fr[q] : 0.f;
                        v[i][0] = make_float4(tmp[0], tmp[1], tmp[2], tmp[3]);
                        v[i][1] = make_float4(tmp[4], tmp[5], tmp[6], tmp[7]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[0] += v[i][0].x; acc[1] += v[i][0].y; acc[2] += v[i][0].z; acc[3] += v[i][0].w;
                acc[4] += v[i][1].x; acc[5] += v[i][1].y; acc[6] += v[i][1].z; acc[7] += v[i][1].w;
            }
        }
        __syncthreads();  // the list is rewritten in the next round
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) ST[(size_t)(l0 + 8 * lq + i) * Np + j0 + jj] = acc[i];
}
