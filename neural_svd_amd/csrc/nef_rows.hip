// NeuralEF on a matrix-free kernel operator: BatchL2NormalizedFunctions in training mode (methods/utils.py:48-68) on a
// plain (B, L) block of raw head outputs, and its reverse mode. The block is tall and narrow (B up to 65536, L <= 64):
// the column reductions run over many blocks of rows and are finished in a fixed order, in float64, without atomics.
//   nef_rows_sumsq_kernel  per block of rows (never across the segment boundary): column sums of u^2, rows in order
//   nef_rows_scale_kernel  every workgroup adds the partials of ITS segment in a fixed order (the same bits everywhere),
//                          n = sqrt(sum / B_h), phi = u / n; workgroup 0 also writes stats and takes the running-norm
//                          updates in the caller's order
//   nef_rows_dot_kernel    per block of rows: column sums of g phi, g = dphi (+ dphi1 + dphi2)
//   nef_rows_du_kernel     s = ordered sum / B_h as above, du = (g - phi s) / n
#include "nsvd_kernels.h"

namespace {

constexpr int NR_TILE = 64;     // rows staged at a time
constexpr int NR_MAXL = 64;
constexpr int NR_BLOCKS = 128;  // blocks of rows aimed at: every workgroup of the second pass adds that many partials
constexpr int NR_MAXB = 65536;

struct NefRows {
    int B, L;
    int Bh[2];    // rows of each segment (Bh[1] == 0: one segment)
    int rpb;      // rows per block, a multiple of NR_TILE
    int nblk[2];  // blocks of each segment
    double* part; // (nblk[0] + nblk[1], L)
};

struct NefOrder {
    int n;
    int seg[4];
};

__host__ __device__ inline int nef_rows_rpb(int B) { return NR_TILE * ((B + NR_TILE * NR_BLOCKS - 1) / (NR_TILE * NR_BLOCKS)); }

// the rows [r0, r0 + nr) of workgroup `blk` and its segment
__device__ __forceinline__ void block_rows(const NefRows& a, int blk, int& h, int& r0, int& nr) {
    h = blk < a.nblk[0] ? 0 : 1;
    const int k = blk - (h ? a.nblk[0] : 0);
    const int s0 = k * a.rpb;
    nr = min(a.rpb, a.Bh[h] - s0);
    r0 = (h ? a.Bh[0] : 0) + s0;
}

// column sums of vals (nr, L) held in LDS tile by tile: thread (c, q) adds the rows q, q + 4, ... of column c of every
// tile in row order, then the four quarter sums are added in a fixed order
template <class Stage>
__device__ __forceinline__ void column_sums(const NefRows& a, int r0, int nr, double* tile, double* red, double* out,
                                            Stage stage) {
    const int L = a.L, c = threadIdx.x & 63, q = threadIdx.x >> 6;
    double acc = 0.0;
    for (int t0 = 0; t0 < nr; t0 += NR_TILE) {
        const int tr = min(NR_TILE, nr - t0);
        const size_t base = (size_t)(r0 + t0) * L;
        __syncthreads();
        for (int t = threadIdx.x; t < tr * L; t += blockDim.x) tile[t] = stage(base + t);
        __syncthreads();
        if (c < L)
            for (int k = q; k < tr; k += 4) acc += tile[k * L + c];
    }
    red[q * NR_MAXL + c] = acc;
    __syncthreads();
    if (q == 0 && c < L) out[c] = (red[c] + red[NR_MAXL + c]) + (red[2 * NR_MAXL + c] + red[3 * NR_MAXL + c]);
}

// out[c] = the partials of segment h, column c, added in a fixed order by the whole workgroup: thread (c, q) adds the
// blocks q, q + 4, ... in block order, then the four quarter sums are added as in column_sums (the same bits in every
// workgroup). red: 4 * NR_MAXL doubles, out: NR_MAXL; ends with a barrier.
__device__ __forceinline__ void ordered_sums(const NefRows& a, int h, double* red, double* out) {
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    double s = 0.0;
    if (c < a.L) {
        const double* p = a.part + (size_t)(h ? a.nblk[0] : 0) * a.L + c;
        for (int k = q; k < a.nblk[h]; k += 4) s += p[(size_t)k * a.L];
    }
    red[q * NR_MAXL + c] = s;
    __syncthreads();
    if (q == 0 && c < a.L) out[c] = (red[c] + red[NR_MAXL + c]) + (red[2 * NR_MAXL + c] + red[3 * NR_MAXL + c]);
    __syncthreads();
}

__global__ void __launch_bounds__(256) nef_rows_sumsq_kernel(NefRows a, const float* __restrict__ u) {
    __shared__ double tile[NR_TILE * NR_MAXL];
    __shared__ double red[4 * NR_MAXL];
    int h, r0, nr;
    block_rows(a, blockIdx.x, h, r0, nr);
    column_sums(a, r0, nr, tile, red, a.part + (size_t)blockIdx.x * a.L, [&](size_t i) {
        const double v = (double)u[i];
        return v * v;
    });
}

__global__ void __launch_bounds__(256) nef_rows_scale_kernel(NefRows a, const float* u, float* phi,
                                                             float* __restrict__ stats, float* __restrict__ rn_b,
                                                             float* __restrict__ rn_u, int* __restrict__ initialized,
                                                             float momentum, NefOrder order) {
    __shared__ double red[4 * NR_MAXL];
    __shared__ double sums[2][NR_MAXL];
    __shared__ float ns[NR_MAXL];
    int h, r0, nr;
    block_rows(a, blockIdx.x, h, r0, nr);
    const int L = a.L;
    ordered_sums(a, h, red, sums[0]);
    if (blockIdx.x == 0 && a.Bh[1]) ordered_sums(a, 1, red, sums[1]);  // (workgroup 0 lies in segment 0)
    if ((int)threadIdx.x < L) {
        const int l = threadIdx.x;
        const float n_own = (float)sqrt(sums[0][l] / (double)a.Bh[h]);
        ns[l] = n_own;
        if (blockIdx.x == 0) {  // (segment 0)
            float n[2];
            n[0] = n_own;
            n[1] = a.Bh[1] ? (float)sqrt(sums[1][l] / (double)a.Bh[1]) : n_own;
            stats[l] = n[0];
            stats[L + l] = n[1];
            if (order.n > 0) {
                // BatchL2NormalizedFunctions.update_norm, once per entry of the caller's order
                float rb = rn_b[l], ru = rn_u[l];
                const int init = *initialized;
                const float m1 = 1.f - momentum;
                for (int e = 0; e < order.n; ++e) {
                    const float ne = n[order.seg[e]];
                    if (e == 0 && !init) {
                        rb = ne;
                        ru = ne;
                    } else {
                        rb = momentum * rb + m1 * ne;
                        ru = sqrtf(momentum * (ru * ru) + m1 * (ne * ne));
                    }
                }
                rn_b[l] = rb;
                rn_u[l] = ru;
            }
        }
    }
    __syncthreads();
    // (every thread of workgroup 0 that read *initialized has done so before the barrier above)
    if (blockIdx.x == 0 && threadIdx.x == 0 && order.n > 0) *initialized = 1;
    const size_t base = (size_t)r0 * L;
    for (int t = threadIdx.x; t < nr * L; t += blockDim.x) phi[base + t] = u[base + t] / ns[t % L];
}

__device__ __forceinline__ double cotangent(const float* dphi, const float* d1, const float* d2, size_t i) {
    double g = (double)dphi[i];
    if (d1) g = (g + (double)d1[i]) + (double)d2[i];
    return g;
}

__global__ void __launch_bounds__(256) nef_rows_dot_kernel(NefRows a, const float* __restrict__ phi, const float* dphi,
                                                           const float* __restrict__ d1, const float* __restrict__ d2) {
    __shared__ double tile[NR_TILE * NR_MAXL];
    __shared__ double red[4 * NR_MAXL];
    int h, r0, nr;
    block_rows(a, blockIdx.x, h, r0, nr);
    column_sums(a, r0, nr, tile, red, a.part + (size_t)blockIdx.x * a.L,
                [&](size_t i) { return cotangent(dphi, d1, d2, i) * (double)phi[i]; });
}

// stats == nullptr: du = g alone (a.part unused)
__global__ void __launch_bounds__(256) nef_rows_du_kernel(NefRows a, const float* __restrict__ phi,
                                                          const float* __restrict__ stats, const float* dphi,
                                                          const float* __restrict__ d1, const float* __restrict__ d2,
                                                          float* du) {
    __shared__ double red[4 * NR_MAXL];
    __shared__ double ss[NR_MAXL];
    __shared__ double ns[NR_MAXL];
    int h, r0, nr;
    block_rows(a, blockIdx.x, h, r0, nr);
    const int L = a.L;
    const size_t base = (size_t)r0 * L;
    if (!stats) {
        for (int t = threadIdx.x; t < nr * L; t += blockDim.x) du[base + t] = (float)cotangent(dphi, d1, d2, base + t);
        return;
    }
    ordered_sums(a, h, red, ss);
    if ((int)threadIdx.x < L) {
        ss[threadIdx.x] = ss[threadIdx.x] / (double)a.Bh[h];
        ns[threadIdx.x] = (double)stats[h * L + threadIdx.x];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nr * L; t += blockDim.x) {
        const int l = t % L;
        const double g = cotangent(dphi, d1, d2, base + t);  // (du may alias dphi: read before the store below)
        du[base + t] = (float)((g - (double)phi[base + t] * ss[l]) / ns[l]);
    }
}

bool rows_shape_ok(int B, int L) { return L >= 1 && L <= NR_MAXL && B >= 1 && B <= NR_MAXB; }

// 0 or an error code; fills `a`
int rows_args(int B, int B1, int L, void* ws, size_t ws_bytes, NefRows* a) {
    if (!rows_shape_ok(B, L)) return NSVD_EUNSUPPORTED;
    if (B1 < 1 || B1 > B) return NSVD_EINVAL;
    if (!nsvd_ws_ok(ws, ws_bytes, nsvd_nef_rows_workspace_bytes(B, L))) return NSVD_EINVAL;
    a->B = B;
    a->L = L;
    a->Bh[0] = B1;
    a->Bh[1] = B - B1;
    a->rpb = nef_rows_rpb(B);
    a->nblk[0] = nsvd_cdiv(B1, a->rpb);
    a->nblk[1] = nsvd_cdiv(B - B1, a->rpb);
    a->part = (double*)ws;
    return 0;
}

}  // namespace

extern "C" size_t nsvd_nef_rows_workspace_bytes(int B, int L) {
    if (!rows_shape_ok(B, L)) return 0;
    // (two segments: each rounds its block count up)
    return nsvd_align((size_t)(nsvd_cdiv(B, nef_rows_rpb(B)) + 1) * L * sizeof(double));
}

extern "C" int nsvd_nef_rows_forward(const float* u, int B, int B1, int L, float* phi, float* stats, float* norm_biased,
                                     float* norm_unbiased, int* initialized, float momentum, const int* order,
                                     int n_order, void* ws, size_t ws_bytes, void* stream) {
    NefRows a;
    const int rc = rows_args(B, B1, L, ws, ws_bytes, &a);
    if (rc) return rc;
    if (!u || !phi || !stats || n_order < 0 || n_order > 4) return NSVD_EINVAL;
    if (n_order > 0 && (!order || !norm_biased || !norm_unbiased || !initialized)) return NSVD_EINVAL;
    NefOrder o;
    o.n = n_order;
    for (int e = 0; e < 4; ++e) {
        o.seg[e] = e < n_order ? order[e] : 0;
        if (o.seg[e] < 0 || o.seg[e] > (a.Bh[1] ? 1 : 0)) return NSVD_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const int nb = a.nblk[0] + a.nblk[1];
    hipLaunchKernelGGL(nef_rows_sumsq_kernel, dim3(nb), dim3(256), 0, s, a, u);
    NSVD_CHECK_LAUNCH();
    hipLaunchKernelGGL(nef_rows_scale_kernel, dim3(nb), dim3(256), 0, s, a, u, phi, stats, norm_biased, norm_unbiased,
                       initialized, momentum, o);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_nef_rows_backward(const float* phi, const float* stats, int B, int B1, int L, const float* dphi,
                                      const float* dphi1, const float* dphi2, float* du, void* ws, size_t ws_bytes,
                                      void* stream) {
    NefRows a;
    const int rc = rows_args(B, B1, L, ws, ws_bytes, &a);
    if (rc) return rc;
    if (!dphi || !du || (stats && !phi) || ((dphi1 == nullptr) != (dphi2 == nullptr))) return NSVD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int nb = a.nblk[0] + a.nblk[1];
    if (stats) {
        hipLaunchKernelGGL(nef_rows_dot_kernel, dim3(nb), dim3(256), 0, s, a, phi, dphi, dphi1, dphi2);
        NSVD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(nef_rows_du_kernel, dim3(nb), dim3(256), 0, s, a, phi, stats, dphi, dphi1, dphi2, du);
    NSVD_CHECK_LAUNCH();
    return 0;
}
