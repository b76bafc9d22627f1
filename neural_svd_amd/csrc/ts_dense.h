// What the dense sides of the two block solvers share (nystrom.hip: the Nystrom baseline; nystrom_svd.hip: the
// truncated-SVD baseline): the limits of a block, the slice rule, and the Gram kernels of tall-skinny float32 blocks with
// the body of their entry points. The two m x m solve kernels stay whole in their files. Every device loop has a trip
// count bounded by an argument or a constant; no atomics. Everything has internal linkage: each file gets its own.
#pragma once
#include "nsvd_kernels.h"

constexpr int NY_MAXM = 80;     // block width limit (64 pairs + 16 columns of oversampling)
constexpr int NY_THREADS = 256;
constexpr int NY_CB = 5;        // column blocks of 16: 5 * 16 = NY_MAXM
constexpr int TS_ROWS = 32;     // rows of X (and Y) per LDS chunk of the Gram kernel
constexpr int TS_MAX_SLICES = 128, TS_SLICE_ROWS = 64;

static inline int ts_slices(int n) {
    const int s = nsvd_cdiv(n, TS_SLICE_ROWS);
    return s < 1 ? 1 : (s > TS_MAX_SLICES ? TS_MAX_SLICES : s);
}

// ---- Gram matrices of (n, m) float32 blocks ----------------------------------------------------------------------------
// part[slice][0 | 1 | 2] = X_s^T X_s | X_s^T Y_s | Y_s^T Y_s (each (m, m); YY false: two slots a slice), the requested
// ones written. Thread (ti, tj) = (t / 16, t % 16) owns the outputs (ti + 16 a, tj + 16 b), a, b < 5, of every product:
// per row of the chunk five reads per operand side (the ti side two addresses per half wave: broadcast; the tj side 16
// consecutive floats) and 25 float64 FMAs per product. Each row tile of X and Y is staged once for all of them.
template <bool XX, bool XY, bool YY>
static __global__ void __launch_bounds__(NY_THREADS) tsgram_partial_kernel(const float* __restrict__ X, size_t ldx,
                                                                           const float* __restrict__ Y, size_t ldy, int n,
                                                                           int m, int S, double* __restrict__ part) {
    constexpr bool HAS_Y = XY || YY;
    __shared__ float xs[TS_ROWS][NY_MAXM];
    __shared__ float ys[HAS_Y ? TS_ROWS : 1][NY_MAXM];
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15, slice = blockIdx.x;
    const int r0 = (int)((long)n * slice / S), r1 = (int)((long)n * (slice + 1) / S);
    double axx[NY_CB][NY_CB], axy[NY_CB][NY_CB], ayy[NY_CB][NY_CB];
#pragma unroll
    for (int a = 0; a < NY_CB; ++a)
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) axx[a][b] = axy[a][b] = ayy[a][b] = 0.0;
    for (int rb = r0; rb < r1; rb += TS_ROWS) {
        const int rows = min(TS_ROWS, r1 - rb);
        __syncthreads();
        for (int e = t; e < TS_ROWS * NY_MAXM; e += NY_THREADS) {
            const int r = e / NY_MAXM, c = e - r * NY_MAXM;
            const bool in = r < rows && c < m;
            xs[r][c] = in ? X[(size_t)(rb + r) * ldx + c] : 0.f;
            if (HAS_Y) ys[r][c] = in ? Y[(size_t)(rb + r) * ldy + c] : 0.f;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            double xa[NY_CB], xb[NY_CB], ya[NY_CB], yb[NY_CB];
#pragma unroll
            for (int a = 0; a < NY_CB; ++a) {
                xa[a] = (double)xs[r][ti + 16 * a];
                if (XX) xb[a] = (double)xs[r][tj + 16 * a];
                if (YY) ya[a] = (double)ys[r][ti + 16 * a];
                if (HAS_Y) yb[a] = (double)ys[r][tj + 16 * a];
            }
#pragma unroll
            for (int a = 0; a < NY_CB; ++a)
#pragma unroll
                for (int b = 0; b < NY_CB; ++b) {
                    if (XX) axx[a][b] = fma(xa[a], xb[b], axx[a][b]);
                    if (XY) axy[a][b] = fma(xa[a], yb[b], axy[a][b]);
                    if (YY) ayy[a][b] = fma(ya[a], yb[b], ayy[a][b]);
                }
        }
    }
    const size_t mm = (size_t)m * m;
    double* p = part + (size_t)slice * (YY ? 3 : 2) * mm;
#pragma unroll
    for (int a = 0; a < NY_CB; ++a)
#pragma unroll
        for (int b = 0; b < NY_CB; ++b) {
            const int i = ti + 16 * a, j = tj + 16 * b;
            if (i < m && j < m) {
                if (XX) p[i * m + j] = axx[a][b];
                if (XY) p[mm + i * m + j] = axy[a][b];
                if (YY) p[2 * mm + i * m + j] = ayy[a][b];
            }
        }
}

// out[e] = sum over slices in slice order; blockIdx.y < slots: 0 = XtX, 1 = XtY, 2 = YtY (a null output is skipped)
static __global__ void __launch_bounds__(NY_THREADS) tsgram_reduce_kernel(const double* __restrict__ part, int m, int S,
                                                                          int slots, double* __restrict__ XtX,
                                                                          double* __restrict__ XtY,
                                                                          double* __restrict__ YtY) {
    double* out = blockIdx.y == 0 ? XtX : (blockIdx.y == 1 ? XtY : YtY);
    const int e = blockIdx.x * NY_THREADS + threadIdx.x, mm = m * m;
    if (!out || e >= mm) return;
    const double* p = part + (size_t)blockIdx.y * mm + e;
    double s = 0.0;
    for (int sl = 0; sl < S; ++sl) s += p[(size_t)sl * slots * mm];
    out[e] = s;
}

static inline size_t ts_gram_workspace_bytes(int n, int m, int slots) {
    if (n <= 0 || m <= 0 || m > NY_MAXM) return 0;
    return nsvd_align((size_t)ts_slices(n) * slots * m * m * sizeof(double));
}

// The body of a Gram entry point behind its own refusals: the checks both share, then the partial and the reduce launch.
// YY: nsvd_tsgram3_f64 (three slots a slice, all outputs given); else nsvd_tsgram_f64 (two slots, XtX or XtY may be null).
template <bool YY>
static inline int ts_gram(const float* X, long ldx, const float* Y, long ldy, int n, int m, double* XtX, double* XtY,
                          double* YtY, void* ws, size_t ws_bytes, void* stream) {
    constexpr int slots = YY ? 3 : 2;
    if (!X || !ws || n <= 0 || m <= 0 || ldx < m) return NSVD_EINVAL;
    if (XtY && (!Y || ldy < m)) return NSVD_EINVAL;
    if (m > NY_MAXM) return NSVD_EUNSUPPORTED;
    if (!nsvd_ws_ok(ws, ws_bytes, ts_gram_workspace_bytes(n, m, slots))) return NSVD_EINVAL;
    const int S = ts_slices(n);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    if constexpr (YY)  // (each file instantiates its own kernels only)
        tsgram_partial_kernel<true, true, true><<<S, NY_THREADS, 0, s>>>(X, (size_t)ldx, Y, (size_t)ldy, n, m, S, part);
    else if (XtX && XtY)
        tsgram_partial_kernel<true, true, false><<<S, NY_THREADS, 0, s>>>(X, (size_t)ldx, Y, (size_t)ldy, n, m, S, part);
    else if (XtX)
        tsgram_partial_kernel<true, false, false><<<S, NY_THREADS, 0, s>>>(X, (size_t)ldx, nullptr, 0, n, m, S, part);
    else
        tsgram_partial_kernel<false, true, false><<<S, NY_THREADS, 0, s>>>(X, (size_t)ldx, Y, (size_t)ldy, n, m, S, part);
    NSVD_CHECK_LAUNCH();
    tsgram_reduce_kernel<<<dim3(nsvd_cdiv(m * m, NY_THREADS), slots), NY_THREADS, 0, s>>>(part, m, S, slots, XtX, XtY,
                                                                                         YtY);
    NSVD_CHECK_LAUNCH();
    return 0;
}
