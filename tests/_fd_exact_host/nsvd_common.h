// Host stand-in for csrc/nsvd_common.h: lets g++ compile csrc/fd_math.h (copied beside this file by
// tests/test_generic_exact_oracle.py) so that the exact-Laplacian product rule of NSVD_PATH_GENERIC_EXACT runs in float32
// on the CPU. Only what fd_math.h uses, restated from csrc/nsvd_common.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "nsvd.h"
#define __device__
#define __forceinline__ inline
#define NSVD_SQRT_P_CLAMP 1e-5f
#define NSVD_SMALL_D 4
#define NSVD_MAX_D 12
struct NsvdBox { int mode; float lim; };
inline float nsvd_sqrt_gauss_pdf(const float* xr, int D, float sigma, float log_norm) {
    float M = 0.f; for (int d = 0; d < D; ++d) { const float t = xr[d] / sigma; M = fmaf(t, t, M); }
    return sqrtf(expf(-0.5f * M + log_norm)); }
static inline float nsvd_gauss_log_norm(int D, float sigma) { return (float)(-0.5 * D * 1.8378770664093453 - D * log((double)sigma)); }
inline float nsvd_stencil_coord(float xc, int d, int e, float eps) { if (e == 0) return xc; const int axis = (e - 1) >> 1; if (axis != d) return xc; return ((e - 1) & 1) ? xc - eps : xc + eps; }
