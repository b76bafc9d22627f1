// The exact-Laplacian epilogue of NSVD_PATH_GENERIC_EXACT (csrc/fd_math.h) on the host, in float32, for
// tests/test_generic_exact_oracle.py: nsvd_fd_exact up to D = 4, the direction-loop form (nsvd_fd_row_nd +
// nsvd_fd_exact_dirs_nd + nsvd_fd_exact_nd) above, both as fd_epilogue.hip's kernels call them. `base` is laid out as
// the generic jets hand it over: (L, ldr) with row block 0 of B samples the head's value, blocks 1 .. D its derivatives
// along each axis, block D + 1 its Laplacian.
#include "fd_math.h"
// TRIG: the instance of nsvd_fd_row_nd, chosen as nsvd_fd_epilogue_exact chooses its kernel (the cosine potential)
template <bool TRIG>
static void run_t(const nsvd_problem* prob, int D, int B, int L, int has_mask, const float* scales, const float* x,
                  const float* base, int ldr, int box_mode, float box_lim, float* f, float* Tf, float* jac, float* dsc) {
    const NsvdBox box{box_mode, box_lim};
    const float ln = nsvd_importance_log_norm(D, *prob);
    for (int b = 0; b < B; ++b) {
        const float* xr = x + (size_t)b * D;
        if (D <= NSVD_FD_MAXD) {
            for (int l = 0; l < L; ++l) {
                const float* bcol = base + (size_t)l * ldr + b;
                float xc[NSVD_FD_MAXD], db[NSVD_FD_MAXD];
                for (int d = 0; d < NSVD_FD_MAXD; ++d) {
                    xc[d] = d < D ? xr[d] : 0.f;
                    db[d] = d < D ? bcol[(size_t)(1 + d) * B] : 0.f;
                }
                const NsvdFdOut o = nsvd_fd_exact(bcol[0], db, bcol[(size_t)(D + 1) * B], xc, D, has_mask != 0,
                                                  has_mask ? scales[l] : 0.f, *prob, ln, box);
                const int i = b * L + l;
                f[i] = o.f; Tf[i] = o.Tf; jac[i] = o.jac; dsc[i] = o.dsc;
            }
            continue;
        }
        const NsvdFdRowNd w = nsvd_fd_row_nd<TRIG>(xr, D, *prob, ln, box);
        float dir[NSVD_MAX_D * NSVD_FDX_DIR_FIELDS];  // one row's table, es = 1
        const NsvdFdExactRowNd e = nsvd_fd_exact_dirs_nd(xr, D, box, dir, 1);
        for (int l = 0; l < L; ++l) {
            const NsvdFdOut o = nsvd_fd_exact_nd(w, e, base + (size_t)l * ldr + b, (size_t)B, D, has_mask != 0,
                                                 has_mask ? scales[l] : 0.f, *prob, box, dir, 1);
            const int i = b * L + l;
            f[i] = o.f; Tf[i] = o.Tf; jac[i] = o.jac; dsc[i] = o.dsc;
        }
    }
}
extern "C" void run_exact(const nsvd_problem* prob, int D, int B, int L, int has_mask, const float* scales,
                          const float* x, const float* base, int ldr, int box_mode, float box_lim, float* f, float* Tf,
                          float* jac, float* dsc) {
    if (prob->potential == NSVD_POT_COSINE)
        run_t<true>(prob, D, B, L, has_mask, scales, x, base, ldr, box_mode, box_lim, f, Tf, jac, dsc);
    else
        run_t<false>(prob, D, B, L, has_mask, scales, x, base, ldr, box_mode, box_lim, f, Tf, jac, dsc);
}
