// The direction-loop epilogue of csrc/fd_math.h (nsvd_fd_row_nd + nsvd_fd_evenodd_nd, the form of 5 <= D <= 12) on the
// host, in float32, for tests/test_highdim_host_epilogue.py. `base` is laid out as the generic path hands it to the
// kernel: (L, ldr) with row block e of B samples at e B (0 the centre, 1 + 2 d / 2 + 2 d the even / odd parts along d).
// trig: the template instance (1: the periodic problems).
#include "fd_math.h"
template <bool TRIG>
static void run_t(const nsvd_problem* prob, int D, int B, int L, int has_mask, const float* scales, const float* x,
                  const float* base, int ldr, NsvdBox box, float* f, float* Tf, float* jac, float* dsc) {
    const float ln = nsvd_importance_log_norm(D, *prob);
    for (int b = 0; b < B; ++b) {
        const float* xr = x + (size_t)b * D;
        const NsvdFdRowNd w = nsvd_fd_row_nd<TRIG>(xr, D, *prob, ln, box);
        float dir[NSVD_MAX_D * NSVD_FD_DIR_FIELDS];  // what the heads share per direction: one row's table, es = 1
        for (int d = 0; d < D; ++d) nsvd_fd_dir_nd<TRIG>(w, xr, d, D, has_mask != 0, *prob, box, dir, 1);
        for (int l = 0; l < L; ++l) {
            const int i = b * L + l;
            const NsvdFdOut o = nsvd_fd_evenodd_nd<TRIG>(w, xr, base + (size_t)l * ldr + b, (size_t)B, D, has_mask != 0,
                                                         has_mask ? scales[l] : 0.f, *prob, box, dir, 1);
            f[i] = o.f; Tf[i] = o.Tf; jac[i] = o.jac; dsc[i] = o.dsc;
        }
    }
}
extern "C" void run_nd(const nsvd_problem* prob, int D, int B, int L, int has_mask, const float* scales, const float* x,
                       const float* base, int ldr, int box_mode, float box_lim, int trig, float* f, float* Tf,
                       float* jac, float* dsc) {
    NsvdBox box{box_mode, box_lim};
    if (trig) run_t<true>(prob, D, B, L, has_mask, scales, x, base, ldr, box, f, Tf, jac, dsc);
    else run_t<false>(prob, D, B, L, has_mask, scales, x, base, ldr, box, f, Tf, jac, dsc);
}
