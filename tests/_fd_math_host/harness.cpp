// The per-(sample, head) epilogue math of csrc/fd_math.h on the host, in float32, for tests/test_periodic_host_epilogue.py:
// mode 0 the even / odd form, mode 1 the point-wise form; run_exact the exact-Laplacian product rule.
#include "fd_math.h"
extern "C" void run(const nsvd_problem* prob, int D, int B, int L, int has_mask, const float* scales, const float* x,
                    const float* base0, const float* bE, const float* bO, const float* bv, int mode, float* f, float* Tf) {
    NsvdBox box{0, 0.f};
    const float ln = nsvd_importance_log_norm(D, *prob);
    for (int b = 0; b < B; ++b) for (int l = 0; l < L; ++l) {
        const int i = b * L + l;
        NsvdFdOut o;
        if (mode == 0) o = nsvd_fd_evenodd(base0[i], bE + (size_t)i * D, bO + (size_t)i * D, x + (size_t)b * D, D, has_mask, has_mask ? scales[l] : 0.f, *prob, ln, box);
        else o = nsvd_fd_point(bv + (size_t)i * (1 + 2 * D), x + (size_t)b * D, D, has_mask, has_mask ? scales[l] : 0.f, *prob, ln, box);
        f[i] = o.f; Tf[i] = o.Tf;
    }
}
extern "C" void run_exact(const nsvd_problem* prob, int D, int B, int L, int has_mask, const float* scales, const float* x,
                    const float* base, const float* dbase, const float* lbase, float* f, float* Tf) {
    NsvdBox box{0, 0.f};
    const float ln = nsvd_importance_log_norm(D, *prob);
    for (int b = 0; b < B; ++b) for (int l = 0; l < L; ++l) {
        const int i = b * L + l;
        NsvdFdOut o = nsvd_fd_exact(base[i], dbase + (size_t)i * D, lbase[i], x + (size_t)b * D, D, has_mask, has_mask ? scales[l] : 0.f, *prob, ln, box);
        f[i] = o.f; Tf[i] = o.Tf;
    }
}
