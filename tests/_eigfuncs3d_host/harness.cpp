// Host program around the three-quantum-number part of csrc/eig_math.h: nsvd_eig3_table_fill (validation, lgamma
// normalisations) and nsvd_eig3_eval (the per-function device math of eigfuncs.hip's 3-D instances) compiled for the
// CPU, so that tests/test_eigfunc3d_oracle.py can run them under -fsanitize=address,undefined and hold them to the
// golden values.
//   stdin:  kind param Lg B, then Lg triples (n, l, m), then B triples of float32 coordinates (%.9g round-trips)
//   stdout: the return code of nsvd_eig3_table_fill, then (code 0) B * Lg values row-major, %.17g
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "nsvd.h"
#include "eig_math.h"

int main() {
    int kind, Lg, B;
    double param;
    if (scanf("%d %lf %d %d", &kind, &param, &Lg, &B) != 4 || Lg < 0 || Lg > 4096 || B < 0) return 2;
    std::vector<int> q(3 * (size_t)Lg);
    for (int& v : q)
        if (scanf("%d", &v) != 1) return 2;
    std::vector<float> x(3 * (size_t)B);
    for (float& v : x)
        if (scanf("%f", &v) != 1) return 2;
    NsvdEigTable3 tab = {};
    const int rc = nsvd_eig3_table_fill(kind, param, q.data(), Lg, &tab);
    printf("%d\n", rc);
    if (rc) return 0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < Lg; ++i)
            printf("%.17g\n", nsvd_eig3_eval(kind, param, tab.fn[i].n, tab.fn[i].l, tab.fn[i].m, tab.fn[i].norm,
                                             (double)x[3 * b], (double)x[3 * b + 1], (double)x[3 * b + 2]));
    return 0;
}
