// Host program around csrc/eig_math.h: the per-function device math of eigfuncs.hip and the host-side table
// (validation, lgamma normalisations) compiled for the CPU, so that tests/test_eigfunc_oracle.py can run them under
// -fsanitize=address,undefined and hold them to the golden values.
//   stdin:  kind param Lg B, then Lg pairs of quantum numbers, then B pairs of float32 coordinates (%.9g round-trips)
//   stdout: the return code of nsvd_eig_table_fill, then (code 0) B * Lg values row-major, %.17g
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "nsvd.h"
#include "eig_math.h"

int main() {
    int kind, Lg, B;
    double param;
    if (scanf("%d %lf %d %d", &kind, &param, &Lg, &B) != 4 || Lg < 0 || Lg > 4096 || B < 0) return 2;
    std::vector<int> q(2 * (size_t)Lg);
    for (int& v : q)
        if (scanf("%d", &v) != 1) return 2;
    std::vector<float> x(2 * (size_t)B);
    for (float& v : x)
        if (scanf("%f", &v) != 1) return 2;
    NsvdEigTable tab = {};
    const int rc = nsvd_eig_table_fill(kind, param, q.data(), Lg, &tab);
    printf("%d\n", rc);
    if (rc) return 0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < Lg; ++i)
            printf("%.17g\n", nsvd_eig_eval(kind, param, tab.fn[i].a, tab.fn[i].b, tab.fn[i].norm, (double)x[2 * b],
                                            (double)x[2 * b + 1]));
    return 0;
}
