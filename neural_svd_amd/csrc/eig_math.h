// Analytic eigenfunctions of the three 2-D ground truths (reference examples/operator/pde/schrodinger/ground_truths.py:
// Hydrogen2D.eigfunc :134-149, HarmonicOscillator._eigfunc_1d/_2d :96-107, InfiniteWell2D.eigfunc :61-63) in float64,
// for the device (eigfuncs.hip) and for the host (nsvd_eig_table_fill below, tests/_eigfuncs_host). The includer
// provides NSVD_GT_* and NSVD_EINVAL (include/nsvd.h). No scipy.special stands behind any of it:
//   hyp1f1(-k, 2a + 1, z) = k! (2a)! / (k + 2a)! L_k^(2a)(z), the generalised Laguerre polynomial by its three-term
//   recurrence; the factorials are folded into the function's normalisation;
//   Hermite (physicists') by its three-term recurrence;
//   cos(l th), sin(l th) from x / r, y / r by the Chebyshev recurrence (no atan2).
// One function = its two quantum numbers and `norm`, everything in its value that does not depend on the point (the
// host computes it with lgamma, once per call). Loop bounds are quantum numbers: no arrays, nothing indexed at run time.
// Below them, with three quantum numbers and a table of its own: the 3-D hydrogen atom (Hydrogen3D.eigfunc :177-193).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define NSVD_EIG_HD __host__ __device__ __forceinline__
#else
#define NSVD_EIG_HD static inline
#endif

#define NSVD_EIG_MAX_FN 80   // functions per call: the table below travels by value in the launch arguments
#define NSVD_EIG_MAX_Q 16    // hydrogen n, oscillator nx / ny; the well takes 1 .. 2 * NSVD_EIG_MAX_Q
// past these the Gaussian / exponential factor is exactly 0 in float64 (exp(-745) is the last denormal) while the
// polynomial in front of it is still finite: the value is returned as 0 and never formed as inf * 0
#define NSVD_EIG_HYD_TAIL 1500.0   // z = Z r / (n + 1/2): exp(-z / 2)
#define NSVD_EIG_OSC_TAIL 3000.0   // q = b |x|^2: exp(-q / 2)

struct NsvdEigFn {
    int a, b;     // (n, l), (nx, ny), (nx, ny)
    double norm;
};
struct NsvdEigTable {
    NsvdEigFn fn[NSVD_EIG_MAX_FN];
};

static inline double nsvd_eig_lfact(int n) {  // log n!
    int sign;
    return lgamma_r((double)n + 1.0, &sign);
}

// Host: check (kind, param, qnums) and fill fn[0 .. Lg). param: Hydrogen2D's charge Z (psi_Z(x) = Z psi_1(Z x)), the
// oscillator's k (b = sqrt(k)), the well's half-width lim (box [-lim, lim]^2). NSVD_EINVAL: an unknown kind, a
// parameter that is not positive and finite, a quantum number the kind does not admit (hydrogen 0 <= n <=
// NSVD_EIG_MAX_Q, |l| <= n; oscillator 0 <= nx, ny <= NSVD_EIG_MAX_Q; well 1 <= nx, ny <= 2 NSVD_EIG_MAX_Q).
static inline int nsvd_eig_table_fill(int kind, double param, const int* qnums, int Lg, NsvdEigTable* t) {
    if (!qnums || !t || Lg < 1 || Lg > NSVD_EIG_MAX_FN) return NSVD_EINVAL;
    if (!(param > 0.0) || !(param < HUGE_VAL)) return NSVD_EINVAL;
    if (kind != NSVD_GT_HYDROGEN2D && kind != NSVD_GT_HARMONIC2D && kind != NSVD_GT_WELL2D) return NSVD_EINVAL;
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < Lg; ++i) {
        const int a = qnums[2 * i], b = qnums[2 * i + 1];
        double norm;
        if (kind == NSVD_GT_HYDROGEN2D) {
            const int l = b < 0 ? -b : b;
            if (a < 0 || a > NSVD_EIG_MAX_Q || l > a) return NSVD_EINVAL;
            // ground_truths.py:137-141 with hyp1f1's factorials folded in: beta sqrt((n - |l|)! / ((2n + 1) (n + |l|)!))
            norm = param / (a + 0.5) * exp(0.5 * (nsvd_eig_lfact(a - l) - nsvd_eig_lfact(a + l) - log(2.0 * a + 1.0))) /
                   sqrt(l ? pi : 2.0 * pi);
        } else if (kind == NSVD_GT_HARMONIC2D) {
            if (a < 0 || a > NSVD_EIG_MAX_Q || b < 0 || b > NSVD_EIG_MAX_Q) return NSVD_EINVAL;
            norm = sqrt(sqrt(param) / pi) *
                   exp(-0.5 * ((a + b) * 0.69314718055994530942 + nsvd_eig_lfact(a) + nsvd_eig_lfact(b)));
        } else {
            if (a < 1 || a > 2 * NSVD_EIG_MAX_Q || b < 1 || b > 2 * NSVD_EIG_MAX_Q) return NSVD_EINVAL;
            norm = 1.0 / param;  // 2 / L with the side L = 2 lim
        }
        t->fn[i].a = a;
        t->fn[i].b = b;
        t->fn[i].norm = norm;
    }
    return 0;
}

// psi_{n,l}(x, y) of the 2-D hydrogen atom with charge Z. At r = 0: the limit (the reference's formula is 0 * log 0 =
// NaN there for l = 0) - the finite value for l = 0, 0 otherwise. l < 0 keeps the reference's sin(l th), negative l inside.
NSVD_EIG_HD double nsvd_eig_hydrogen2d(double Z, int n, int l, double norm, double x, double y) {
    const int a = l < 0 ? -l : l, k = n - a;
    const double r = sqrt(x * x + y * y);
    const double z = Z * r / (n + 0.5);
    if (z > NSVD_EIG_HYD_TAIL) return 0.0;
    if (a > 0 && r == 0.0) return 0.0;
    double za = 1.0;  // z^|l|
    for (int i = 0; i < a; ++i) za *= z;
    // (j + 1) L_{j+1} = (2j + 1 + alpha - z) L_j - (j + alpha) L_{j-1}, alpha = 2 |l|
    const double alpha = 2.0 * a;
    double lm = 0.0, lc = 1.0;
    for (int j = 0; j < k; ++j) {
        const double ln = ((2.0 * j + 1.0 + alpha - z) * lc - (j + alpha) * lm) / (j + 1.0);
        lm = lc;
        lc = ln;
    }
    double ang = 1.0;
    if (a > 0) {
        const double c = x / r, s = y / r;
        double cm = 1.0, cc = c, sm = 0.0, sc = s;  // cos / sin of (j - 1) th and j th
        for (int j = 1; j < a; ++j) {
            const double cn = 2.0 * c * cc - cm, sn = 2.0 * c * sc - sm;
            cm = cc;
            cc = cn;
            sm = sc;
            sc = sn;
        }
        ang = l > 0 ? cc : -sc;
    }
    return norm * za * exp(-0.5 * z) * lc * ang;
}

// H_n(u): H_0 = 1, H_1 = 2u, H_{j+1} = 2u H_j - 2j H_{j-1}
NSVD_EIG_HD double nsvd_eig_hermite(int n, double u) {
    double hm = 0.0, hc = 1.0;
    for (int j = 0; j < n; ++j) {
        const double hn = 2.0 * u * hc - 2.0 * j * hm;
        hm = hc;
        hc = hn;
    }
    return hc;
}

// psi_{nx,ny}(x, y) of V = k |x|^2 under -lap + V: the reference's b = 1 formula at b = sqrt(k)
NSVD_EIG_HD double nsvd_eig_harmonic2d(double k, int nx, int ny, double norm, double x, double y) {
    const double sb = sqrt(sqrt(k));
    const double u = sb * x, v = sb * y;
    const double q = u * u + v * v;
    if (q > NSVD_EIG_OSC_TAIL) return 0.0;
    return norm * exp(-0.5 * q) * nsvd_eig_hermite(nx, u) * nsvd_eig_hermite(ny, v);
}

// psi_{nx,ny} of the box [-lim, lim]^2: the reference's [0, L] formula at L = 2 lim, shifted; 0 outside the walls
NSVD_EIG_HD double nsvd_eig_well2d(double lim, int nx, int ny, double norm, double x, double y) {
    if (!(fabs(x) <= lim) || !(fabs(y) <= lim)) return 0.0;
    const double pi = 3.14159265358979323846, side = 2.0 * lim;
    return norm * sin(nx * pi * (x + lim) / side) * sin(ny * pi * (y + lim) / side);
}

NSVD_EIG_HD double nsvd_eig_eval(int kind, double param, int a, int b, double norm, double x, double y) {
    if (kind == NSVD_GT_HYDROGEN2D) return nsvd_eig_hydrogen2d(param, a, b, norm, x, y);
    if (kind == NSVD_GT_HARMONIC2D) return nsvd_eig_harmonic2d(param, a, b, norm, x, y);
    return nsvd_eig_well2d(param, a, b, norm, x, y);
}

// ---- three quantum numbers: the 3-D hydrogen atom (ground_truths.py: Hydrogen3D.eigfunc :177-193, real_sph_harm /
// sph_harm :218-270, which the reference defines and never evaluates - its validation grid stops at ndim 2). A table
// and a fill of their own: the 2-D ones above keep their layout and keep refusing every other kind.
struct NsvdEigFn3 {
    int n, l, m;
    double norm;
};
struct NsvdEigTable3 {
    NsvdEigFn3 fn[NSVD_EIG_MAX_FN];
};

// Host: check (kind, param, qnums) and fill fn[0 .. Lg). kind: NSVD_GT_HYDROGEN3D only (the 2-D kinds are
// NSVD_EINVAL here), param the charge Z, qnums (n, l, m) with 1 <= n <= NSVD_EIG_MAX_Q, 0 <= l < n, |m| <= l.
// With a = |m|:  norm = sqrt((Z/n)^3 / (2n)) sqrt((n-l-1)! / (n+l)!) sqrt((2l+1) / (4 pi) (l-a)! / (l+a)!) (2a-1)!!
// times the reference's pairing of the real harmonics: 1 (m = 0), sqrt(2) (m < 0, with cos(a phi)), -sqrt(2) (m > 0,
// with sin(a phi)). (2a-1)!! is P_a^a's leading factor, (2a)! / (2^a a!).
static inline int nsvd_eig3_table_fill(int kind, double param, const int* qnums, int Lg, NsvdEigTable3* t) {
    if (!qnums || !t || Lg < 1 || Lg > NSVD_EIG_MAX_FN) return NSVD_EINVAL;
    if (!(param > 0.0) || !(param < HUGE_VAL)) return NSVD_EINVAL;
    if (kind != NSVD_GT_HYDROGEN3D) return NSVD_EINVAL;
    const double pi = 3.14159265358979323846, ln2 = 0.69314718055994530942;
    for (int i = 0; i < Lg; ++i) {
        const int n = qnums[3 * i], l = qnums[3 * i + 1], m = qnums[3 * i + 2];
        if (n < 1 || n > NSVD_EIG_MAX_Q || l < 0 || l >= n) return NSVD_EINVAL;
        const int a = m < 0 ? -m : m;
        if (a > l) return NSVD_EINVAL;
        const double zn = param / n;
        double norm = sqrt(zn * zn * zn / (2.0 * n) * (2.0 * l + 1.0) / (4.0 * pi)) *
                      exp(0.5 * (nsvd_eig_lfact(n - l - 1) - nsvd_eig_lfact(n + l) + nsvd_eig_lfact(l - a) -
                                 nsvd_eig_lfact(l + a)) +
                          nsvd_eig_lfact(2 * a) - a * ln2 - nsvd_eig_lfact(a));
        if (m) norm *= m < 0 ? 1.41421356237309504880 : -1.41421356237309504880;
        t->fn[i].n = n;
        t->fn[i].l = l;
        t->fn[i].m = m;
        t->fn[i].norm = norm;
    }
    return 0;
}

// psi_{n,l,m}(x, y, z) of -lap - Z / r, rho = Z r / n, a = |m|:
//   norm rho^l exp(-rho / 2) L_{n-l-1}^(2l+1)(rho) P_l^a(z / r) {1, cos(a phi), sin(a phi)}
// P_l^a WITHOUT the Condon-Shortley phase (the reference's lpmv carries it and real_sph_harm's sign takes it out again):
// P_a^a = (2a-1)!! st^a, the double factorial in norm, then (j - a + 1) P_{j+1} = (2j + 1) ct P_j - (j + a) P_{j-1}.
// cos / sin of a phi by the Chebyshev recurrence on x / s, y / s, s = sqrt(x^2 + y^2); on the z axis phi = 0
// (arctan2(0, 0)). At r = 0 (theta = arctan2(0, 0) = 0): the finite value for l = 0, exactly 0 otherwise.
NSVD_EIG_HD double nsvd_eig_hydrogen3d(double Z, int n, int l, int m, double norm, double x, double y, double z) {
    const int a = m < 0 ? -m : m;
    const double s = sqrt(x * x + y * y);
    const double r = sqrt(x * x + y * y + z * z);
    const double rho = Z * r / n;
    if (rho > NSVD_EIG_HYD_TAIL) return 0.0;
    if (l > 0 && r == 0.0) return 0.0;
    double ct = 1.0, st = 0.0, c = 1.0, sn = 0.0;
    if (r > 0.0) {
        ct = z / r;
        st = s / r;
    }
    if (s > 0.0) {
        c = x / s;
        sn = y / s;
    }
    double rl = 1.0;  // rho^l
    for (int i = 0; i < l; ++i) rl *= rho;
    // (j + 1) L_{j+1} = (2j + 1 + alpha - rho) L_j - (j + alpha) L_{j-1}, alpha = 2l + 1
    const double alpha = 2.0 * l + 1.0;
    double lm = 0.0, lc = 1.0;
    for (int j = 0; j < n - l - 1; ++j) {
        const double ln = ((2.0 * j + 1.0 + alpha - rho) * lc - (j + alpha) * lm) / (j + 1.0);
        lm = lc;
        lc = ln;
    }
    double pm = 0.0, pc = 1.0;  // P_{j-1}^a, P_j^a from j = a
    for (int i = 0; i < a; ++i) pc *= st;
    for (int j = a; j < l; ++j) {
        const double pn = ((2.0 * j + 1.0) * ct * pc - (double)(j + a) * pm) / (double)(j - a + 1);
        pm = pc;
        pc = pn;
    }
    double ang = 1.0;
    if (a > 0) {
        double cm = 1.0, cc = c, sm = 0.0, sc = sn;  // cos / sin of (j - 1) phi and j phi
        for (int j = 1; j < a; ++j) {
            const double cn = 2.0 * c * cc - cm, sq = 2.0 * c * sc - sm;
            cm = cc;
            cc = cn;
            sm = sc;
            sc = sq;
        }
        ang = m < 0 ? cc : sc;  // (the signs and sqrt(2) are in norm)
    }
    return norm * rl * exp(-0.5 * rho) * lc * pc * ang;
}

NSVD_EIG_HD double nsvd_eig3_eval(int kind, double param, int n, int l, int m, double norm, double x, double y,
                                  double z) {
    (void)kind;  // NSVD_GT_HYDROGEN3D: the only kind nsvd_eig3_table_fill admits
    return nsvd_eig_hydrogen3d(param, n, l, m, norm, x, y, z);
}
