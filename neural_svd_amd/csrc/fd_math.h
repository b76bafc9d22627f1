// Per-(sample, head) math of the importance-weighted finite-difference Hamiltonian, shared by the
// generic epilogue kernel and the fused MFMA kernel's epilogue so both paths are the same arithmetic.
#pragma once
#include "nsvd_common.h"

#define NSVD_FD_MAXD 4
#ifdef NSVD_SMALL_D
static_assert(NSVD_FD_MAXD == NSVD_SMALL_D, "nsvd_problem_status routes D > NSVD_SMALL_D to the direction-loop form");
#endif

struct NsvdFdOut {
    float f, Tf, jac, dsc;
};

// sqrt p(x) of the problem's importance density: Gaussian (log_norm = nsvd_gauss_log_norm), uniform (a constant,
// log_norm = log p = -D log(2 sigma): main_pde.py:116-118) or none; host: nsvd_importance_log_norm
__device__ __forceinline__ float nsvd_sqrt_p(const nsvd_problem& prob, const float* xr, int D, float log_norm) {
    if (prob.use_importance == NSVD_IMP_GAUSSIAN) return nsvd_sqrt_gauss_pdf(xr, D, prob.sigma, log_norm);
    if (prob.use_importance == NSVD_IMP_UNIFORM) return sqrtf(expf(log_norm));
    return 1.f;
}
static inline float nsvd_importance_log_norm(int D, const nsvd_problem& prob) {
    // (the exponent of the uniform density is the SPACE dimension D / n_particles: main_pde.py:118)
    if (prob.use_importance == NSVD_IMP_UNIFORM)
        return (float)(-(double)(prob.n_particles > 1 ? D / prob.n_particles : D) * log(2.0 * (double)prob.sigma));
    return nsvd_gauss_log_norm(D, prob.sigma);
}

// pot_coef[d] by a chain of selects on the uniform d: constant indices only, so the by-value nsvd_problem of the
// kernel arguments is read where it lies (scalar registers) and never copied into a per-thread array
__device__ __forceinline__ float nsvd_pot_coef(const nsvd_problem& prob, int d) {
    return d == 0 ? prob.pot_coef[0] : d == 1 ? prob.pot_coef[1] : d == 2 ? prob.pot_coef[2] : prob.pot_coef[3];
}
// S(x) = sum_d cs[d] cos x_d: the cosine potential (potentials.py:30-31) and the argument of sin-of-cos (others.py:33-34)
__device__ __forceinline__ float nsvd_cos_sum(const nsvd_problem& prob, const float* xc, int D) {
    float S = 0.f;
    for (int d = 0; d < D; ++d) S = fmaf(nsvd_pot_coef(prob, d), cosf(xc[d]), S);
    return S;
}

// ---- the many-electron potential (potentials.py:35-57): x holds n_particles electrons of sd = D / n_particles
// coordinates each, pot_table n_nuclei rows (R_0, .., R_{sd-1}, Z):
//   V = pot_const - sum_i sum_a Z_a / |r_i - R_a| + sum_{i<j} 1 / |r_i - r_j|
// Every distance from coordinate DIFFERENCES (exact beside a nucleus and at a coalescence: Sterbenz), never from
// expanded squares. X: coordinate k of the row - a chain of selects over a register array (NsvdCoordArr: constant
// indices only, D <= NSVD_FD_MAXD) or a load (NsvdCoordMem); the table is read with uniform indices from global memory.
struct NsvdCoordArr {
    float x0, x1, x2, x3;
    __device__ __forceinline__ float operator()(int k) const { return k == 0 ? x0 : k == 1 ? x1 : k == 2 ? x2 : x3; }
};
struct NsvdCoordMem {
    const float* xr;
    __device__ __forceinline__ float operator()(int k) const { return xr[k]; }
};
template <class X>
__device__ __forceinline__ float nsvd_molecule_potential(const nsvd_problem& prob, X x, int D) {
    const int np = prob.n_particles > 0 ? prob.n_particles : 1, sd = D / np;
    const bool three = sd > 2;
    const float* tab = prob.pot_table;
    float V = prob.pot_const;
    for (int i = 0; i < np; ++i) {
        const float x0 = x(i * sd), x1 = x(i * sd + 1), x2 = three ? x(i * sd + 2) : 0.f;
        for (int a = 0; a < prob.n_nuclei; ++a) {
            const float* row = tab + a * (sd + 1);
            const float d0 = x0 - row[0], d1 = x1 - row[1], d2 = three ? x2 - row[2] : 0.f;
            V -= row[sd] / sqrtf(fmaf(d2, d2, fmaf(d1, d1, d0 * d0)));
        }
        for (int j = i + 1; j < np; ++j) {
            const float d0 = x0 - x(j * sd), d1 = x1 - x(j * sd + 1), d2 = three ? x2 - x(j * sd + 2) : 0.f;
            V += 1.f / sqrtf(fmaf(d2, d2, fmaf(d1, d1, d0 * d0)));
        }
    }
    return V;
}

// V(x) of the Schroedinger kind at the centre xc, |xc| = r0 (potentials.py:5-8, 11-17, 20-21, 24-27, 30-31)
// TRIG (here and in the finite-difference forms below): false compiles the periodic problems - the cosine potential
// and the Fokker-Planck kind, whose sinf / cosf carry their own argument reduction - out of an instance; a kernel that
// has such an instance (fd_epilogue.hip) keeps the registers and occupancy of its other problems.
template <bool TRIG = true>
__device__ __forceinline__ float nsvd_potential(const nsvd_problem& prob, const float* xc, int D, float r0) {
    if (prob.potential == NSVD_POT_HYDROGEN) return -(prob.charge_or_k / r0);
    if (prob.potential == NSVD_POT_ZERO) return 0.f;
    if (TRIG && prob.potential == NSVD_POT_COSINE) return nsvd_cos_sum(prob, xc, D);
    if (prob.potential == NSVD_POT_MOLECULE) {
        // (a molecule has at least two coordinates; entries past D are never selected)
        const NsvdCoordArr xa{xc[0], xc[1], D > 2 ? xc[2] : 0.f, D > 3 ? xc[3] : 0.f};
        return nsvd_molecule_potential(prob, xa, D);
    }
    if (prob.potential == NSVD_POT_H2_ION) {
        // the nuclei sit at +-R on the last axis; x_last -+ R is exact next to a nucleus (Sterbenz), where
        // |x|^2 -+ 2 R x_last + R^2 would be a difference of O(1) numbers
        const float R = prob.pot_coef[0];
        float rest = 0.f, xl = 0.f;
        for (int d = 0; d < D; ++d) {
            const bool last = d == D - 1;
            rest = last ? rest : fmaf(xc[d], xc[d], rest);
            xl = last ? xc[d] : xl;
        }
        const float dm = xl - R, dp = xl + R;
        return -(prob.charge_or_k / sqrtf(fmaf(dm, dm, rest))) - prob.charge_or_k / sqrtf(fmaf(dp, dp, rest));
    }
    return prob.charge_or_k * (r0 * r0);
}

// ---- Fokker-Planck kind (others.py:6-30): Tf = fp_scale (Lap f + grad V . grad f + f Lap V), V = sin S ---------------
// The reference differences V with the stencil it uses for f. Along direction d, S(x +- eps e_d) = S + a -+ b with
//   a = cs_d (cos x_d cos eps - cos x_d) = -2 cs_d cos x_d sin^2(eps / 2),   b = cs_d sin x_d sin eps
// and the differences of sin follow without subtracting two O(1) numbers:
//   V_+ - V_-       = sin(S + a - b) - sin(S + a + b) = -2 cos(S + a) sin b
//   V_+ + V_- - 2 V = 2 sin(S + a) cos b - 2 sin S    = 4 cos(S + a / 2) sin(a / 2) cos b - 4 sin S sin^2(b / 2)
struct NsvdPotDiff {
    float dif, sum2;  // V_+ - V_-,  V_+ + V_- - 2 V_0
};
__device__ __forceinline__ NsvdPotDiff nsvd_sin_of_cos_diff_cs(float cs, float eps, float S, float xd) {
    const float she = sinf(0.5f * eps);
    const float a = -2.f * cs * cosf(xd) * (she * she), b = cs * sinf(xd) * sinf(eps);
    const float shb = sinf(0.5f * b);
    NsvdPotDiff o;
    o.dif = -2.f * cosf(S + a) * sinf(b);
    o.sum2 = 4.f * cosf(S + 0.5f * a) * sinf(0.5f * a) * cosf(b) - 4.f * sinf(S) * (shb * shb);
    return o;
}
__device__ __forceinline__ NsvdPotDiff nsvd_sin_of_cos_diff(const nsvd_problem& prob, float S, float xd, int d) {
    return nsvd_sin_of_cos_diff_cs(nsvd_pot_coef(prob, d), prob.eps, S, xd);
}
// from the per-direction sums adv = sum_d (V_+ - V_-)(g_+ - g_-) / u and lv = sum_d (V_+ + V_- - 2 V), with
// lap = Lap g / sqrt p and fs as the Schroedinger kind forms them, u the factor adv still lacks (c w0 / sqrt p):
//   grad V . grad f = u adv / (2 eps)^2,   Lap V = lv / eps^2
__device__ __forceinline__ float nsvd_fp_apply(const nsvd_problem& prob, float lap, float fs, float u, float adv,
                                               float lv, float eps2) {
    return prob.fp_scale * (lap + u * adv / (4.f * eps2) + fs * (lv / eps2));
}

// ---- Dirichlet box mask (boundary.py:16-36): M(x) = prod_d m(clamp(x_d, -lim, lim)) --------------------------------
// Everything is written in the distances to the two walls a = lim - t, b = lim + t (a b = lim^2 - t^2): a is exact in
// float32 near the right wall, b near the left one (Sterbenz), and the shifted points take a -+ eps, b +- eps - so the
// mask near a wall, where it is ~ eps / lim, keeps its relative accuracy. At and beyond the wall m = 0 exactly.
//   sqrt: m = (sqrt(lim^2 + a b) - lim) / lim = a b / (lim (sqrt(lim^2 + a b) + lim))     (no difference of O(lim) numbers)
//   exp:  m = (1 - e^-a)(1 - e^-b) = expm1(-a) expm1(-b)
__device__ __forceinline__ float nsvd_box_m1(float a, float b, const NsvdBox& bx) {
    if (!(a > 0.f) || !(b > 0.f)) return 0.f;
    if (bx.mode == NSVD_BOX_SQRT) {
        const float ab = a * b;
        return ab / (bx.lim * (sqrtf(fmaf(bx.lim, bx.lim, ab)) + bx.lim));
    }
    return expm1f(-a) * expm1f(-b);
}
// M at stencil point e of the row xc
__device__ __forceinline__ float nsvd_box_point(const float* xc, int D, int e, float eps, const NsvdBox& bx) {
    float M = 1.f;
    for (int d = 0; d < D; ++d) {
        float a = bx.lim - xc[d], b = bx.lim + xc[d];
        if (e > 0 && ((e - 1) >> 1) == d) {
            const float sh = ((e - 1) & 1) ? -eps : eps;
            a -= sh;
            b += sh;
        }
        M *= nsvd_box_m1(a, b, bx);
    }
    return M;
}
// Along one direction: m0 = m(x_d) and delta_+- = m(x_d +- eps) - m0 as their sum ds (O(eps^2) inside the box) and
// difference dd, neither formed by subtracting two O(1) numbers. With bb = 2 x_d eps, e2 = eps^2:
//   sqrt: A = lim^2 + a b, A_+- = A - (e2 +- bb), sqrt(A_+-) - sqrt(A) = -(e2 +- bb) / (s_+- + s0)  (the tsum / tdif algebra):
//         ds = -[e2 (S + 2 s0) + 2 bb^2 / S] / (lim den),  dd = -bb [(S + 2 s0) + 2 e2 / S] / (lim den),
//         S = s_+ + s_-, den = (s_+ + s0)(s_- + s0)
//   exp:  m = 1 + e^-2lim - 2 e^-lim cosh t:  ds = -8 e^-lim cosh x sinh^2(eps / 2),  dd = -4 e^-lim sinh x sinh eps,
//         e^-lim cosh x = (e^-a + e^-b) / 2, e^-lim sinh x = (e^-a - e^-b) / 2
// A stencil point at or beyond the wall has m = 0 exactly (delta = -m0), a centre outside m0 = 0 with its inner
// neighbour still counting: the kink makes that row's Laplacian O(1 / eps), not a small difference, so the point-wise
// deltas are exact enough there - and they are what the reference computes.
struct NsvdBoxEO {
    float m0, ds, dd;
};
__device__ __forceinline__ NsvdBoxEO nsvd_box_eo(float xd, float eps, const NsvdBox& bx) {
    const float lim = bx.lim, a = lim - xd, b = lim + xd;
    NsvdBoxEO o;
    o.m0 = nsvd_box_m1(a, b, bx);
    const bool smooth = a > 0.f && b > 0.f && (a - eps) > 0.f && (b - eps) > 0.f;
    if (!smooth) {
        const float dp = nsvd_box_m1(a - eps, b + eps, bx) - o.m0, dm = nsvd_box_m1(a + eps, b - eps, bx) - o.m0;
        o.ds = dp + dm;
        o.dd = dp - dm;
    } else if (bx.mode == NSVD_BOX_SQRT) {
        const float e2 = eps * eps, bb = 2.f * xd * eps;
        const float A0 = fmaf(lim, lim, a * b);
        const float s0 = sqrtf(A0), sp = sqrtf(A0 - (e2 + bb)), sm = sqrtf(A0 - (e2 - bb));
        const float S = sp + sm, den = lim * ((sp + s0) * (sm + s0));
        o.ds = -(e2 * (S + 2.f * s0) + 2.f * bb * bb / S) / den;
        o.dd = -bb * ((S + 2.f * s0) + 2.f * e2 / S) / den;
    } else {
        const float ea = expf(-a), eb = expf(-b);
        const float sh = sinhf(0.5f * eps);
        o.ds = -4.f * (ea + eb) * sh * sh;
        o.dd = -2.f * (ea - eb) * sinhf(eps);
    }
    return o;
}

// bv[e]: raw head output base_l(x_e) at the stencil points (e = 0 centre, 1+2i: +eps e_i, 2+2i: -eps e_i)
// xc: centre coordinates. Follows the reference's operation order:
//   g_e   = sqrt(p(x_e)) * (c * base_e * mask_l(x_e))          pde/__init__.py:16, diff_ops.py:13
//   lap_g = (-2 D g_0 + sum_i (g_+i + g_-i)) / eps^2           diff_ops.py:38-48
//   lap   = lap_g / clamp(sqrt p(x_0), 1e-5),  fs = g_0 / clamp(...)   diff_ops.py:15-18
//   Tf    = scale * -( -c_k lap + V(x) fs ) + shift * fs       schrodinger/__init__.py:18-22, examples/__init__.py:9
// one stencil point: g_e and (needed of the centre only) sqrt p, mask, |x|
struct NsvdFdG {
    float g, sp, mk, r;
};
__device__ __forceinline__ NsvdFdG nsvd_fd_g(int e, float bve, const float* xc, int D, bool has_mask, float s_l,
                                             const nsvd_problem& prob, float log_norm, const NsvdBox& box) {
    float xe[NSVD_FD_MAXD];
    float r2 = 0.f;
    for (int d = 0; d < D; ++d) {
        xe[d] = nsvd_stencil_coord(xc[d], d, e, prob.eps);
        r2 = fmaf(xe[d], xe[d], r2);
    }
    NsvdFdG o;
    o.sp = nsvd_sqrt_p(prob, xe, D, log_norm);
    float model = prob.hard_mul_const * bve;
    o.mk = 1.f;
    o.r = sqrtf(r2);
    if (has_mask) {
        o.mk = expf(-o.r / s_l);
        model *= o.mk;
    }
    if (box.mode) model *= nsvd_box_point(xc, D, e, prob.eps, box);
    o.g = o.sp * model;
    return o;
}

// stencil combination; g[e] from nsvd_fd_g, (sp0, mask0, r0) of the centre point, bv0 = bv[0]
// (M0: the box mask at the centre, 1 without one)
// (xc: the centre coordinates, for the potentials that are no function of r0)
template <bool TRIG = true>
__device__ __forceinline__ NsvdFdOut nsvd_fd_combine(const float* g, float sp0, float mask0, float r0, float bv0, int D,
                                                     bool has_mask, float s_l, const nsvd_problem& prob, float M0,
                                                     const float* xc) {
    float lap = -2.f * (float)D * g[0];
    for (int i = 0; i < D; ++i) lap += (g[1 + 2 * i] + g[2 + 2 * i]);
    const float eps2 = (float)((double)prob.eps * (double)prob.eps);
    lap = lap / eps2;
    const float spc = prob.use_importance ? fmaxf(sp0, NSVD_SQRT_P_CLAMP) : 1.f;
    lap = lap / spc;
    const float fs = g[0] / spc;
    NsvdFdOut o;
    o.f = fs;
    if (TRIG && prob.operator_kind == NSVD_OP_FOKKER_PLANCK) {
        const float S = nsvd_cos_sum(prob, xc, D);
        float adv = 0.f, lv = 0.f;
        for (int i = 0; i < D; ++i) {
            const NsvdPotDiff v = nsvd_sin_of_cos_diff(prob, S, xc[i], i);
            adv = fmaf(v.dif, g[1 + 2 * i] - g[2 + 2 * i], adv);
            lv += v.sum2;
        }
        o.Tf = prob.op_scale * nsvd_fp_apply(prob, lap, fs, 1.f / spc, adv, lv, eps2) + prob.op_shift * fs;
    } else {
        const float V = nsvd_potential<TRIG>(prob, xc, D, r0);
        const float kinetic = -prob.scale_kinetic * lap;
        const float H = kinetic + V * fs;
        o.Tf = prob.op_scale * (-H) + prob.op_shift * fs;
    }
    const float w = (sp0 / spc) * prob.hard_mul_const;
    o.jac = w * mask0 * M0;
    o.dsc = has_mask ? w * bv0 * mask0 * r0 / (s_l * s_l) * M0 : 0.f;
    return o;
}

// The same central difference with the stencil points given in EVEN / ODD form (the bf16x3 forward propagates
// perturbations, pmlp_layer0_bf3.h): along direction d the head's raw output is base(x +- eps e_d) = base0 + bE[d] +- bO[d],
// and the weight w(x) = sqrt p(x) mask_l(x) at the shifted point is w0 (1 + rho_+-), rho = expm1(log w(x_+-) - log w(x0))
// with |x_+-|^2 - |x0|^2 = eps (+-2 x_d + eps) formed exactly:
//     g_+ + g_- - 2 g_0 = c w0 [ (rho_+ + rho_-)(base0 + bE) + 2 bE + (rho_+ - rho_-) bO ]
// - every term small, none the difference of two large numbers: the float32 result carries the Laplacian to ~1e-6 where
// the point-wise form (nsvd_fd_combine, the reference's own float32 arithmetic) carries it to a few per cent.
// With a box mask the weight at x +- eps e_d is w0 (1 + rho_+-) M_rest (m0 + delta_+-) - along d only m(x_d) changes,
// M_rest = prod_{j != d} m(x_j) - and (1 + rho)(m0 + delta) = m0 + sigma, sigma = m0 rho + delta + rho delta:
//     g_+ + g_- - 2 g_0 = c w0 M_rest [ (sigma_+ + sigma_-)(base0 + bE) + 2 m0 bE + (sigma_+ - sigma_-) bO ]
// with sigma_+ +- sigma_- from the even / odd parts of rho (ev, od) and of delta (nsvd_box_eo: ds, dd):
//     rho_+ delta_+ +- rho_- delta_- = (ev ds + od dd) / 2, (ev dd + od ds) / 2
// The Fokker-Planck kind (no box mask) also needs the first difference, the odd part of the same expansion:
//     g_+ - g_- = c w0 [ od (base0 + bE) + (2 + ev) bO ]
template <bool TRIG = true>
__device__ __forceinline__ NsvdFdOut nsvd_fd_evenodd(float base0, const float* bE, const float* bO, const float* xc,
                                                     int D, bool has_mask, float s_l, const nsvd_problem& prob,
                                                     float log_norm, const NsvdBox& box) {
    float r2 = 0.f;
    for (int d = 0; d < D; ++d) r2 = fmaf(xc[d], xc[d], r2);
    const float r0 = sqrtf(r2);
    const float c = prob.hard_mul_const;
    const float sp0 = nsvd_sqrt_p(prob, xc, D, log_norm);
    const float mk0 = has_mask ? expf(-r0 / s_l) : 1.f;
    const float eps = prob.eps;
    // d log sqrt p / d |x|^2 (the uniform density is a constant)
    const float qs = prob.use_importance == NSVD_IMP_GAUSSIAN ? -1.f / (4.f * prob.sigma * prob.sigma) : 0.f;
    const float e2 = eps * eps;
    float acc = 0.f;
    const bool fp = TRIG && prob.operator_kind == NSVD_OP_FOKKER_PLANCK;
    const float S = fp ? nsvd_cos_sum(prob, xc, D) : 0.f;
    float adv = 0.f, lv = 0.f;
    // (no per-direction arrays for the box mask: indexed by a run-time d they would live in scratch memory, in every
    // instance of the fused forward, the headline's included - M_rest is recomputed from xc instead)
    float M0 = 1.f;
    if (box.mode)
        for (int d = 0; d < D; ++d) M0 *= nsvd_box_m1(box.lim - xc[d], box.lim + xc[d], box);
    for (int d = 0; d < D; ++d) {
        // log w(x_+-) - log w(x0) = s +- a, split into its even part s = O(eps^2) and odd part a = O(eps) BEFORE any
        // exponential: rho_+ + rho_- is O(eps^2) while each rho is O(eps), so expm1(s + a) + expm1(s - a) loses
        // |x_d| / eps ~ 10^3 of its digits (measured: 7e-5 relative at the median of a [-50, 50] grid, i.e. the whole
        // Laplacian term); with |x_+-|^2 - |x0|^2 = e2 +- b, b = 2 x_d eps:
        //     rho_+ + rho_- = 2 [expm1(s) cosh a + (cosh a - 1)],  cosh a - 1 = 2 sinh^2(a / 2)
        //     rho_+ - rho_- = 2 exp(s) sinh a
        const float b = 2.f * xc[d] * eps;
        float sv = qs * e2, av = qs * b;
        if (has_mask) {
            // |x_+-| - |x0| = (e2 +- b) / (r_+- + r0) =: t_+-, with r_- - r_+ = -2 b / (r_+ + r_-):
            //   t_+ + t_- = [e2 (S + 2 r0) - 2 b^2 / S] / den,  t_+ - t_- = b [(S + 2 r0) - 2 e2 / S] / den,
            //   S = r_+ + r_-, den = (r_+ + r0)(r_- + r0)
            const float rp = sqrtf(fmaxf(r2 + (e2 + b), 0.f)), rm = sqrtf(fmaxf(r2 + (e2 - b), 0.f));
            const float S = rp + rm, den = (rp + r0) * (rm + r0);
            const float tsum = (e2 * (S + 2.f * r0) - 2.f * b * b / S) / den;
            const float tdif = b * ((S + 2.f * r0) - 2.f * e2 / S) / den;
            sv -= 0.5f * tsum / s_l;
            av -= 0.5f * tdif / s_l;
        }
        const float sh = sinhf(0.5f * av), chm1 = 2.f * sh * sh, es1 = expm1f(sv);
        const float ev = 2.f * (es1 * (1.f + chm1) + chm1);  // rho_+ + rho_-
        const float od = 2.f * (1.f + es1) * sinhf(av);      // rho_+ - rho_-
        if (box.mode) {
            float Mrest = 1.f;
            for (int j = 0; j < D; ++j)
                if (j != d) Mrest *= nsvd_box_m1(box.lim - xc[j], box.lim + xc[j], box);
            const NsvdBoxEO bm = nsvd_box_eo(xc[d], eps, box);
            const float m0 = bm.m0, ds = bm.ds, dd = bm.dd;
            const float sgs = m0 * ev + ds + 0.5f * (ev * ds + od * dd);  // sigma_+ + sigma_-
            const float sgd = m0 * od + dd + 0.5f * (ev * dd + od * ds);  // sigma_+ - sigma_-
            acc += Mrest * (sgs * (base0 + bE[d]) + 2.f * m0 * bE[d] + sgd * bO[d]);
        } else {
            acc += ev * (base0 + bE[d]) + 2.f * bE[d] + od * bO[d];
            if (fp) {
                const NsvdPotDiff v = nsvd_sin_of_cos_diff(prob, S, xc[d], d);
                adv = fmaf(v.dif, od * (base0 + bE[d]) + (2.f + ev) * bO[d], adv);
                lv += v.sum2;
            }
        }
    }
    const float eps2 = (float)((double)prob.eps * (double)prob.eps);
    const float spc = prob.use_importance ? fmaxf(sp0, NSVD_SQRT_P_CLAMP) : 1.f;
    const float lap = ((c * (sp0 * mk0)) * acc / eps2) / spc;
    const float fs = (sp0 * (c * base0 * (mk0 * M0))) / spc;
    NsvdFdOut o;
    o.f = fs;
    if (fp) {
        o.Tf = prob.op_scale * nsvd_fp_apply(prob, lap, fs, (c * (sp0 * mk0)) / spc, adv, lv, eps2) + prob.op_shift * fs;
    } else {
        const float V = nsvd_potential<TRIG>(prob, xc, D, r0);
        const float H = -prob.scale_kinetic * lap + V * fs;
        o.Tf = prob.op_scale * (-H) + prob.op_shift * fs;
    }
    const float w = (sp0 / spc) * c;
    o.jac = w * (mk0 * M0);
    o.dsc = has_mask ? w * base0 * (mk0 * M0) * r0 / (s_l * s_l) : 0.f;
    return o;
}

// ---- the even / odd form for 5 <= D <= NSVD_MAX_D: a loop over directions that reads xr[d], bE[d], bO[d] from MEMORY --------
// nsvd_fd_evenodd's expressions, term for term; no per-thread array indexed by a run-time d exists (a 12-entry one would
// live in scratch memory). xr: the row's D coordinates; the head's raw outputs are base0 = bcol[0], bE[d] =
// bcol[(1 + 2 d) bs], bO[d] = bcol[(2 + 2 d) bs] (bs = B in the (L, E B) layout of the generic path). The cosine /
// sin-of-cos coefficients come from prob.pot_table (D floats).
// What a row's L heads share is computed once: per row (nsvd_fd_row_nd) |x|, sqrt p, the potential, the box mask at the
// centre; per row and direction (nsvd_fd_dir_nd) everything of the loop body that does not depend on the head.
struct NsvdFdRowNd {
    float r2, r0, sp0, V, M0, S;  // S: the cosine sum of the Fokker-Planck drift potential
};
template <bool TRIG>
__device__ __forceinline__ NsvdFdRowNd nsvd_fd_row_nd(const float* xr, int D, const nsvd_problem& prob, float log_norm,
                                                      const NsvdBox& box) {
    NsvdFdRowNd w;
    float r2 = 0.f;
    for (int d = 0; d < D; ++d) r2 = fmaf(xr[d], xr[d], r2);
    w.r2 = r2;
    w.r0 = sqrtf(r2);
    w.sp0 = nsvd_sqrt_p(prob, xr, D, log_norm);
    w.M0 = 1.f;
    if (box.mode)
        for (int d = 0; d < D; ++d) w.M0 *= nsvd_box_m1(box.lim - xr[d], box.lim + xr[d], box);
    float S = 0.f;
    if (TRIG && (prob.potential == NSVD_POT_COSINE || prob.potential == NSVD_POT_SIN_OF_COS))
        for (int d = 0; d < D; ++d) S = fmaf(prob.pot_table[d], cosf(xr[d]), S);
    w.S = S;
    w.V = 0.f;
    if (prob.operator_kind != NSVD_OP_FOKKER_PLANCK) {
        if (prob.potential == NSVD_POT_HYDROGEN) w.V = -(prob.charge_or_k / w.r0);
        else if (prob.potential == NSVD_POT_ZERO) w.V = 0.f;
        else if (prob.potential == NSVD_POT_COSINE) w.V = S;
        else if (prob.potential == NSVD_POT_MOLECULE) w.V = nsvd_molecule_potential(prob, NsvdCoordMem{xr}, D);
        else if (prob.potential == NSVD_POT_H2_ION) {
            const float R = prob.pot_coef[0], xl = xr[D - 1];
            float rest = 0.f;
            for (int d = 0; d < D - 1; ++d) rest = fmaf(xr[d], xr[d], rest);
            const float dm = xl - R, dp = xl + R;
            w.V = -(prob.charge_or_k / sqrtf(fmaf(dm, dm, rest))) - prob.charge_or_k / sqrtf(fmaf(dp, dp, rest));
        } else w.V = prob.charge_or_k * (w.r0 * w.r0);
    }
    return w;
}
// What the L heads of a row share along direction d (nsvd_fd_dir_nd), NSVD_FD_DIR_FIELDS floats: field k of direction d
// lies at dir[(d NSVD_FD_DIR_FIELDS + k) es] - es = 1: one row's table, contiguous; the kernel keeps the table of its
// 64 rows in LDS with the row fastest (es = 64). Without the exponential mask rho's even / odd parts (ev, od: two
// sinhf and one expm1f) do not depend on the head; nor do the box mask's M_rest, m0, ds, dd (O(D) mask values per
// direction) and the Fokker-Planck differences of V (six sinf / cosf). With the mask ev / od depend on scales_l and
// stay in the head's loop.
// (the Fokker-Planck kind has no box mask: its two values share the slots of M_rest and m0)
#define NSVD_FD_DIR_FIELDS 6
enum { NSVD_DIR_EV = 0, NSVD_DIR_OD, NSVD_DIR_MREST, NSVD_DIR_M0, NSVD_DIR_DS, NSVD_DIR_DD,
       NSVD_DIR_VDIF = NSVD_DIR_MREST, NSVD_DIR_VSUM2 = NSVD_DIR_M0 };
template <bool TRIG>
__device__ __forceinline__ void nsvd_fd_dir_nd(const NsvdFdRowNd& w, const float* xr, int d, int D, bool has_mask,
                                               const nsvd_problem& prob, const NsvdBox& box, float* dir, size_t es) {
    const float xd = xr[d], eps = prob.eps;
    float* q = dir + (size_t)d * NSVD_FD_DIR_FIELDS * es;
    if (!has_mask) {
        const float qs = prob.use_importance == NSVD_IMP_GAUSSIAN ? -1.f / (4.f * prob.sigma * prob.sigma) : 0.f;
        const float e2 = eps * eps, b = 2.f * xd * eps;
        const float sv = qs * e2, av = qs * b;
        const float sh = sinhf(0.5f * av), chm1 = 2.f * sh * sh, es1 = expm1f(sv);
        q[NSVD_DIR_EV * es] = 2.f * (es1 * (1.f + chm1) + chm1);
        q[NSVD_DIR_OD * es] = 2.f * (1.f + es1) * sinhf(av);
    }
    if (box.mode) {
        float Mrest = 1.f;
        for (int j = 0; j < D; ++j)
            if (j != d) Mrest *= nsvd_box_m1(box.lim - xr[j], box.lim + xr[j], box);
        const NsvdBoxEO bm = nsvd_box_eo(xd, eps, box);
        q[NSVD_DIR_MREST * es] = Mrest;
        q[NSVD_DIR_M0 * es] = bm.m0;
        q[NSVD_DIR_DS * es] = bm.ds;
        q[NSVD_DIR_DD * es] = bm.dd;
    } else if (TRIG && prob.operator_kind == NSVD_OP_FOKKER_PLANCK) {
        const NsvdPotDiff v = nsvd_sin_of_cos_diff_cs(prob.pot_table[d], eps, w.S, xd);
        q[NSVD_DIR_VDIF * es] = v.dif;
        q[NSVD_DIR_VSUM2 * es] = v.sum2;
    }
}
template <bool TRIG>
__device__ __forceinline__ NsvdFdOut nsvd_fd_evenodd_nd(const NsvdFdRowNd& w, const float* xr, const float* bcol,
                                                        size_t bs, int D, bool has_mask, float s_l,
                                                        const nsvd_problem& prob, const NsvdBox& box,
                                                        const float* dir, size_t es) {
    const float r2 = w.r2, r0 = w.r0, sp0 = w.sp0;
    const float base0 = bcol[0];
    const float c = prob.hard_mul_const;
    const float mk0 = has_mask ? expf(-r0 / s_l) : 1.f;
    const float eps = prob.eps;
    const float qs = prob.use_importance == NSVD_IMP_GAUSSIAN ? -1.f / (4.f * prob.sigma * prob.sigma) : 0.f;
    const float e2 = eps * eps;
    float acc = 0.f;
    const bool fp = TRIG && prob.operator_kind == NSVD_OP_FOKKER_PLANCK;
    float adv = 0.f, lv = 0.f;
    for (int d = 0; d < D; ++d) {
        const float bEd = bcol[(size_t)(1 + 2 * d) * bs], bOd = bcol[(size_t)(2 + 2 * d) * bs];
        const float* q = dir + (size_t)d * NSVD_FD_DIR_FIELDS * es;
        float ev, od;
        if (has_mask) {  // rho depends on scales_l: nsvd_fd_evenodd's expressions, per head
            const float b = 2.f * xr[d] * eps;
            float sv = qs * e2, av = qs * b;
            const float rp = sqrtf(fmaxf(r2 + (e2 + b), 0.f)), rm = sqrtf(fmaxf(r2 + (e2 - b), 0.f));
            const float S = rp + rm, den = (rp + r0) * (rm + r0);
            const float tsum = (e2 * (S + 2.f * r0) - 2.f * b * b / S) / den;
            const float tdif = b * ((S + 2.f * r0) - 2.f * e2 / S) / den;
            sv -= 0.5f * tsum / s_l;
            av -= 0.5f * tdif / s_l;
            const float sh = sinhf(0.5f * av), chm1 = 2.f * sh * sh, es1 = expm1f(sv);
            ev = 2.f * (es1 * (1.f + chm1) + chm1);  // rho_+ + rho_-
            od = 2.f * (1.f + es1) * sinhf(av);      // rho_+ - rho_-
        } else {
            ev = q[NSVD_DIR_EV * es];
            od = q[NSVD_DIR_OD * es];
        }
        if (box.mode) {
            const float Mrest = q[NSVD_DIR_MREST * es], m0 = q[NSVD_DIR_M0 * es];
            const float ds = q[NSVD_DIR_DS * es], dd = q[NSVD_DIR_DD * es];
            const float sgs = m0 * ev + ds + 0.5f * (ev * ds + od * dd);
            const float sgd = m0 * od + dd + 0.5f * (ev * dd + od * ds);
            acc += Mrest * (sgs * (base0 + bEd) + 2.f * m0 * bEd + sgd * bOd);
        } else {
            acc += ev * (base0 + bEd) + 2.f * bEd + od * bOd;
            if (fp) {
                adv = fmaf(q[NSVD_DIR_VDIF * es], od * (base0 + bEd) + (2.f + ev) * bOd, adv);
                lv += q[NSVD_DIR_VSUM2 * es];
            }
        }
    }
    const float eps2 = (float)((double)prob.eps * (double)prob.eps);
    const float spc = prob.use_importance ? fmaxf(sp0, NSVD_SQRT_P_CLAMP) : 1.f;
    const float lap = ((c * (sp0 * mk0)) * acc / eps2) / spc;
    const float fs = (sp0 * (c * base0 * (mk0 * w.M0))) / spc;
    NsvdFdOut o;
    o.f = fs;
    if (fp) {
        o.Tf = prob.op_scale * nsvd_fp_apply(prob, lap, fs, (c * (sp0 * mk0)) / spc, adv, lv, eps2) + prob.op_shift * fs;
    } else {
        const float H = -prob.scale_kinetic * lap + w.V * fs;
        o.Tf = prob.op_scale * (-H) + prob.op_shift * fs;
    }
    const float wt = (sp0 / spc) * c;
    o.jac = wt * (mk0 * w.M0);
    o.dsc = has_mask ? wt * base0 * (mk0 * w.M0) * r0 / (s_l * s_l) : 0.f;
    return o;
}

template <bool TRIG = true>
__device__ __forceinline__ NsvdFdOut nsvd_fd_point(const float* bv, const float* xc, int D, bool has_mask, float s_l,
                                                   const nsvd_problem& prob, float log_norm, const NsvdBox& box) {
    const int E = 1 + 2 * D;
    float g[2 * NSVD_FD_MAXD + 1];
    float sp0 = 1.f, mask0 = 1.f, r0 = 0.f;
    for (int e = 0; e < E; ++e) {
        const NsvdFdG o = nsvd_fd_g(e, bv[e], xc, D, has_mask, s_l, prob, log_norm, box);
        g[e] = o.g;
        if (e == 0) {
            sp0 = o.sp;
            mask0 = o.mk;
            r0 = o.r;
        }
    }
    return nsvd_fd_combine<TRIG>(g, sp0, mask0, r0, bv[0], D, has_mask, s_l, prob,
                           box.mode ? nsvd_box_point(xc, D, 0, prob.eps, box) : 1.f, xc);
}

// Exact-Laplacian mode (laplacian_eps <= 0: VectorizedLaplacian.exact_laplacian, diff_ops.py:54-61): the model's
// value, gradient and Laplacian at x come from the forward-mode jet; here the product rule with the radial factor
// u = c * sqrt p(x) * mask_l(x), whose derivatives are closed forms:
//   sqrt p = C exp(-|x|^2 / (4 sigma^2)):  grad = -x / (2 sigma^2) sqrt p,  Lap = (-D / (2 sigma^2) + |x|^2 / (4 sigma^4)) sqrt p
//   mask   = exp(-r / s):                  grad = -(x / r) / s mask,        Lap = (1 / s^2 - (D - 1) / (r s)) mask
//   Lap(u v) = u Lap v + 2 grad u . grad v + v Lap u;  then lap / clamp(sqrt p), f = g / clamp(sqrt p), Tf as above.
// Box mask: U = u M, grad M_d = m'(x_d) prod_{j != d} m(x_j) =: G_d, Lap M = sum_d m''(x_d) prod_{j != d} m(x_j) (no
// division by m_d), grad U = u (M gu x + G), Lap U = u (M lu + 2 gu x . G + Lap M); outside the box all of it is 0:
//   sqrt: A = lim^2 + a b, m' = -t / (lim sqrt A), m'' = -2 lim / A^(3/2)
//   exp:  m' = -(e^-a - e^-b), m'' = -(e^-a + e^-b)
__device__ __forceinline__ NsvdFdOut nsvd_fd_exact(float base, const float* dbase, float lbase, const float* xc, int D,
                                                   bool has_mask, float s_l, const nsvd_problem& prob, float log_norm,
                                                   const NsvdBox& box) {
    float r2 = 0.f;
    for (int d = 0; d < D; ++d) r2 = fmaf(xc[d], xc[d], r2);
    const float r0 = sqrtf(r2);
    const float c = prob.hard_mul_const;
    float sp = 1.f, lsp_f = 0.f, dsp_f = 0.f;  // sqrt p, Lap sqrt p / sqrt p, and grad sqrt p = dsp_f * x * sqrt p
    if (prob.use_importance == NSVD_IMP_GAUSSIAN) {
        sp = nsvd_sqrt_gauss_pdf(xc, D, prob.sigma, log_norm);
        const float is2 = 1.f / (2.f * prob.sigma * prob.sigma);
        dsp_f = -is2;
        lsp_f = -(float)D * is2 + r2 * is2 * is2;
    } else if (prob.use_importance == NSVD_IMP_UNIFORM) {
        sp = nsvd_sqrt_p(prob, xc, D, log_norm);
    }
    float mk = 1.f, lmk_f = 0.f, dmk_f = 0.f;  // mask, Lap mask / mask, grad mask = dmk_f * x * mask
    if (has_mask) {
        mk = expf(-r0 / s_l);
        dmk_f = -1.f / (r0 * s_l);
        lmk_f = 1.f / (s_l * s_l) - (float)(D - 1) / (r0 * s_l);
    }
    const float u = c * sp * mk;
    // grad u = u (dsp_f + dmk_f) x;  Lap u = u (lsp_f + 2 dsp_f dmk_f |x|^2 + lmk_f)
    const float gu = dsp_f + dmk_f;
    float dot = 0.f;
    for (int d = 0; d < D; ++d) dot = fmaf(xc[d], dbase[d], dot);
    const float lu = lsp_f + 2.f * dsp_f * dmk_f * r2 + lmk_f;
    float g = u * base;
    float lap = u * (lbase + 2.f * gu * dot + base * lu);
    float M = 1.f;
    if (box.mode) {
        float m[NSVD_FD_MAXD], m1[NSVD_FD_MAXD], m2[NSVD_FD_MAXD];
        for (int d = 0; d < D; ++d) {
            const float a = box.lim - xc[d], b = box.lim + xc[d];
            m[d] = nsvd_box_m1(a, b, box);
            m1[d] = m2[d] = 0.f;
            if (a > 0.f && b > 0.f) {
                if (box.mode == NSVD_BOX_SQRT) {
                    const float A = fmaf(box.lim, box.lim, a * b), sA = sqrtf(A);
                    m1[d] = -xc[d] / (box.lim * sA);
                    m2[d] = -2.f * box.lim / (A * sA);
                } else {
                    const float ea = expf(-a), eb = expf(-b);
                    m1[d] = -(ea - eb);
                    m2[d] = -(ea + eb);
                }
            }
            M *= m[d];
        }
        float gdot = 0.f, xG = 0.f, lM = 0.f;  // G . grad base, x . G, Lap M
        for (int d = 0; d < D; ++d) {
            float Mrest = 1.f;
            for (int j = 0; j < D; ++j)
                if (j != d) Mrest *= m[j];
            gdot = fmaf(m1[d] * Mrest, dbase[d], gdot);
            xG = fmaf(m1[d] * Mrest, xc[d], xG);
            lM = fmaf(m2[d], Mrest, lM);
        }
        g = u * M * base;
        lap = u * (M * lbase + 2.f * (M * gu * dot + gdot) + base * (M * lu + 2.f * gu * xG + lM));
    }
    const float spc = prob.use_importance ? fmaxf(sp, NSVD_SQRT_P_CLAMP) : 1.f;
    lap = lap / spc;
    const float fs = g / spc;
    const float V = nsvd_potential(prob, xc, D, r0);
    const float H = -prob.scale_kinetic * lap + V * fs;
    NsvdFdOut o;
    o.f = fs;
    o.Tf = prob.op_scale * (-H) + prob.op_shift * fs;
    const float w = (sp / spc) * c;
    o.jac = w * (mk * M);
    o.dsc = has_mask ? w * base * (mk * M) * r0 / (s_l * s_l) : 0.f;
    return o;
}

// ---- the same product rule for 5 <= D <= NSVD_MAX_D (NSVD_PATH_GENERIC_EXACT): a loop over directions ----------------
// nsvd_fd_exact's expressions with the head's jet read from MEMORY - base = bcol[0], d base / d x_d = bcol[(1 + d) bs],
// Lap base = bcol[(D + 1) bs] (bs = B in the (L, (D + 2) B) layout of the generic jets) - and no per-thread array indexed
// by a run-time d. What the L heads of a row share comes from nsvd_fd_row_nd (|x|, sqrt p, V, the box mask at the centre)
// and, per direction, from a table of NSVD_FDX_DIR_FIELDS floats that ONE thread per row fills (nsvd_fd_exact_dirs_nd):
// field k of direction d at dir[(d NSVD_FDX_DIR_FIELDS + k) es], as nsvd_fd_dir_nd's. The box factors
// G_d = m'(x_d) prod_{j != d} m(x_j) take a prefix product on the way up and a suffix product on the way down instead of
// the j != d inner loop; x . G and Lap M, which no head changes, are summed on the way down.
#define NSVD_FDX_DIR_FIELDS 3
enum { NSVD_XDIR_X = 0, NSVD_XDIR_G, NSVD_XDIR_M2 };
struct NsvdFdExactRowNd {
    float xG, lM;  // x . G, Lap M (0 without a box mask)
};
// m'(t), m''(t) inside the box (0 at and beyond the wall): nsvd_fd_exact's closed forms
__device__ __forceinline__ void nsvd_box_m12(float t, const NsvdBox& box, float* m1, float* m2) {
    const float a = box.lim - t, b = box.lim + t;
    *m1 = *m2 = 0.f;
    if (a > 0.f && b > 0.f) {
        if (box.mode == NSVD_BOX_SQRT) {
            const float A = fmaf(box.lim, box.lim, a * b), sA = sqrtf(A);
            *m1 = -t / (box.lim * sA);
            *m2 = -2.f * box.lim / (A * sA);
        } else {
            const float ea = expf(-a), eb = expf(-b);
            *m1 = -(ea - eb);
            *m2 = -(ea + eb);
        }
    }
}
__device__ __forceinline__ NsvdFdExactRowNd nsvd_fd_exact_dirs_nd(const float* xr, int D, const NsvdBox& box, float* dir,
                                                                  size_t es) {
    float pre = 1.f;  // prod_{j < d} m(x_j)
    for (int d = 0; d < D; ++d) {
        float* q = dir + (size_t)d * NSVD_FDX_DIR_FIELDS * es;
        const float xd = xr[d];
        q[NSVD_XDIR_X * es] = xd;
        if (box.mode) {
            float m1, m2;
            nsvd_box_m12(xd, box, &m1, &m2);
            q[NSVD_XDIR_G * es] = pre * m1;
            q[NSVD_XDIR_M2 * es] = pre * m2;
            pre *= nsvd_box_m1(box.lim - xd, box.lim + xd, box);
        }
    }
    NsvdFdExactRowNd o;
    o.xG = o.lM = 0.f;
    if (box.mode) {
        float suf = 1.f;  // prod_{j > d} m(x_j)
        for (int d = D - 1; d >= 0; --d) {
            float* q = dir + (size_t)d * NSVD_FDX_DIR_FIELDS * es;
            const float xd = q[NSVD_XDIR_X * es];
            const float G = q[NSVD_XDIR_G * es] * suf;
            q[NSVD_XDIR_G * es] = G;
            o.xG = fmaf(G, xd, o.xG);
            o.lM = fmaf(q[NSVD_XDIR_M2 * es], suf, o.lM);
            suf *= nsvd_box_m1(box.lim - xd, box.lim + xd, box);
        }
    }
    return o;
}
__device__ __forceinline__ NsvdFdOut nsvd_fd_exact_nd(const NsvdFdRowNd& w, const NsvdFdExactRowNd& e, const float* bcol,
                                                      size_t bs, int D, bool has_mask, float s_l,
                                                      const nsvd_problem& prob, const NsvdBox& box, const float* dir,
                                                      size_t es) {
    const float r2 = w.r2, r0 = w.r0, sp = w.sp0;
    const float base = bcol[0], lbase = bcol[(size_t)(D + 1) * bs];
    const float c = prob.hard_mul_const;
    float lsp_f = 0.f, dsp_f = 0.f;  // Lap sqrt p / sqrt p, and grad sqrt p = dsp_f * x * sqrt p
    if (prob.use_importance == NSVD_IMP_GAUSSIAN) {
        const float is2 = 1.f / (2.f * prob.sigma * prob.sigma);
        dsp_f = -is2;
        lsp_f = -(float)D * is2 + r2 * is2 * is2;
    }
    float mk = 1.f, lmk_f = 0.f, dmk_f = 0.f;  // mask, Lap mask / mask, grad mask = dmk_f * x * mask
    if (has_mask) {
        mk = expf(-r0 / s_l);
        dmk_f = -1.f / (r0 * s_l);
        lmk_f = 1.f / (s_l * s_l) - (float)(D - 1) / (r0 * s_l);
    }
    const float u = c * sp * mk;
    const float gu = dsp_f + dmk_f;
    float dot = 0.f, gdot = 0.f;  // x . grad base, G . grad base
    for (int d = 0; d < D; ++d) {
        const float* q = dir + (size_t)d * NSVD_FDX_DIR_FIELDS * es;
        const float db = bcol[(size_t)(1 + d) * bs];
        dot = fmaf(q[NSVD_XDIR_X * es], db, dot);
        if (box.mode) gdot = fmaf(q[NSVD_XDIR_G * es], db, gdot);
    }
    const float lu = lsp_f + 2.f * dsp_f * dmk_f * r2 + lmk_f;
    const float M = w.M0;
    float g = u * base;
    float lap = u * (lbase + 2.f * gu * dot + base * lu);
    if (box.mode) {
        g = u * M * base;
        lap = u * (M * lbase + 2.f * (M * gu * dot + gdot) + base * (M * lu + 2.f * gu * e.xG + e.lM));
    }
    const float spc = prob.use_importance ? fmaxf(sp, NSVD_SQRT_P_CLAMP) : 1.f;
    lap = lap / spc;
    const float fs = g / spc;
    const float H = -prob.scale_kinetic * lap + w.V * fs;
    NsvdFdOut o;
    o.f = fs;
    o.Tf = prob.op_scale * (-H) + prob.op_shift * fs;
    const float wt = (sp / spc) * c;
    o.jac = wt * (mk * M);
    o.dsc = has_mask ? wt * base * (mk * M) * r0 / (s_l * s_l) : 0.f;
    return o;
}

// ---- NeuralEF (neuralef.hip): every stencil point divided by its own batch norm (methods/utils.py:48-56) ----------------
// Even / odd parts of rho_+- = w(x_+-) / w(x0) - 1 along direction d: ev = rho_+ + rho_-, od = rho_+ - rho_-, with
// w = sqrt p (qs = d log sqrt p / d |x|^2, 0 without importance) times the mask (has_mask) - nsvd_fd_evenodd's arithmetic
struct NsvdEvenOdd {
    float ev, od;
};
__device__ __forceinline__ NsvdEvenOdd nsvd_fd_ratio_eo(float xd, float r2, float r0, float eps, float qs, bool has_mask,
                                                        float s_l) {
    const float e2 = eps * eps;
    const float b = 2.f * xd * eps;
    float sv = qs * e2, av = qs * b;
    if (has_mask) {
        const float rp = sqrtf(fmaxf(r2 + (e2 + b), 0.f)), rm = sqrtf(fmaxf(r2 + (e2 - b), 0.f));
        const float S = rp + rm, den = (rp + r0) * (rm + r0);
        const float tsum = (e2 * (S + 2.f * r0) - 2.f * b * b / S) / den;
        const float tdif = b * ((S + 2.f * r0) - 2.f * e2 / S) / den;
        sv -= 0.5f * tsum / s_l;
        av -= 0.5f * tdif / s_l;
    }
    const float sh = sinhf(0.5f * av), chm1 = 2.f * sh * sh, es1 = expm1f(sv);
    NsvdEvenOdd o;
    o.ev = 2.f * (es1 * (1.f + chm1) + chm1);
    o.od = 2.f * (1.f + es1) * sinhf(av);
    return o;
}

// Head output u = c base mask at x +- eps e_d minus the centre's, u_+- - u0 = P +- Q (mask ratio (evm, odm)):
//   P = c mk0 [evm / 2 (base0 + bE) + odm / 2 bO + bE],  Q = c mk0 [odm / 2 (base0 + bE) + evm / 2 bO + bO]
// so that the per-sample terms of n_+-^2 - n_0^2 = mean_b (u_+-^2 - u0^2) are formed without a difference of large numbers:
//   u_+-^2 - u0^2 = (2 u0 P + P^2 + Q^2) +- (2 u0 Q + 2 P Q)
struct NsvdNefDelta {
    float even, odd;
};
__device__ __forceinline__ NsvdNefDelta nsvd_nef_sqdelta(float u0, float cmk0, float base0, float bE, float bO,
                                                         NsvdEvenOdd m) {
    const float be = base0 + bE;
    const float P = cmk0 * (0.5f * m.ev * be + 0.5f * m.od * bO + bE);
    const float Q = cmk0 * (0.5f * m.od * be + 0.5f * m.ev * bO + bO);
    NsvdNefDelta o;
    o.even = 2.f * u0 * P + P * P + Q * Q;
    o.odd = 2.f * (u0 * Q + P * Q);
    return o;
}

// nsvd_fd_evenodd with the stencil point x_e divided by its batch norm n_e = n0 / (1 + nu_e): g_+- = (c w0 / n0)
// (1 + sig_+-)(base0 + bE +- bO), 1 + sig = (1 + rho)(1 + nu), so the central difference keeps its even / odd form:
//     g_+ + g_- - 2 g_0 = (c w0 / n0) [ (sig_+ + sig_-)(base0 + bE) + 2 bE + (sig_+ - sig_-) bO ]
// nu[2 d], nu[2 d + 1]: nu of x + eps e_d, x - eps e_d. Outputs phi, Tphi (f, Tf), h = u0 / n0, r = sqrt p / clamp(sqrt p),
// and jac / dsc of u0 (d u0 / d base0, d u0 / d scales_l) - what the normalisation backward hands to the centre backward.
struct NsvdNefOut {
    float phi, Tphi, h, r, jac, dsc;
};
__device__ __forceinline__ NsvdNefOut nsvd_nef_evenodd(float base0, const float* bE, const float* bO, const float* xc,
                                                       int D, bool has_mask, float s_l, const nsvd_problem& prob,
                                                       float log_norm, float n0, const float* nu) {
    float r2 = 0.f;
    for (int d = 0; d < D; ++d) r2 = fmaf(xc[d], xc[d], r2);
    const float r0 = sqrtf(r2);
    const float c = prob.hard_mul_const;
    const float sp0 = prob.use_importance ? nsvd_sqrt_gauss_pdf(xc, D, prob.sigma, log_norm) : 1.f;
    const float mk0 = has_mask ? expf(-r0 / s_l) : 1.f;
    const float qs = prob.use_importance ? -1.f / (4.f * prob.sigma * prob.sigma) : 0.f;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) {
        const NsvdEvenOdd w = nsvd_fd_ratio_eo(xc[d], r2, r0, prob.eps, qs, has_mask, s_l);
        const float rp = 0.5f * (w.ev + w.od), rm = 0.5f * (w.ev - w.od);
        const float np = nu[2 * d], nm = nu[2 * d + 1];
        const float ev = w.ev + (np + nm) + (rp * np + rm * nm);
        const float od = w.od + (np - nm) + (rp * np - rm * nm);
        acc += ev * (base0 + bE[d]) + 2.f * bE[d] + od * bO[d];
    }
    const float eps2 = (float)((double)prob.eps * (double)prob.eps);
    const float spc = prob.use_importance ? fmaxf(sp0, NSVD_SQRT_P_CLAMP) : 1.f;
    const float u0 = c * base0 * mk0;
    const float h = u0 / n0;
    const float lap = ((c * (sp0 * mk0) / n0) * acc / eps2) / spc;
    const float fs = (sp0 * h) / spc;
    const float V = nsvd_potential(prob, xc, D, r0);
    const float H = -prob.scale_kinetic * lap + V * fs;
    NsvdNefOut o;
    o.phi = fs;
    o.Tphi = prob.op_scale * (-H) + prob.op_shift * fs;
    o.h = h;
    o.r = sp0 / spc;
    o.jac = c * mk0;
    o.dsc = has_mask ? c * base0 * mk0 * r0 / (s_l * s_l) : 0.f;
    return o;
}
