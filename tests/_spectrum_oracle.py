"""Float64 numpy restatement of one compute_spectrum_evd accumulation (reference methods/spectrum.py:56-75), the
reference of tests/test_spectrum_accumulate_gpu.py; held to the reference's own run by tests/test_spectrum_oracle.py
(tests/golden/spectrum_acc.npz). No torch device, no HIP.

    w     = sqrt(p_train(x)) / sqrt(p_val)      p_train: the N(0, sigma^2 I_D) pdf, or 1 (no importance_train)
                                                p_val: the FLOAT32 value 1 / (2 lim)^D and its float32 square root
                                                (main_pde.py:129-130 builds a float32 tensor; :24 takes .sqrt() of it)
    phi   = w f, Tphi = w Tf                    (:66-67)
    pad:    a constant-one column in front of both, after the weighting (:68-70)
    nan_to_num with float32 semantics (the kernels' inputs are float32): NaN -> 0, +-inf -> +-FLT_MAX (:71-72)
    rows of Tphi - the padded column too - zeroed where every |x_d| <= 1e-8 (torch.isclose(x, 0), :73)
    cov += phi^T phi, quad += phi^T Tphi        (:74-75)
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
LOG_2PI = 1.8378770664093453


def gauss_log_norm(D, sigma):
    return -0.5 * D * LOG_2PI - D * np.log(float(sigma))


def gauss_exponent(x, sigma):
    """log p_train(x) of the Gaussian density, float64: -0.5 |x / sigma|^2 + log_norm. The float32 exp of the kernel
    (and of the float32 reference) underflows below about -87: the GPU tests state and check > -80 for every row."""
    x = np.asarray(x, dtype=np.float64)
    return -0.5 * ((x / float(sigma)) ** 2).sum(1) + gauss_log_norm(x.shape[1], sigma)


def sqrt_weight(x, sigma, lim, gaussian, weight32=False):
    """w (B,) float64. weight32: the same formula evaluated in numpy float32 in the kernel's order (x / sigma, the sum
    of squares, exp, sqrt, times 1 / sqrt(p_val)) and widened - the yardstick for what a float32 weight costs."""
    x = np.asarray(x)
    B, D = x.shape
    pval = np.float32(1.0 / (2.0 * float(lim)) ** D)
    if weight32:
        x32 = x.astype(np.float32)
        inv = np.float32(1.0) / np.sqrt(pval)
        if not gaussian:
            return np.full(B, inv, dtype=np.float32).astype(np.float64)
        t = x32 / np.float32(sigma)
        m = np.zeros(B, dtype=np.float32)
        for d in range(D):
            m = t[:, d] * t[:, d] + m
        sp = np.sqrt(np.exp(np.float32(-0.5) * m + np.float32(gauss_log_norm(D, sigma))))
        return (sp * inv).astype(np.float64)
    sv = float(np.sqrt(pval))  # the float32 square root of the float32 value
    if not gaussian:
        return np.full(B, 1.0 / sv)
    return np.sqrt(np.exp(gauss_exponent(x, sigma))) / sv


def nan_to_num32(a):
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = 0.0
    a[np.isposinf(a)] = FLT_MAX
    a[np.isneginf(a)] = -FLT_MAX
    return a


def weighted(f, Tf, x, sigma, lim, gaussian, pad, weight32=False):
    """phi, Tphi (B, L + pad) float64 as they enter the two products"""
    f = np.asarray(f, dtype=np.float64)
    Tf = np.asarray(Tf, dtype=np.float64)
    x = np.asarray(x)
    w = sqrt_weight(x, sigma, lim, gaussian, weight32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        phi, tphi = w * f, w * Tf
    if pad:
        one = np.ones((f.shape[0], 1))
        phi, tphi = np.concatenate([one, phi], 1), np.concatenate([one, tphi], 1)
    phi, tphi = nan_to_num32(phi), nan_to_num32(tphi)
    tphi[np.all(np.abs(x.astype(np.float64)) <= 1e-8, axis=1)] = 0.0
    return phi, tphi


def accumulate(f, Tf, x, sigma, lim, gaussian, pad, weight32=False):
    """cov, quad, tt = phi^T phi, phi^T Tphi, Tphi^T Tphi of one chunk (float64). tt is not accumulated by anything: its
    diagonal is the Cauchy-Schwarz scale of quad's entries, |quad_ij| <= sqrt(cov_ii tt_jj)."""
    phi, tphi = weighted(f, Tf, x, sigma, lim, gaussian, pad, weight32)
    return phi.T @ phi, phi.T @ tphi, tphi.T @ tphi


def entry_error(got, want, row_scale, col_scale):
    """max_ij |got - want|_ij / sqrt(row_scale_i col_scale_j): each entry against its Cauchy-Schwarz bound (a relative
    L2 norm lets the large entries hide the small ones)"""
    s = np.sqrt(np.outer(np.asarray(row_scale, dtype=np.float64), np.asarray(col_scale, dtype=np.float64)))
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(s, 1e-300)))


def planted_rows(D):
    """the four rows that decide the x ~ 0 rule (D >= 2; at D = 1 the third is simply not at 0): the origin; 5e-9 on
    every axis (alternating signs): zeroed; (0, 1, 1, ...): some coordinates 0 only - kept; one coordinate 2e-8, the
    others 0: above isclose's 1e-8 - kept"""
    r = np.zeros((4, D), dtype=np.float32)
    r[1] = np.float32(5e-9) * np.where(np.arange(D) % 2 == 0, 1.0, -1.0).astype(np.float32)
    r[2] = 1.0
    if D > 1:
        r[2, 0] = 0.0
    r[3, D - 1] = np.float32(2e-8)
    return r
