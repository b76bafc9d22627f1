"""Float64 numpy restatement of the eigenfunction evaluation: the analytic functions of the three 2-D ground truths
(reference examples/operator/pde/schrodinger/ground_truths.py), the three weighted products of one chunk
(nsvd_eigfunc_accumulate_f64) and the metrics (examples/linalg.py), the reference of tests/test_eigfuncs_gpu.py; itself
held to the reference's own values by tests/test_eigfunc_oracle.py (tests/golden/eigfuncs.npz). No scipy, no torch
device, no HIP.

The functions are written the reference's way (polar coordinates and cos(l th) from arctan2 for hydrogen, the 1-D
product for the oscillator, the [0, L] formula for the well) and NOT the kernel's (x / r and the Chebyshev recurrence):
only the two polynomial recurrences are shared with the package. The metrics work on the (n, k) BLOCKS, as linalg.py
does, not on the small matrices eigenfunction_metrics takes.
"""
import math

import numpy as np

from tests._spectrum_oracle import gauss_log_norm, nan_to_num32

HYDROGEN2D, HARMONIC2D, WELL2D = 0, 1, 2


def laguerre(k, alpha, z):
    lm, lc = np.zeros_like(z), np.ones_like(z)
    for j in range(k):
        lm, lc = lc, ((2 * j + 1 + alpha - z) * lc - (j + alpha) * lm) / (j + 1)
    return lc


def hermite(n, u):
    hm, hc = np.zeros_like(u), np.ones_like(u)
    for j in range(n):
        hm, hc = hc, 2 * u * hc - 2 * j * hm
    return hc


def hydrogen(Z, n, l, x, y):
    """Z psi_1(Z x): ground_truths.py:134-149 with hyp1f1(-k, 2a + 1, z) = k! (2a)! / (k + 2a)! L_k^(2a)(z); at r = 0
    the limit (0 ** 0 = 1 for l = 0, 0 otherwise; arctan2(0, 0) = 0)"""
    r, th = np.sqrt(x * x + y * y) * Z, np.arctan2(y, x)
    a, beta = abs(l), 1.0 / (n + 0.5)
    lg = math.lgamma
    # the reference's coefficient times hyp1f1's k! (2a)! / (k + 2a)!, k = n - a
    coef = math.exp(math.log(beta) - lg(2 * a + 1) + 0.5 * (lg(n + a + 1) - math.log(2 * n + 1) - lg(n - a + 1))
                    + lg(n - a + 1) + lg(2 * a + 1) - lg(n + a + 1))
    z = beta * r
    radial = coef * z ** a * np.exp(-z / 2) * laguerre(n - a, 2 * a, z)
    if l > 0:
        ang = np.cos(l * th) / math.sqrt(math.pi)
    elif l < 0:
        ang = np.sin(l * th) / math.sqrt(math.pi)
    else:
        ang = 1.0 / math.sqrt(2 * math.pi)
    return Z * radial * ang


def harmonic(k, nx, ny, x, y):
    b = math.sqrt(k)

    def one(n, t):
        return (1.0 / math.sqrt(2.0 ** n * math.factorial(n)) * (b / math.pi) ** 0.25 * np.exp(-b * t ** 2 / 2) *
                hermite(n, math.sqrt(b) * t))
    return one(nx, x) * one(ny, y)


def well(lim, nx, ny, x, y):
    side = 2.0 * lim
    inside = (np.abs(x) <= lim) & (np.abs(y) <= lim)
    v = 2.0 / side * np.sin(nx * np.pi * (x + lim) / side) * np.sin(ny * np.pi * (y + lim) / side)
    return np.where(inside, v, 0.0)


def evaluate(kind, param, qnums, x):
    """psi (B, Lg) float64 at the float32 points x (B, 2), widened first"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    fn = {HYDROGEN2D: hydrogen, HARMONIC2D: harmonic, WELL2D: well}[kind]
    return np.stack([fn(float(param), int(a), int(b), x[:, 0], x[:, 1]) for a, b in qnums], 1)


def inv_sqrt_val32(lim):
    """1 / sqrt(p_val) as the library forms it on the host: p_val = 1 / (2 lim)^2 rounded to float32, its float32 square
    root, the float32 reciprocal"""
    pval = np.float32(1.0 / (2.0 * float(np.float32(lim))) ** 2)
    return np.float32(1.0) / np.sqrt(pval)


def weights32(x, sigma, lim, gaussian):
    """w = sqrt(p_train) / sqrt(p_val) per row in numpy float32 in the kernel's order (nsvd_sqrt_gauss_pdf, then one
    float32 product with 1 / sqrt(p_val)). The device's expf may differ from numpy's in the last bit, which is 6e-8 of
    phi: the GPU tests MEASURE the device's w (exactly: the square root of a one-row float64 cov) and hand that to
    `weighted`; without importance w is the host constant and this function is exact."""
    x = np.asarray(x, dtype=np.float32)
    inv = inv_sqrt_val32(lim)
    if not gaussian:
        return np.full(len(x), inv, dtype=np.float32)
    t = x / np.float32(sigma)
    m = np.zeros(len(x), dtype=np.float32)
    for d in range(x.shape[1]):
        m = t[:, d] * t[:, d] + m
    return np.sqrt(np.exp(np.float32(-0.5) * m + np.float32(gauss_log_norm(x.shape[1], sigma)))) * inv


def weighted(kind, param, qnums, f, x, lim, w32):
    """psi_w (B, Lg), phi (B, L) float64 as they enter the products. phi is FLOAT32 arithmetic, as spectrum.hip's:
    phi = nan_to_num(w * f), one float32 product, w (B,) float32 as above. psi_w = psi / sqrt(p_val), float64."""
    w = np.asarray(w32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        phi = nan_to_num32(w[:, None] * np.asarray(f, dtype=np.float32))
    return evaluate(kind, param, qnums, x) * float(inv_sqrt_val32(lim)), phi


def products(kind, param, qnums, f, x, lim, w32):
    """gram, cross, cov of one chunk"""
    psi, phi = weighted(kind, param, qnums, f, x, lim, w32)
    return psi.T @ psi, psi.T @ phi, phi.T @ phi


# ---- examples/linalg.py on (n, k) blocks -----------------------------------------------------------------------------
def _inv_sqrt(M):
    w, V = np.linalg.eigh(M)
    return (V / np.sqrt(w)) @ V.T


def subspace_distance(A1, A2):
    """linalg.py:5-8 with k = the columns of A2 (the reference's k = A1.shape[1] for two blocks of equal width)"""
    k = A2.shape[1]
    return 1 - np.trace(A2.T @ A1 @ np.linalg.inv(A1.T @ A1) @ A1.T @ A2 @ np.linalg.inv(A2.T @ A2)) / k


def rotate(U_, V_):
    """linalg.py:11-16: the projection of the columns of U_ onto span(V_)"""
    Vhat = V_ @ _inv_sqrt(V_.T @ V_)
    return Vhat @ (Vhat.T @ U_)


def procrustes_q(A_, Ahat_):
    """linalg.py:19-28: Q with Ahat_ Q closest to A_"""
    U, _, Vt = np.linalg.svd(Ahat_.T @ A_)
    return U @ Vt


def metrics(Psi, Phi, degeneracy, order=None):
    """what eigfuncs.eigenfunction_metrics returns, from the (n, Lg) and (n, L) blocks"""
    n, Lg = Psi.shape
    L = Phi.shape[1]
    order = np.arange(L) if order is None else np.asarray(order)
    dist, resid, defect, rot, levels = [], [], [], [], []
    angle = np.full(Lg, np.nan)
    for s, e in zip(degeneracy[:-1], degeneracy[1:]):
        if s >= L:
            break
        cols = order[s:min(e, L)]
        A1, A2 = Psi[:, s:e], Phi[:, cols]
        dist.append(subspace_distance(A1, A2))
        defect.append(np.max(np.abs(A1.T @ A1 / n - np.eye(e - s))))
        levels.append((s, e, len(cols)))
        if len(cols) < e - s:
            rot.append(None)
            resid.append(np.nan)
            continue
        proj = rotate(A1, A2)
        cosv = np.linalg.norm(proj, axis=0) / np.linalg.norm(A1, axis=0)
        angle[s:e] = np.arccos(np.clip(cosv, 0.0, 1.0))
        Ph, Ps = A2 @ _inv_sqrt(A2.T @ A2), A1 @ _inv_sqrt(A1.T @ A1)
        Q = procrustes_q(Ps, Ph)
        rot.append(Q)
        resid.append(np.linalg.norm(Ph @ Q - Ps) ** 2 / (e - s))
    return dict(subspace_distance=np.array(dist), angle=angle[:levels[-1][1]], rotation=rot,
                procrustes_residual=np.array(resid), gram_defect=np.array(defect), levels=levels)
