"""Float64 numpy restatement of the 3-D hydrogen eigenfunctions (reference examples/operator/pde/schrodinger/
ground_truths.py: Hydrogen3D.eigfunc :177-193, real_sph_harm / sph_harm :218-270, cartesian_to_spherical :204-209) and
of the three weighted products of one chunk (nsvd_eigfunc3_accumulate_f64): the reference of
tests/test_eigfuncs3d_gpu.py, itself held to the reference's own values by tests/test_eigfunc3d_oracle.py
(tests/golden/eigfuncs3d.npz). No scipy, no torch device, no HIP.

Written the reference's way and NOT the kernel's: spherical angles from arctan2, cos(th) and sin(th) of them, the
complex exponential exp(-i |m| phi) whose real / imaginary part real_sph_harm picks, lpmv WITH its Condon-Shortley
phase and real_sph_harm's (-1)^|m| on top of it, factorials as integers. Only the Laguerre recurrence is shared with
the package (tests/_eigfunc_oracle.py). The metrics on (n, k) blocks are _eigfunc_oracle.metrics: they do not know the
dimension.
"""
import math

import numpy as np

from tests._eigfunc_oracle import laguerre, metrics, subspace_distance  # noqa: F401  (re-exported)
from tests._spectrum_oracle import gauss_log_norm, nan_to_num32

def qnums(count):
    """(n, l, m), n ascending, then l, then m from -l: the reference's order"""
    out, n = [], 1
    while len(out) < count:
        out += [(n, l, m) for l in range(n) for m in range(-l, l + 1)]
        n += 1
    return out[:count]


def lpmv(a, l, u, s):
    """scipy's lpmv(a, l, u) for integers 0 <= a <= l, u = cos(th): P_l^a WITH the Condon-Shortley phase (-1)^a.
    s = sin(th) is handed in: sqrt(1 - u^2) loses half the digits next to the z axis, where sin(arctan2(., .)) keeps them"""
    pm, pc = np.zeros_like(u), np.ones_like(u)
    for j in range(1, a + 1):
        pc = -(2 * j - 1) * s * pc
    for j in range(a, l):
        pm, pc = pc, ((2 * j + 1) * u * pc - (j + a) * pm) / (j - a + 1)
    return pc


def hydrogen3d(Z, n, l, m, x, y, z):
    r = np.sqrt(x ** 2 + y ** 2 + z ** 2)
    th = np.arctan2(np.sqrt(x ** 2 + y ** 2), z)
    phi = np.arctan2(y, x)
    f = math.factorial
    a0 = 2.0 / Z
    rho = 2 * r / (n * a0)
    radial = (math.sqrt((2 / (n * a0)) ** 3 / (2 * n)) * rho ** l * np.exp(-0.5 * rho) *
              math.sqrt(f(n - l - 1) / f(n + l)) * laguerre(n - l - 1, 2 * l + 1, rho))
    a = abs(m)
    # sph_harm([-a, l], [phi, th]): exp(-i a phi) * sqrt((2l + 1) / 2 * (l - a)! / (l + a)!) lpmv(a, l, cos th) / sqrt(2 pi)
    ys = np.exp(-1j * a * phi) * math.sqrt((2 * l + 1) / 2 * f(l - a) / f(l + a)) * lpmv(a, l, np.cos(th), np.sin(th)) / math.sqrt(
        2 * math.pi)
    if a == 0:
        return radial * ys.real
    sign = 1 if a % 2 == 0 else -1
    return radial * math.sqrt(2) * sign * (ys.imag if m > 0 else ys.real)


def evaluate(Z, q, x):
    """psi (B, Lg) float64 at the float32 points x (B, 3), widened first"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return np.stack([hydrogen3d(float(Z), int(n), int(l), int(m), x[:, 0], x[:, 1], x[:, 2]) for n, l, m in q], 1)


def inv_sqrt_val32(lim):
    """1 / sqrt(p_val) as the library forms it on the host: p_val = (2 lim)^-3 rounded to float32, its float32 square
    root, the float32 reciprocal"""
    pval = np.float32(1.0 / (2.0 * float(np.float32(lim))) ** 3)
    return np.float32(1.0) / np.sqrt(pval)


def weights32(x, sigma, lim, gaussian):
    """w = sqrt(p_train) / sqrt(p_val) per row in numpy float32, in the kernel's order over three coordinates
    (_eigfunc_oracle.weights32 at D = 3 with the 3-D p_val). With importance the device's expf may differ in the last
    bit: the GPU tests measure the device's w and hand that to `weighted`."""
    x = np.asarray(x, dtype=np.float32)
    inv = inv_sqrt_val32(lim)
    if not gaussian:
        return np.full(len(x), inv, dtype=np.float32)
    t = x / np.float32(sigma)
    m = np.zeros(len(x), dtype=np.float32)
    for d in range(3):
        m = t[:, d] * t[:, d] + m
    return np.sqrt(np.exp(np.float32(-0.5) * m + np.float32(gauss_log_norm(3, sigma)))) * inv


def weighted(Z, q, f, x, lim, w32):
    """psi_w (B, Lg), phi (B, L) float64 as they enter the products: phi = nan_to_num(w * f) in float32, w (B,) float32;
    psi_w = psi / sqrt(p_val) in float64"""
    w = np.asarray(w32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        phi = nan_to_num32(w[:, None] * np.asarray(f, dtype=np.float32))
    return evaluate(Z, q, x) * float(inv_sqrt_val32(lim)), phi


def products(Z, q, f, x, lim, w32):
    """gram, cross, cov of one chunk"""
    psi, phi = weighted(Z, q, f, x, lim, w32)
    return psi.T @ psi, psi.T @ phi, phi.T @ phi
