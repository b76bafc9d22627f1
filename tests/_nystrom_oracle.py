"""Two restatements of the Nystrom baseline (reference methods/nystrom.py:8-47; neural_svd_amd/nystrom.py).

(a) ``definition``: the float64 Gram matrix of tests/_rbf_oracle.radial_kernel_matrix, ``np.linalg.eigh`` on it, the
    top eigenpairs of G = K / n, and the projection formula K(xnew, xs) @ eigvecs / eigvals / sqrt(n).
(b) ``subspace_iteration``: the block subspace iteration with Rayleigh-Ritz the device solver runs (same steps, same
    stopping rule), with every small matrix in float64 and library eigh / Cholesky in place of the device's Jacobi.
    ``store`` is the dtype of the n x m blocks: with float32 the product W = G V is a float32 matmul and V is rounded
    to float32 between the steps - what the device does, and what keeps W^T W positive definite at a numerically
    rank-deficient Gaussian Gram (the float32 product leaves a noise floor of ~1e-7 lambda_0 under the trailing
    columns; without it W^T W of a random start has eigenvalues below the float64 rounding of its entries and the
    Cholesky factorisation can fail); float64 is the recurrence without any rounding, for well-conditioned input.
"""
import numpy as np
import torch

from tests import _rbf_oracle as R

GAUSSIAN, EXPONENTIAL = R.GAUSSIAN, R.EXPONENTIAL


def gram(xs, kind, ell):
    """G = k(xs, xs) / n, float64 numpy"""
    K = R.radial_kernel_matrix(xs, xs, kind, ell).numpy()
    return K / K.shape[0]


def definition(xs, kind, ell, dim):
    """(eigvals (dim,), eigvecs (n, dim), all eigenvalues descending) of G in float64"""
    w, U = np.linalg.eigh(gram(xs, kind, ell))
    w, U = w[::-1], U[:, ::-1]
    return w[:dim].copy(), U[:, :dim].copy(), w.copy()


def project(xnew, xs, kind, ell, eigvals, eigvecs):
    """the reference's __call__: kernel(xnew, xs) @ eigvecs / eigvals / sqrt(n), in float64"""
    K = R.radial_kernel_matrix(xnew, xs, kind, ell).numpy()
    return K @ np.asarray(eigvecs, dtype=np.float64) / np.asarray(eigvals, dtype=np.float64) / np.sqrt(len(xs))


def ritz_step(S, A, C=None):
    """step 3 of the recurrence in float64 numpy: (theta, resid, Q, T); A None: orthonormalisation only; C = V^T V of
    the basis as stored (None: the identity): resid_k^2 = M_kk - theta_k^2 (2 - q_k^T C q_k) = |W q_k - theta_k V q_k|^2"""
    m = S.shape[0]
    if A is None:
        theta, Q = np.zeros(m), np.eye(m)
        M = S
    else:
        w, Q = np.linalg.eigh(0.5 * (A + A.T))
        order = np.argsort(-w, kind="stable")
        theta, Q = w[order], Q[:, order]
        M = Q.T @ S @ Q
    dk = np.zeros(m) if C is None else np.einsum("ik,ij,jk->k", Q, C - np.eye(m), Q)
    resid = np.sqrt(np.maximum(np.diag(M) - theta ** 2 * (1.0 - dk), 0.0)) if A is not None else np.zeros(m)
    Rm = np.linalg.cholesky(0.5 * (M + M.T)).T  # upper
    T = np.linalg.solve(Rm.T, Q.T).T            # Q R^-1
    return theta, resid, Q, T


def subspace_iteration(G, dim, oversample=8, tol=1e-5, max_iters=200, seed=0, store=np.float32):
    """-> dict(eigvals, eigvecs, iterations, residuals (relative), converged). G: (n, n) float64."""
    n = G.shape[0]
    m = min(n, dim + oversample)
    rng = np.random.default_rng(seed)
    V0 = rng.standard_normal((n, m)).astype(store).astype(np.float64)
    _, _, _, T = ritz_step(V0.T @ V0, None)
    V = (V0 @ T).astype(store).astype(np.float64)
    Gs = G.astype(store)
    it, converged = 0, False
    for it in range(1, max_iters + 1):
        W = (Gs @ V.astype(store)).astype(np.float64)
        theta, resid, Q, T = ritz_step(W.T @ W, V.T @ W, V.T @ V)
        if theta[0] > 0 and resid[:dim].max() <= tol * theta[0]:
            converged = True
            break
        if it < max_iters:
            V = (W @ T).astype(store).astype(np.float64)
    return dict(eigvals=theta[:dim].copy(), eigvecs=(V @ Q[:, :dim]).astype(store).astype(np.float64), iterations=it,
                residuals=resid[:dim] / theta[0], converged=converged)


def tsgram_slices(n):
    """nsvd_tsgram_f64's split rule (csrc/nystrom.hip:ts_slices): slices of 64 rows, at most 128"""
    return max(1, min(128, (n + 63) // 64))


def tsgram_workspace_bytes(n, m):
    """two (m, m) float64 partial matrices per slice, rounded up to 256 bytes"""
    return (tsgram_slices(n) * 2 * m * m * 8 + 255) // 256 * 256


# ---- the solver cases shared by tests/test_nystrom_oracle.py (recurrence (b) against (a)) and tests/test_nystrom_gpu.py
# (n, D, L, kind, ell, shift). Gaussian ell 1.5 (D <= 2: with sigma = 1 the 1-D Mercer spectrum is 0.75 x 0.25^k) or
# 1.7 (D = 3), 8 at D = 64; exponential ell 2.
CASES = [
    (200, 1, 6, GAUSSIAN, 1.5, 0.0),     # well separated
    (64, 3, 5, GAUSSIAN, 1.7, 0.0),
    (65, 3, 5, GAUSSIAN, 1.7, 0.0),
    (1030, 3, 5, GAUSSIAN, 1.7, 0.0),    # two slices in rbf_apply
    (200, 64, 5, GAUSSIAN, 8.0, 0.0),
    (200, 3, 1, GAUSSIAN, 1.7, 0.0),
    (200, 3, 56, GAUSSIAN, 1.7, 0.0),    # m = 64, trailing columns are noise
    (200, 3, 64, GAUSSIAN, 1.7, 0.0),    # m = 72, second head tile
    (10, 2, 4, GAUSSIAN, 1.5, 0.0),      # m = n
    (333, 3, 10, EXPONENTIAL, 2.0, 0.0),
    (200, 2, 6, GAUSSIAN, 1.5, 100.0),   # shifted by 100
]
MAX_ITERS_GAUSSIAN, MAX_ITERS_EXPONENTIAL = 27, 29  # what recurrence (b) may take at tol = 1e-5, oversample = 8
MIN_GAP = 1e-4


def case_id(case):
    n, D, L, kind, ell, shift = case
    return f"n{n}-D{D}-L{L}-{'gauss' if kind == GAUSSIAN else 'exp'}" + ("-shift" if shift else "")


def case_points(case, nnew=40):
    """(xs (n, D), xnew (nnew, D)) float32, seeded by the shape"""
    n, D, L, kind, ell, shift = case
    g = torch.Generator().manual_seed(7 + 1000 * n + 10 * D + L)
    xs = (torch.randn(n, D, generator=g) + shift).float()
    xnew = (torch.randn(nnew, D, generator=g) + shift).float()
    return xs, xnew


def eigen_gaps(w, L):
    """relative gaps (w_k - w_{k+1}) / w_k among the first L + 1 eigenvalues (L of them; fewer when n == L)"""
    w = np.asarray(w[:L + 1], dtype=np.float64)
    return (w[:-1] - w[1:]) / w[:-1]


_SOLVED = {}


def solved(case):
    """(definition, recurrence) of a case, computed once per process and left unchanged"""
    key = case_id(case)
    if key not in _SOLVED:
        n, D, L, kind, ell, shift = case
        xs, _ = case_points(case)
        G = gram(xs, kind, ell)
        w, U = np.linalg.eigh(G)
        w, U = w[::-1].copy(), U[:, ::-1].copy()
        _SOLVED[key] = dict(G=G, w=w, U=U, rec=subspace_iteration(G, L))
    return _SOLVED[key]
