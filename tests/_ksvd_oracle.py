"""Two restatements of the truncated-SVD baseline of the kernel SVD operators (neural_svd_amd/nystrom_svd.py): the top
singular triplets of the empirical cross operator C = k(xs, ys) / sqrt(n_x n_y).

(a) ``definition``: the float64 cross Gram of tests/_pair_oracle.py (radial kinds) / tests/_dot_pair_oracle.py (dot-product
    kinds), ``np.linalg.svd`` on it, and the two projection formulas
    left(xnew) = k(xnew, ys) @ right / svals / sqrt(n_y), right(ynew) = k(ynew, xs) @ left / svals / sqrt(n_x).
(b) ``two_sided_iteration``: the two-sided block iteration the device solver runs (same steps, same stopping rule), with
    every small matrix in float64 and library svd / Cholesky in place of the device's one-sided Jacobi; ``svd_ritz_step``
    restates the small step of nsvd_svd_ritz_step_f64. ``store`` is the dtype of the n x m blocks: with float32 the
    products P = C V, R = C^T U are float32 matmuls and U, V are rounded to float32 between the steps - what the device
    does. ``short_residual`` swaps the three-term residual for Mp_kk - sigma_k^2 (exact only for an orthonormal basis and
    an H that equals U^T P exactly): the form the device does NOT use, kept to pin why.
"""
import numpy as np
import torch

from tests import _dot_pair_oracle as DP
from tests import _pair_oracle as P

GAUSSIAN, EXPONENTIAL, POLYNOMIAL, ARCCOS1 = "gauss", "exp", "poly", "arccos"
ELL = 1.5           # both radial kinds
POLY = (1.0, 1.0, 2)  # (gamma, coef0, degree): (x.y + 1)^2, rank C(D + 2, 2)


def kernel_matrix(kind, a, b):
    """k(a, b) (len(a), len(b)) float64 numpy, from the pair oracles' kernel matrices"""
    if kind in (GAUSSIAN, EXPONENTIAL):
        return P.R.radial_kernel_matrix(a, b, P.GAUSSIAN if kind == GAUSSIAN else P.EXPONENTIAL, ELL).numpy()
    if kind == POLYNOMIAL:
        return DP.DO.dot_kernel_matrix(a, b, DP.POLYNOMIAL, *POLY).numpy()
    return DP.DO.dot_kernel_matrix(a, b, DP.ARCCOS1).numpy()


def cross(kind, xs, ys):
    """C = k(xs, ys) / sqrt(n_x n_y), float64 numpy"""
    return kernel_matrix(kind, xs, ys) / np.sqrt(len(xs) * len(ys))


def definition(C, dim):
    """(svals (dim,), left (n_x, dim), right (n_y, dim), all singular values descending) of C in float64"""
    U, s, Vt = np.linalg.svd(C, full_matrices=False)
    return s[:dim].copy(), U[:, :dim].copy(), Vt[:dim].T.copy(), s.copy()


def left_functions(kind, xnew, ys, svals, right):
    """k(xnew, ys) @ right / svals / sqrt(n_y), in float64"""
    return kernel_matrix(kind, xnew, ys) @ np.asarray(right, np.float64) / np.asarray(svals, np.float64) / np.sqrt(len(ys))


def right_functions(kind, ynew, xs, svals, left):
    """k(ynew, xs) @ left / svals / sqrt(n_x), in float64"""
    return kernel_matrix(kind, ynew, xs) @ np.asarray(left, np.float64) / np.asarray(svals, np.float64) / np.sqrt(len(xs))


def _chol_rotate(X, M):
    """X chol(M)^-1 with the upper factor"""
    Rm = np.linalg.cholesky(0.5 * (M + M.T)).T
    return np.linalg.solve(Rm.T, X.T).T


def svd_ritz_step(PtU, RtV, Sp, Sr, Cu=None, Cv=None, short_residual=False):
    """the small step in float64 numpy: (sigma, resid_l, resid_r, A, B, Tu, Tv). Hl = PtU^T, Hr = RtV,
    (Hl + Hr) / 2 = A diag(sigma) B^T, Mp = B^T Sp B, Mr = A^T Sr A,
    resid_l_k^2 = Mp_kk - 2 sigma_k (A^T Hl B)_kk + sigma_k^2 (A^T Cu A)_kk = |P b_k - sigma_k U a_k|^2 and the same on the
    right with Hr, Cv (None: the identity), Tu = B chol(Mp)^-1, Tv = A chol(Mr)^-1"""
    m = Sp.shape[0]
    Hl, Hr = PtU.T, RtV
    A, sigma, Bt = np.linalg.svd(0.5 * (Hl + Hr))
    B = Bt.T
    Mp, Mr = B.T @ Sp @ B, A.T @ Sr @ A
    Cu = np.eye(m) if Cu is None else Cu
    Cv = np.eye(m) if Cv is None else Cv
    if short_residual:
        rl2, rr2 = np.diag(Mp) - sigma ** 2, np.diag(Mr) - sigma ** 2
    else:
        rl2 = np.diag(Mp) - 2.0 * sigma * np.einsum("ik,ij,jk->k", A, Hl, B) + sigma ** 2 * np.einsum("ik,ij,jk->k", A, Cu, A)
        rr2 = np.diag(Mr) - 2.0 * sigma * np.einsum("ik,ij,jk->k", A, Hr, B) + sigma ** 2 * np.einsum("ik,ij,jk->k", B, Cv, B)
    return (sigma, np.sqrt(np.maximum(rl2, 0.0)), np.sqrt(np.maximum(rr2, 0.0)), A, B, _chol_rotate(B, Mp),
            _chol_rotate(A, Mr))


def two_sided_iteration(C, dim, oversample=8, tol=1e-5, max_iters=200, seed=0, store=np.float32, short_residual=False):
    """-> dict(svals, left, right, iterations, residuals (relative: the larger side over sigma_0), converged).
    C: (n_x, n_y) float64."""
    nx, ny = C.shape
    m = min(nx, ny, dim + oversample)
    rng = np.random.default_rng(seed)

    def rnd(X):
        return X.astype(store).astype(np.float64)

    U0, V0 = rnd(rng.standard_normal((nx, m))), rnd(rng.standard_normal((ny, m)))
    U, V = rnd(_chol_rotate(U0, U0.T @ U0)), rnd(_chol_rotate(V0, V0.T @ V0))
    Cs = C.astype(store)
    it, converged = 0, False
    for it in range(1, max_iters + 1):
        Pm = (Cs @ V.astype(store)).astype(np.float64)
        Rm = (Cs.T @ U.astype(store)).astype(np.float64)
        sigma, rl, rr, A, B, Tu, Tv = svd_ritz_step(Pm.T @ U, Rm.T @ V, Pm.T @ Pm, Rm.T @ Rm, U.T @ U, V.T @ V,
                                                    short_residual)
        resid = np.maximum(rl, rr)
        if sigma[0] > 0 and resid[:dim].max() <= tol * sigma[0]:
            converged = True
            break
        if it < max_iters:
            U, V = rnd(Pm @ Tu), rnd(Rm @ Tv)
    # left64 / right64: the Ritz vectors before their rounding to `store`, the ones the claimed residuals belong to.
    # left / right: rounded, then orthonormalised once more among themselves as the device does (chol(Mp) leaves U
    # orthonormal to eps64 cond(P)^2 only - 1e-4 in the trailing columns of a dim = 56 block on a fast-decaying spectrum)
    L0, R0 = rnd(U @ A[:, :dim]), rnd(V @ B[:, :dim])
    return dict(svals=sigma[:dim].copy(), left=rnd(_chol_rotate(L0, L0.T @ L0)), right=rnd(_chol_rotate(R0, R0.T @ R0)),
                left64=U @ A[:, :dim], right64=V @ B[:, :dim], iterations=it, residuals=resid[:dim] / sigma[0],
                converged=converged)


def tsgram3_workspace_bytes(n, m):
    """three (m, m) float64 partial matrices per slice of nsvd_tsgram_f64's split rule, rounded up to 256 bytes"""
    return (max(1, min(128, (n + 63) // 64)) * 3 * m * m * 8 + 255) // 256 * 256


# ---- the solver cases shared by tests/test_ksvd_baseline_oracle.py (recurrence (b) against (a)) and
# tests/test_ksvd_baseline_gpu.py: (kind, n_x, n_y, D, dim, oversample). x ~ N(0, I), y ~ 0.5 N(0, I).
CASES = [
    (GAUSSIAN, 64, 50, 3, 5, 8),
    (GAUSSIAN, 257, 130, 3, 5, 8),
    (EXPONENTIAL, 257, 130, 3, 5, 8),
    (ARCCOS1, 257, 130, 3, 5, 8),
    (GAUSSIAN, 1030, 515, 3, 5, 8),      # more than one row group and column slice in the pair product
    (EXPONENTIAL, 130, 257, 2, 10, 8),   # n_x < n_y, m = 18
    (GAUSSIAN, 300, 300, 16, 10, 8),     # the slowest: a flat spectrum
    (POLYNOMIAL, 200, 150, 3, 4, 4),     # rank 10: m = 8 <= rank
    (GAUSSIAN, 10, 7, 2, 4, 8),          # m = n_y
    (GAUSSIAN, 200, 200, 3, 1, 8),
    (GAUSSIAN, 200, 120, 3, 56, 8),      # m = 64, trailing columns are noise
    (GAUSSIAN, 200, 120, 3, 64, 8),      # m = 72, second head tile
]
SLOWEST = CASES[6]
MIN_GAP = 0.005


def case_id(case):
    kind, nx, ny, D, dim, over = case
    return f"{kind}-nx{nx}-ny{ny}-D{D}-L{dim}"


def case_points(case, nnew=40):
    """(xs (n_x, D), ys (n_y, D), xnew (nnew, D), ynew (nnew, D)) float32, seeded by the shape"""
    kind, nx, ny, D, dim, over = case
    g = torch.Generator().manual_seed(11 + 1000 * nx + 10 * ny + D + dim)
    xs, ys = torch.randn(nx, D, generator=g).float(), (0.5 * torch.randn(ny, D, generator=g)).float()
    xnew, ynew = torch.randn(nnew, D, generator=g).float(), (0.5 * torch.randn(nnew, D, generator=g)).float()
    return xs, ys, xnew, ynew


def relative_gaps(s, dim):
    """per column k < dim: the distance to the nearer neighbouring singular value over s_k (the value after the last
    column is s_dim, or 0 when the matrix has no more)"""
    s = np.asarray(s, dtype=np.float64)
    ext = np.append(s, 0.0)
    below = ext[:dim] - ext[1:dim + 1]
    above = np.append(np.inf, s[:dim - 1] - s[1:dim])
    return np.minimum(below, above) / s[:dim]


_SOLVED = {}


def solved(case):
    """(definition, recurrence) of a case, computed once per process and left unchanged"""
    key = case_id(case)
    if key not in _SOLVED:
        kind, nx, ny, D, dim, over = case
        xs, ys, _, _ = case_points(case)
        C = cross(kind, xs, ys)
        s, U, V, s_all = definition(C, dim)
        _SOLVED[key] = dict(C=C, s=s, U=U, V=V, s_all=s_all, rec=two_sided_iteration(C, dim, over))
    return _SOLVED[key]
