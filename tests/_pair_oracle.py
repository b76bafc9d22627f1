"""Float64 restatements for the kernel SVD path (nsvd_rbf_apply_pair, neural_svd_amd/kernel_svd.py):

- ``radial_kernel_apply_pair``: out_x = scale_g * K g, out_y = scale_f * K^T f with K = k(|x_i - y_j|) from direct
  differences (tests/_rbf_oracle.py's kernel matrix);
- ``quadrature_singular_values``: the singular values of k = exp(-(x - y)^2 / (2 ell^2)) as an operator from
  L2(N(0, sigma_y^2)) to L2(N(0, sigma_x^2)) by Gauss-Hermite quadrature on both sides (the SVD of
  diag(sqrt w_x) K diag(sqrt w_y));
- ``svd_step``: loss, d loss / d f, d loss / d g of NestedLoRALossFunctionSVD from the formulas in its docstring
  (neural_svd_amd/nested_lowrank.py);
- ``pair_split`` / ``pair_workspace_bytes``: the partition rule and workspace layout of csrc/rbf_apply_pair.hip."""
import numpy as np
import torch

from tests import _rbf_oracle as R

GAUSSIAN, EXPONENTIAL = R.GAUSSIAN, R.EXPONENTIAL


def radial_kernel_apply_pair(x, y, g, f, kind, ell, scale_g, scale_f):
    K = R.radial_kernel_matrix(x, y, kind, ell)
    return scale_g * (K @ torch.as_tensor(g).double()), scale_f * (K.T @ torch.as_tensor(f).double())


def quadrature_singular_values(sigma_x, sigma_y, ell, n, points=160):
    t, w = np.polynomial.hermite.hermgauss(points)
    xs, ys = np.sqrt(2.0) * sigma_x * t, np.sqrt(2.0) * sigma_y * t
    wq = w / np.sqrt(np.pi)
    K = np.exp(-(xs[:, None] - ys[None, :]) ** 2 / (2.0 * ell ** 2))
    A = np.sqrt(wq)[:, None] * K * np.sqrt(wq)[None, :]
    return np.linalg.svd(A, compute_uv=False)[:n]


def svd_step(f, Tg, g, Tadjf, v, M):
    """(loss, d loss / d f, d loss / d g), everything float64 torch; v: (L,), M: (L, L)"""
    f, Tg, g, Tadjf, v, M = (torch.as_tensor(t).double() for t in (f, Tg, g, Tadjf, v, M))
    B1, B2 = f.shape[0], g.shape[0]
    lam_f, lam_g = f.T @ f / B1, g.T @ g / B2
    loss = -2.0 * (v * f * Tg).sum(dim=1).mean() + (M * lam_f * lam_g).sum()
    df = -(2.0 / B1) * v * Tg + (2.0 / B1) * f @ (M * lam_g)
    dg = -(2.0 / B2) * v * Tadjf + (2.0 / B2) * g @ (M * lam_f)
    return loss, df, dg


PAIR_SLICE, PAIR_MAX_GROUPS, PAIR_FILL = 4, 32, 512


def pair_split(B1, B2, L):
    """(row groups, column slices) - csrc/pair_common.h:pair_split: runs of 64-row x tiles and runs of slices of
    four 64-row y chunks; whichever side has more items per group is halved until head tiles * groups reach 512
    workgroups or both sides are at one item per group or at 32 groups"""
    xt, sl, lt = (B1 + 63) // 64, ((B2 + 63) // 64 + PAIR_SLICE - 1) // PAIR_SLICE, (L + 63) // 64
    rg = cg = 1
    rmax, cmax = min(xt, PAIR_MAX_GROUPS), min(sl, PAIR_MAX_GROUPS)
    while lt * rg * cg < PAIR_FILL:
        can_r, can_c = 2 * rg <= rmax, 2 * cg <= cmax
        if not can_r and not can_c:
            break
        if can_r and (not can_c or xt * cg >= sl * rg):
            rg *= 2
        else:
            cg *= 2
    return rg, cg


def pair_workspace_bytes(B1, B2, D, L):
    def up(n, m):
        return (n + m - 1) // m * m
    B1p, B2p, Dp, Lp = up(B1, 64), up(B2, 64), up(D, 4), up(L, 64)
    rg, cg = pair_split(B1, B2, L)
    return sum(up(4 * n, 256) for n in (B2p * Dp, Lp * B2p, Lp * B1p, cg * B1p * Lp, rg * B2p * Lp))
