"""Float64 restatement of the two-sided dot-product kernel operator (nsvd_dot_apply_pair,
kernel_ops.DotKernelOperator.apply_pair_raw): out_x = scale_g * K g and out_y = scale_f * K^T f with K from
tests/_dot_oracle.py:dot_kernel_matrix, and the partition rule and workspace layout of csrc/dot_apply_pair.hip (the
rule is csrc/pair_common.h's, restated by tests/_pair_oracle.py:pair_split: the slice length is unchanged)."""
import torch

from tests import _dot_oracle as DO
from tests._pair_oracle import pair_split  # noqa: F401  (the same rule, the same slice length)

POLYNOMIAL, ARCCOS1 = DO.POLYNOMIAL, DO.ARCCOS1


def dot_kernel_apply_pair(x, y, g, f, kind, gamma, coef0, degree, scale_g, scale_f):
    K = DO.dot_kernel_matrix(x, y, kind, gamma, coef0, degree)
    return scale_g * (K @ torch.as_tensor(g).double()), scale_f * (K.T @ torch.as_tensor(f).double())


def pair_workspace_bytes(B1, B2, D, L):
    """padded x and |x|, padded y and |y| (D rounded up to 8, the first contraction's step), g^T, f^T and the partial
    copies of both outputs, each rounded up to 256 bytes"""
    def up(n, m):
        return (n + m - 1) // m * m
    B1p, B2p, Dp, Lp = up(B1, 64), up(B2, 64), up(D, 8), up(L, 64)
    rg, cg = pair_split(B1, B2, L)
    return sum(up(4 * n, 256) for n in (B1p * Dp, B1p, B2p * Dp, B2p, Lp * B2p, Lp * B1p, cg * B1p * Lp, rg * B2p * Lp))
