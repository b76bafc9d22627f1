"""Float64 restatement of the radial kernel operator (nsvd_rbf_apply, neural_svd_amd/kernel_ops.RadialKernelOperator):
out[i] = scale * sum_j k(|x_i - y_j|) f[j], distances by direct differences. Its Gaussian kind with scale = 1 / B2 is
oracle/nsvd_oracle.py:gaussian_kernel_apply (tests/test_rbf_oracle.py), the definition tests/golden/kernel_loss.npz pins."""
import torch

GAUSSIAN, EXPONENTIAL = 0, 1


def radial_kernel_matrix(x, y, kind, ell):
    x, y = torch.as_tensor(x).double(), torch.as_tensor(y).double()
    d2 = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    if kind == GAUSSIAN:
        return torch.exp(-d2 / (2.0 * ell ** 2))
    if kind == EXPONENTIAL:
        return torch.exp(-d2.sqrt() / ell)
    raise ValueError(kind)


def radial_kernel_apply(x, y, f, kind, ell, scale):
    return scale * (radial_kernel_matrix(x, y, kind, ell) @ torch.as_tensor(f).double())


def split_slices(B1, B2, L):
    """nsvd_rbf_apply's split rule (csrc/rbf_apply.hip:carve): 64 x 64 output tiles, the reference rows in chunks of
    64; the slice count doubles while there are fewer than 512 workgroups and a slice keeps at least 8 chunks."""
    tiles = ((B1 + 63) // 64) * ((L + 63) // 64)
    chunks = (B2 + 63) // 64
    S = 1
    while tiles * S < 512 and chunks // (2 * S) >= 8:
        S *= 2
    return S


def workspace_bytes(B1, B2, D, L):
    """the workspace layout of the same function: padded y, f^T and S partial tiles, each rounded up to 256 bytes"""
    def up(n, m):
        return (n + m - 1) // m * m
    B1p, B2p, Dp, Lp = up(B1, 64), up(B2, 64), up(D, 4), up(L, 64)
    return sum(up(4 * n, 256) for n in (B2p * Dp, Lp * B2p, split_slices(B1, B2, L) * B1p * Lp))
