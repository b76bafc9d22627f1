"""Kernel operators for ``NestedLoRA.compute_loss_kernel`` (methods/nestedlora.py:230-252).

The reference defines only the consumer contract - ``get_approx_kernel_op(x)(model, x, importance) -> (Kf, f)`` - and
ships no kernel operator. This module provides the dense one of the kernel-operator configuration (SURVEY.md 8,
cfg4): a fixed symmetric PSD matrix K on N points z_j, minibatches are point INDICES drawn with replacement,

    f  = model(x) = net(z[x]),        Kf = K[x][:, x_ref] @ model(x_ref) / len(x_ref)

(the model handed to NestedLoRA takes indices: ``op.index_model(net)`` wraps a coordinate network, so that the
contract's own ``self.model(x2)`` call works on an index batch),

with the (B x B) . (B x L) contraction done by ``nsvd_kernel_apply`` on the fp32 MFMA (gathered rows of K, the batch
scattered into the index space). No gradient flows through Kf (the EVD loss function returns none for it).

``RadialKernelOperator`` is the matrix-free one: a radial kernel k(|x - y|) (Gaussian or exponential) on COORDINATE
batches drawn fresh every step,

    f = model(x),        Kf(x_i) = (1 / B2) sum_j k(|x_i - x_ref_j|) model(x_ref)_j

- the definition oracle/nsvd_oracle.py:gaussian_kernel_apply restates and tests/golden/kernel_loss.npz pins - through
``nsvd_rbf_apply``, which never stores the (B, B2) kernel matrix. Under the Gaussian measure N(0, sigma^2 I) the
Gaussian kernel's Mercer spectrum is known in closed form (``gaussian_kernel_eigvals`` / ``_eigenfunctions``), and
``kernel_spectrum`` evaluates the Rayleigh quotients of any functions against it on a sample.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import hip_ops as H


class IndexedModel(nn.Module):
    """model(idx) = net(points[idx]): lets a coordinate network consume minibatches of point indices."""

    def __init__(self, net: nn.Module, points: torch.Tensor):
        super().__init__()
        self.net = net
        self.register_buffer("points", points, persistent=False)

    def forward(self, idx):
        return self.net(self.points[idx.to(torch.int64)])


class DenseKernelOperator:
    """K: (N, N) float32 symmetric PSD; points: (N, D) coordinates the model is evaluated at."""

    def __init__(self, K: torch.Tensor, points: torch.Tensor):
        if K.dim() != 2 or K.shape[0] != K.shape[1] or points.shape[0] != K.shape[0]:
            raise ValueError("K must be (N, N) and points (N, D)")
        if not K.is_cuda:
            raise H.NsvdError("DenseKernelOperator: K must live on the GPU (no CPU path)")
        N = K.shape[0]
        ld = (N + 63) // 64 * 64
        self.N = N
        # rows are read in whole 64-float chunks: keep a zero-padded copy with a leading dimension of ceil64(N)
        self.K = torch.zeros((N, ld), dtype=torch.float32, device=K.device)
        self.K[:, :N] = K.float()
        self.points = points.to(K.device).float().contiguous()

    def get_approx_kernel_op(self, x_ref: torch.Tensor):
        """x_ref: (B2,) int64 indices of the reference batch -> op(model, x, importance=None) -> (Kf, f)."""
        x_ref = x_ref.to(torch.int64).contiguous()

        def op(model, x, importance=None):
            if importance is not None:
                raise NotImplementedError("DenseKernelOperator: importance weights are not defined for an index batch")
            x = x.to(torch.int64).contiguous()
            f = model(x)  # an index model (index_model below)
            same = x.data_ptr() == x_ref.data_ptr() and x.numel() == x_ref.numel()
            with torch.no_grad():
                f_ref = f.detach() if same else model(x_ref).detach()
                Kf = H.kernel_apply(self.K, self.N, x, x_ref, f_ref.contiguous(), 1.0 / x_ref.numel())
            return Kf, f
        return op

    def index_model(self, net: nn.Module) -> IndexedModel:
        return IndexedModel(net, self.points)

    def sample_indices(self, batch_size: int, generator=None) -> torch.Tensor:
        return torch.randint(self.N, (batch_size,), device=self.K.device, generator=generator)


class IndexColumnModel(nn.Module):
    """model(idx) = net(points[idx]) for an index batch (B,) or (B, 1): the column form is how index batches travel
    through ``NestedLoRA.compute_loss_kernel_svd``, which insists on 2-D batches."""

    def __init__(self, net: nn.Module, points: torch.Tensor):
        super().__init__()
        self.net = net
        self.register_buffer("points", points, persistent=False)

    def forward(self, idx):
        return self.net(self.points.index_select(0, _flat_indices(idx, "IndexColumnModel")))


def _flat_indices(idx: torch.Tensor, who: str) -> torch.Tensor:
    """an index batch (B,) or (B, 1) as contiguous 1-D int64 on the GPU; anything else raises"""
    if not idx.is_cuda:
        raise H.NsvdError(f"{who}: index batches must live on the GPU (no CPU path)")
    if idx.dim() == 2 and idx.shape[1] == 1:
        idx = idx[:, 0]
    if idx.dim() != 1 or idx.dtype not in (torch.int64, torch.int32):
        raise H.NsvdError(f"{who}: an index batch is (B,) or (B, 1) of integers (got {tuple(idx.shape)} {idx.dtype})")
    return idx.to(torch.int64).contiguous()


class DenseCrossOperator:
    """A: (N1, N2) float32, any values (rectangular, not symmetric): a stored matrix between N1 row points
    ``points_x`` (N1, Dx) and N2 column points ``points_y`` (N2, Dy), as an operator from functions of the column points
    to functions of the row points under the UNIFORM measures on both,

        (A g)(i) = (1 / N2) sum_j A[i][j] g(j),

    whose singular values are ``svdvals(A) / sqrt(N1 N2)``. Minibatches are point INDICES drawn with replacement, rows
    and columns apart; the two-sided product of an SVD step is one ``nsvd_kernel_apply_pair`` call on the zero-padded
    copy kept here (lda = ceil64(N2)) - no transposed copy exists. ``kernel_svd.DenseSvdTrainer`` trains on it; the
    class path is ``NestedLoRA.compute_loss_kernel_svd(op.get_approx_kernel_svd_op(), idx_x[:, None], idx_y[:, None])``
    on ``op.index_models(f_net, g_net)``."""

    def __init__(self, A: torch.Tensor, points_x: torch.Tensor, points_y: torch.Tensor):
        if A.dim() != 2 or points_x.dim() != 2 or points_y.dim() != 2 or points_x.shape[0] != A.shape[0] or \
                points_y.shape[0] != A.shape[1]:
            raise ValueError("DenseCrossOperator: A must be (N1, N2), points_x (N1, Dx) and points_y (N2, Dy)")
        if not A.is_cuda:
            raise H.NsvdError("DenseCrossOperator: A must live on the GPU (no CPU path)")
        self.N1, self.N2 = int(A.shape[0]), int(A.shape[1])
        self.device = A.device
        ld = (self.N2 + 63) // 64 * 64
        # rows are read in whole 64-float chunks: a zero-padded copy with a leading dimension of ceil64(N2)
        self.A = torch.zeros((self.N1, ld), dtype=torch.float32, device=A.device)
        self.A[:, :self.N2] = A.float()
        self.points_x = points_x.to(A.device).float().contiguous()
        self.points_y = points_y.to(A.device).float().contiguous()
        self.dim_x, self.dim_y = int(points_x.shape[1]), int(points_y.shape[1])

    def sample_indices(self, batch_size: int, generator=None):
        """(idx_x, idx_y): `batch_size` row indices and as many column indices, drawn with replacement"""
        return (torch.randint(self.N1, (batch_size,), device=self.device, generator=generator),
                torch.randint(self.N2, (batch_size,), device=self.device, generator=generator))

    def workspace_pair(self, B1: int, B2: int, L: int, device=None) -> torch.Tensor:
        return H.kernel_apply_pair_workspace(self.N1, self.N2, B1, B2, L, self.device if device is None else device)

    def apply_pair_raw(self, rows, cols, g, f, scale_g, scale_f, ws=None, out_x=None, out_y=None):
        """(out_x, out_y) = (scale_g * A[rows][:, cols] @ g, scale_f * A[rows][:, cols]^T @ f): one
        nsvd_kernel_apply_pair call, no gradient. rows (B1,), cols (B2,) int64; g: (B2, L), f: (B1, L)."""
        return H.kernel_apply_pair(self.A, self.N1, self.N2, rows, cols, g, f, scale_g, scale_f, ws=ws, out_x=out_x,
                                   out_y=out_y)

    def index_models(self, f_net: nn.Module, g_net: nn.Module):
        """the PairedFunctions of index wrappers: .f takes row indices, .g column indices, (B,) or (B, 1)"""
        from .kernel_svd import PairedFunctions
        return PairedFunctions(IndexColumnModel(f_net, self.points_x), IndexColumnModel(g_net, self.points_y))

    def get_approx_kernel_svd_op(self):
        """-> svd_op(model_f, model_g, x, y, importance=None) -> (Tg, f, Tadjf, g), the arguments of
        NestedLoRALossFunctionSVD: x, y index batches ((B,) or (B, 1)), f = model_f(x) and g = model_g(y) differentiable
        (index models: ``index_models``), Tg = A[x][:, y] g / B2 and Tadjf = A[x][:, y]^T f / B1 without gradient."""
        def svd_op(model_f, model_g, x, y, importance=None):
            if importance is not None:
                raise NotImplementedError("DenseCrossOperator: importance weights are not defined for an index batch")
            rows, cols = _flat_indices(x, "DenseCrossOperator: x"), _flat_indices(y, "DenseCrossOperator: y")
            f, g = model_f(x), model_g(y)
            with torch.no_grad():
                Tg, Tadjf = self.apply_pair_raw(rows, cols, g.detach().float().contiguous(),
                                                f.detach().float().contiguous(), 1.0 / cols.numel(), 1.0 / rows.numel())
            return Tg, f, Tadjf, g
        return svd_op

    @torch.no_grad()
    def quotients(self, model_f, model_g):
        """Singular-value estimates of the column pairs of F = model_f(points_x) (N1, L) and G = model_g(points_y)
        (N2, L), coordinate models evaluated on ALL points:
        s_l = (F_l^T A G_l / (N1 N2)) / sqrt((|F_l|^2 / N1) (|G_l|^2 / N2)), with A G from one nsvd_kernel_apply_pair
        call at rows = arange(N1), cols = arange(N2) and the column sums in float64. Returns dict(svals, norms_f,
        norms_g) of float64 numpy arrays - the counterpart of ``kernel_singular_values``; compare with
        ``svdvals(A) / sqrt(N1 N2)``."""
        F = model_f(self.points_x).float().contiguous()
        G = model_g(self.points_y).float().contiguous()
        if F.dim() != 2 or G.dim() != 2 or F.shape[0] != self.N1 or G.shape[0] != self.N2 or F.shape[1] != G.shape[1]:
            raise H.NsvdError("DenseCrossOperator.quotients: the models must return (N1, L) and (N2, L)")
        rows = torch.arange(self.N1, device=self.device)
        cols = torch.arange(self.N2, device=self.device)
        AG, _ = self.apply_pair_raw(rows, cols, G, F, 1.0 / self.N2, 1.0 / self.N1)
        F64 = F.double()
        cross = (F64 * AG.double()).sum(0) / self.N1
        nf, ng = (F64 * F64).sum(0) / self.N1, (G.double() ** 2).sum(0) / self.N2
        return dict(svals=(cross / torch.sqrt(nf * ng)).cpu().numpy(), norms_f=nf.cpu().numpy(),
                    norms_g=ng.cpu().numpy())


def synthetic_psd_kernel(N: int = 10000, rank: int = 256, dim: int = 16, seed: int = 0, device="cuda:0"):
    """cfg4's operator: z_j ~ N(0, I_dim), K = A A^T / rank + 1e-3 I with A ~ randn(N, rank); seeded on the host."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, dim, generator=g)
    A = torch.randn(N, rank, generator=g).to(device)
    K = A @ A.T / rank
    K.diagonal().add_(1e-3)
    return DenseKernelOperator(K, z.to(device))


class MatrixFreeKernelOperator:
    """What ``kernel_spectrum``, ``FusedKernelTrainer`` and ``nystrom.Nystrom`` need of a matrix-free operator on
    `dim`-dimensional coordinates (attributes ``dim``, ``sigma``, ``device``): a subclass supplies

        workspace(B1, B2, L, device=None)             the workspace of one product of that shape (on `device`;
                                                      None: the operator's own)
        apply_raw(x, y, f, scale, ws=None, out=None)  out = scale * k(x, y) @ f, one C-ABI call, no gradient

    and inherits ``apply`` (scale = 1 / B2), the consumer contract ``get_approx_kernel_op`` and ``sample``.

    The two-sided product of a kernel SVD step (``kernel_svd``) - out_x = scale_g k(x, y) g and
    out_y = scale_f k(x, y)^T f - is ``apply_pair_raw`` with ``workspace_pair``: here two ``apply_raw`` calls with the
    arguments swapped (k(y, x) = k(x, y)^T for every kernel this class serves), which a subclass may replace by one
    call; ``get_approx_kernel_svd_op`` is its consumer contract."""

    def _init_common(self, dim: int, sigma: float, device, entry: str):
        name = type(self).__name__
        if not 1 <= int(dim) <= 64:
            raise H.NsvdError(f"{name}: unsupported input dimension ({entry} takes 1 <= D <= 64)")
        self.dim, self.sigma = int(dim), float(sigma)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise H.NsvdError(f"{name}: the operator lives on the GPU (no CPU path)")

    def workspace(self, B1: int, B2: int, L: int, device=None) -> torch.Tensor:
        raise NotImplementedError

    def apply_raw(self, x, y, f, scale, ws=None, out=None) -> torch.Tensor:
        raise NotImplementedError

    def apply(self, x: torch.Tensor, x_ref: torch.Tensor, f_ref: torch.Tensor, ws=None, out=None) -> torch.Tensor:
        """Kf = (1 / B2) k(x, x_ref) @ f_ref, (B, L) float32; no gradient."""
        with torch.no_grad():
            return self.apply_raw(x, x_ref, f_ref, 1.0 / x_ref.shape[0], ws=ws, out=out)

    def get_approx_kernel_op(self, x_ref: torch.Tensor):
        """x_ref: (B2, dim) reference coordinates -> op(model, x, importance=None) -> (Kf, f)."""
        name = type(self).__name__
        if not x_ref.is_cuda:
            raise H.NsvdError(f"{name}: x_ref must live on the GPU (no CPU path)")
        y = x_ref.detach().float().contiguous()

        def op(model, x, importance=None):
            if importance is not None:
                raise NotImplementedError(f"{name}: importance-weighted kernel operators are not built")
            if not x.is_cuda:
                raise H.NsvdError(f"{name}: x must live on the GPU (no CPU path)")
            f = model(x)
            same = x is x_ref or (x.data_ptr() == x_ref.data_ptr() and x.shape == x_ref.shape and
                                  x.stride() == x_ref.stride() and x.dtype == x_ref.dtype)
            with torch.no_grad():
                f_ref = f.detach() if same else model(x_ref).detach()
                Kf = self.apply(x.detach().float().contiguous(), y, f_ref.float().contiguous())
            return Kf, f
        return op

    def sample(self, batch_size: int, generator=None) -> torch.Tensor:
        return self.sigma * torch.randn(batch_size, self.dim, device=self.device, generator=generator)

    def workspace_pair(self, B1: int, B2: int, L: int, device=None) -> torch.Tensor:
        """the workspace of one apply_pair_raw of that shape: here the larger of the two products' (used in turn; the
        two sizes are compared on the meta device, one buffer is allocated)"""
        a, b = self.workspace(B1, B2, L, "meta").numel(), self.workspace(B2, B1, L, "meta").numel()
        return self.workspace(B1, B2, L, device) if a >= b else self.workspace(B2, B1, L, device)

    def apply_pair_raw(self, x, y, g, f, scale_g, scale_f, ws=None, out_x=None, out_y=None):
        """(out_x, out_y) = (scale_g * k(x, y) @ g, scale_f * k(x, y)^T @ f): (B1, L) and (B2, L), no gradient.
        x: (B1, dim), y: (B2, dim), g: (B2, L), f: (B1, L)."""
        out_x = self.apply_raw(x, y, g, scale_g, ws=ws, out=out_x)
        out_y = self.apply_raw(y, x, f, scale_f, ws=ws, out=out_y)
        return out_x, out_y

    def get_approx_kernel_svd_op(self):
        """-> svd_op(model_f, model_g, x, y, importance=None) -> (Tg, f, Tadjf, g), the arguments of
        NestedLoRALossFunctionSVD: f = model_f(x) and g = model_g(y) differentiable,
        Tg = k(x, y) g / B2 and Tadjf = k(x, y)^T f / B1 without gradient (one apply_pair_raw)."""
        name = type(self).__name__

        def svd_op(model_f, model_g, x, y, importance=None):
            if importance is not None:
                raise NotImplementedError(f"{name}: importance-weighted kernel operators are not built")
            if not x.is_cuda or not y.is_cuda:
                raise H.NsvdError(f"{name}: x and y must live on the GPU (no CPU path)")
            f, g = model_f(x), model_g(y)
            with torch.no_grad():
                Tg, Tadjf = self.apply_pair_raw(x.detach().float().contiguous(), y.detach().float().contiguous(),
                                                g.detach().float().contiguous(), f.detach().float().contiguous(),
                                                1.0 / y.shape[0], 1.0 / x.shape[0])
            return Tg, f, Tadjf, g
        return svd_op


class RadialKernelOperator(MatrixFreeKernelOperator):
    """k(x, y) = exp(-|x - y|^2 / (2 ell^2)) (kind H.RBF_GAUSSIAN) or exp(-|x - y| / ell) (H.RBF_EXPONENTIAL) on
    `dim`-dimensional coordinates; training batches are sigma * randn(B, dim). Serves NestedLoRA.compute_loss_kernel
    and NeuralEigenfunctions.compute_loss_kernel in both split_batch modes: the models take coordinates as they are."""

    def __init__(self, kind: int, ell: float, dim: int, sigma: float = 1.0, device="cuda:0"):
        if kind not in (H.RBF_GAUSSIAN, H.RBF_EXPONENTIAL):
            raise ValueError("RadialKernelOperator: kind must be H.RBF_GAUSSIAN or H.RBF_EXPONENTIAL")
        if not ell > 0 or not sigma > 0:
            raise ValueError("RadialKernelOperator: ell and sigma must be positive")
        self.kind, self.ell = int(kind), float(ell)
        self._init_common(dim, sigma, device, "nsvd_rbf_apply")

    def workspace(self, B1: int, B2: int, L: int, device=None) -> torch.Tensor:
        return H.rbf_apply_workspace(B1, B2, self.dim, L, self.device if device is None else device)

    def apply_raw(self, x, y, f, scale, ws=None, out=None) -> torch.Tensor:
        return H.rbf_apply(x, y, f, self.kind, self.ell, scale, ws=ws, out=out)

    def workspace_pair(self, B1: int, B2: int, L: int, device=None) -> torch.Tensor:
        """nsvd_rbf_apply_pair_workspace_bytes. With B1p, B2p, Lp = B1, B2, L rounded up to 64, Dp = dim rounded up to 4
        and (RG, CG) = hip_ops.rbf_apply_pair_partition(B1, B2, dim, L), both at most 32:
        4 * (B2p Dp + Lp (B1p + B2p) + CG B1p Lp + RG B2p Lp) bytes, each term rounded up to 256 - the partial copies
        dominate: 100 MiB at B1 = B2 = 8192, L = 64 (RG, CG = 32, 16), about 0.8 GiB at 65 536 rows a side."""
        return H.rbf_apply_pair_workspace(B1, B2, self.dim, L, self.device if device is None else device)

    def apply_pair_raw(self, x, y, g, f, scale_g, scale_f, ws=None, out_x=None, out_y=None):
        """one nsvd_rbf_apply_pair call: every kernel value evaluated once for both products"""
        return H.rbf_apply_pair(x, y, g, f, self.kind, self.ell, scale_g, scale_f, ws=ws, out_x=out_x, out_y=out_y)


def _is_relu_kind(kind) -> bool:
    return kind in (H.DOT_RELU_NNGP, H.DOT_RELU_NTK)


def relu_kernel_diagonal(kind: int, r2, gamma: float, coef0: float, depth: int) -> np.ndarray:
    """k(x, x) of the deep ReLU kinds in closed form from r2 = |x|^2, float64 numpy: q_0 = r2,
    q_l = gamma q_{l-1} + coef0; H.DOT_RELU_NNGP: q_depth, H.DOT_RELU_NTK: sum over l = 0 .. depth of
    gamma^(depth - l) q_l (T_l(x, x) = q_l + gamma T_{l-1}(x, x): A1(1) = A0(1) = 1). A zero row needs no case of its
    own: where the kernel takes both A terms as 0, T_{l-1} is 0 as well."""
    if not _is_relu_kind(kind):
        raise ValueError("relu_kernel_diagonal: kind must be H.DOT_RELU_NNGP or H.DOT_RELU_NTK")
    if int(depth) != depth or not 1 <= int(depth) <= 8:
        raise ValueError("relu_kernel_diagonal: depth must be an integer in 1..8")
    q = np.asarray(r2, dtype=np.float64).copy()
    t = q.copy()
    for _ in range(int(depth)):
        q = float(gamma) * q + float(coef0)
        t = q + float(gamma) * t
    return q if kind == H.DOT_RELU_NNGP else t


class DotKernelOperator(MatrixFreeKernelOperator):
    """A kernel of the inner product on `dim`-dimensional coordinates (nsvd_dot_apply: x.y on the fp32 MFMA, the
    (B, B2) matrix never stored): kind H.DOT_POLYNOMIAL k = (gamma x.y + coef0)^degree with an integer degree in 1..8, or
    H.DOT_ARCCOS1 k = |x||y| / pi (sin t + (pi - t) cos t), cos t = x.y / (|x||y|) - Cho & Saul's order-1 arc-cosine
    kernel, the NNGP kernel of one ReLU layer (gamma, coef0, degree unused). Training batches are sigma * randn(B, dim);
    the same contract and callers as RadialKernelOperator. Polynomial kind: gamma <= 0 or coef0 < 0 are refused (not PSD
    in general).
    A polynomial kernel has FINITE rank C(dim + degree, degree) (see nystrom.Nystrom's note on ``oversample``).
    The two-sided product of a kernel SVD step is one nsvd_dot_apply_pair call (``apply_pair_raw``).

    H.DOT_RELU_NNGP and H.DOT_RELU_NTK are the NNGP kernel and the neural tangent kernel of a ReLU network ``depth``
    layers deep (an integer in 1..8, ``op.depth``; ``degree`` is ignored) with weight variance gamma > 0 and bias
    variance coef0 >= 0. With A1(c) = (sin t + (pi - t) cos t) / pi and A0(c) = (pi - t) / pi, cos t = c clamped to
    [-1, 1] (Cho & Saul's orders 1 and 0; A1 = 2 E[relu u relu v], A0 = 2 E[1{u>0} 1{v>0}] for unit Gaussians of
    correlation c), S_0 = T_0 = x.y, q_0(x) = |x|^2, and for l = 1 .. depth

        p = sqrt(q_{l-1}(x) q_{l-1}(y)),   c = S_{l-1} / p,   S_l = gamma p A1(c) + coef0,
        T_l = S_l + gamma T_{l-1} A0(c),   q_l(x) = gamma q_{l-1}(x) + coef0   (= S_l(x, x)),

    the NNGP kind is k = S_depth and the NTK kind k = T_depth (diagonals: ``relu_kernel_diagonal``). Two conventions:
    S_0 is x.y itself (no variance on the input layer), and where p = 0 - a zero row at level 1, at every level when
    coef0 = 0 - both A terms are taken as 0, so S_l = T_l = coef0. gamma = 1, coef0 = 0, depth = 1 makes the NNGP kind
    H.DOT_ARCCOS1. Both are positive semi-definite. The NTK kind inherits A0's unbounded slope at c = +-1: float32
    leaves about 2e-4 per level on the diagonal of a Gram, on near-parallel rows and on every pair at dim = 1
    (include/nsvd.h); the NNGP kind is as well conditioned as H.DOT_ARCCOS1."""

    def __init__(self, kind: int, dim: int, *, gamma: float = 1.0, coef0: float = 1.0, degree: int = 2,
                 depth: int = 1, sigma: float = 1.0, device="cuda:0"):
        if kind not in (H.DOT_POLYNOMIAL, H.DOT_ARCCOS1, H.DOT_RELU_NNGP, H.DOT_RELU_NTK):
            raise ValueError("DotKernelOperator: kind must be H.DOT_POLYNOMIAL, H.DOT_ARCCOS1, H.DOT_RELU_NNGP or "
                             "H.DOT_RELU_NTK")
        if kind == H.DOT_POLYNOMIAL:  # (the arc-cosine kind ignores the three, as the C entry point does)
            if not (gamma > 0 and math.isfinite(gamma)) or not (coef0 >= 0 and math.isfinite(coef0)):
                raise ValueError("DotKernelOperator: gamma must be positive and coef0 non-negative (and finite): "
                                 "the kernel is not positive semi-definite otherwise")
            if int(degree) != degree or not 1 <= int(degree) <= 8:
                raise ValueError("DotKernelOperator: degree must be an integer in 1..8")
            depth = 1
        elif _is_relu_kind(kind):
            if not (gamma > 0 and math.isfinite(gamma)) or not (coef0 >= 0 and math.isfinite(coef0)):
                raise ValueError("DotKernelOperator: gamma (the weight variance) must be positive and coef0 (the bias "
                                 "variance) non-negative, both finite")
            if not isinstance(depth, (int, float, np.integer, np.floating)) or not math.isfinite(depth) or \
                    int(depth) != depth or not 1 <= int(depth) <= 8:
                raise ValueError("DotKernelOperator: depth must be an integer in 1..8")
            degree = 2
        else:
            gamma, coef0, degree, depth = 1.0, 1.0, 2, 1
        if not sigma > 0:
            raise ValueError("DotKernelOperator: sigma must be positive")
        self.kind, self.gamma, self.coef0, self.degree = int(kind), float(gamma), float(coef0), int(degree)
        self.depth = int(depth)
        # what the entry points take in their degree slot: the deep ReLU kinds read their depth there
        self._slot = self.depth if _is_relu_kind(self.kind) else self.degree
        self._init_common(dim, sigma, device, "nsvd_dot_apply")

    def workspace(self, B1: int, B2: int, L: int, device=None) -> torch.Tensor:
        return H.dot_apply_workspace(B1, B2, self.dim, L, self.device if device is None else device)

    def apply_raw(self, x, y, f, scale, ws=None, out=None) -> torch.Tensor:
        return H.dot_apply(x, y, f, self.kind, self.gamma, self.coef0, self._slot, scale, ws=ws, out=out)

    def workspace_pair(self, B1: int, B2: int, L: int, device=None) -> torch.Tensor:
        """nsvd_dot_apply_pair_workspace_bytes. With B1p, B2p, Lp = B1, B2, L rounded up to 64, Dp = dim rounded up to 8
        and (RG, CG) = hip_ops.dot_apply_pair_partition(B1, B2, dim, L), both at most 32:
        4 * (B1p Dp + B1p + B2p Dp + B2p + Lp (B2p + B1p) + CG B1p Lp + RG B2p Lp) bytes, each term rounded up to 256
        (padded x, |x|, padded y, |y|, g^T, f^T and the partial copies, which dominate: 100 MiB at B1 = B2 = 8192,
        L = 64 with RG, CG = 32, 16)."""
        return H.dot_apply_pair_workspace(B1, B2, self.dim, L, self.device if device is None else device)

    def apply_pair_raw(self, x, y, g, f, scale_g, scale_f, ws=None, out_x=None, out_y=None):
        """one nsvd_dot_apply_pair call at every dim and kind: every x_i . y_j formed and mapped once for both products
        (the two-call route stays reachable as MatrixFreeKernelOperator.apply_pair_raw(op, ...))"""
        return H.dot_apply_pair(x, y, g, f, self.kind, self.gamma, self.coef0, self._slot, scale_g, scale_f, ws=ws,
                                out_x=out_x, out_y=out_y)


def _gaussian_kernel_constants(sigma: float, ell: float):
    a, b = 1.0 / (4.0 * sigma * sigma), 1.0 / (2.0 * ell * ell)
    c = math.sqrt(a * a + 2.0 * a * b)
    return a, b, c, a + b + c


def _mode_indices(dim: int, n: int) -> np.ndarray:
    """the first n multi-indices (n, dim) by total degree, lexicographic within a degree"""
    def compositions(k, d):
        if d == 1:
            yield (k,)
            return
        for j in range(k, -1, -1):
            for rest in compositions(k - j, d - 1):
                yield (j,) + rest

    idx, deg = [], 0
    while len(idx) < n:
        for comp in compositions(deg, dim):
            idx.append(comp)
            if len(idx) == n:
                break
        deg += 1
    return np.asarray(idx, dtype=np.int64).reshape(n, dim)


def gaussian_kernel_modes(sigma: float, ell: float, dim: int, neigs: int):
    """The first `neigs` Mercer modes of k = exp(-|x - y|^2 / (2 ell^2)) under N(0, sigma^2 I_dim): eigenvalues
    (descending, float64) and their multi-indices (neigs, dim). Per dimension lambda_k = sqrt(2a / A) (b / A)^k with
    a = 1 / (4 sigma^2), b = 1 / (2 ell^2), c = sqrt(a^2 + 2ab), A = a + b + c; a mode's eigenvalue is the product over
    dimensions, so modes come by total degree n (eigenvalue lambda_0^dim (b / A)^n), lexicographic within a degree."""
    a, b, c, A = _gaussian_kernel_constants(sigma, ell)
    lam0, ratio = math.sqrt(2.0 * a / A), b / A
    idx = _mode_indices(dim, neigs)
    vals = np.array([np.prod([lam0 * ratio ** int(k) for k in row]) for row in idx], dtype=np.float64)
    return vals, idx


def gaussian_kernel_eigvals(sigma: float, ell: float, dim: int, neigs: int) -> np.ndarray:
    return gaussian_kernel_modes(sigma, ell, dim, neigs)[0]


def gaussian_kernel_eigenfunctions(x: torch.Tensor, sigma: float, ell: float, neigs: int) -> torch.Tensor:
    """The (unnormalised) eigenfunctions of the same modes at x (n, dim), in float64 on x's device:
    prod_d exp(-(c - a) x_d^2) H_k(sqrt(2c) x_d) with the physicists' Hermite polynomials. (n, neigs)."""
    a, b, c, A = _gaussian_kernel_constants(sigma, ell)
    x = x.double()
    _, idx = gaussian_kernel_modes(sigma, ell, x.shape[1], neigs)
    kmax = int(idx.max())
    z = math.sqrt(2.0 * c) * x
    herm = [torch.ones_like(z), 2.0 * z]
    for k in range(1, kmax):
        herm.append(2.0 * z * herm[k] - 2.0 * k * herm[k - 1])
    env = torch.exp(-(c - a) * (x * x).sum(dim=1))
    cols = []
    for row in idx:
        v = env.clone()
        for d, k in enumerate(row):
            v = v * herm[int(k)][:, d]
        cols.append(v)
    return torch.stack(cols, dim=1)


def gaussian_cross_modes(sigma_x: float, sigma_y: float, ell: float, dim: int, n: int):
    """The first `n` singular values (descending, float64) of k = exp(-|x - y|^2 / (2 ell^2)) as an operator from
    L2(N(0, sigma_y^2 I_dim)) to L2(N(0, sigma_x^2 I_dim)), (Kg)(x) = E_y[k(x, y) g(y)], and their multi-indices
    (n, dim). Per dimension s_k = s_0 rho^k with a = 1 / (4 sigma_x^2) + 1 / (2 ell^2),
    b = 1 / (4 sigma_y^2) + 1 / (2 ell^2), c = 1 / (2 ell^2), t = c / sqrt(a b), r = sqrt(1 - t^2), rho = t / (1 + r),
    s_0 = (2 pi sigma_x^2)^(-1/4) (2 pi sigma_y^2)^(-1/4) (a b)^(-1/4) sqrt(pi / (1 + r)) (Mehler's formula after
    rescaling both sides); a mode's value is the product over dimensions, ordered as gaussian_kernel_modes orders them.
    With sigma_x == sigma_y these are gaussian_kernel_eigvals."""
    c = 1.0 / (2.0 * ell * ell)
    a, b = 1.0 / (4.0 * sigma_x * sigma_x) + c, 1.0 / (4.0 * sigma_y * sigma_y) + c
    t = c / math.sqrt(a * b)
    r = math.sqrt(1.0 - t * t)
    rho = t / (1.0 + r)
    s0 = ((2.0 * math.pi * sigma_x * sigma_x) ** -0.25 * (2.0 * math.pi * sigma_y * sigma_y) ** -0.25 *
          (a * b) ** -0.25 * math.sqrt(math.pi / (1.0 + r)))
    idx = _mode_indices(dim, n)
    vals = np.array([np.prod([s0 * rho ** int(k) for k in row]) for row in idx], dtype=np.float64)
    return vals, idx


def gaussian_cross_singular_values(sigma_x: float, sigma_y: float, ell: float, dim: int, n: int) -> np.ndarray:
    return gaussian_cross_modes(sigma_x, sigma_y, ell, dim, n)[0]


def _multi_indices_up_to(dim: int, degree: int) -> np.ndarray:
    """every multi-index of `dim` entries with |alpha| <= degree, by total degree"""
    n = math.comb(dim + degree, degree)
    return _mode_indices(dim, n)


def polynomial_cross_singular_values(sigma_x: float, sigma_y: float, gamma: float, coef0: float, degree: int, dim: int,
                                     n: int) -> np.ndarray:
    """The first `n` singular values (descending, float64; zeros beyond the rank) of k = (gamma x.y + coef0)^degree as
    an operator from L2(N(0, sigma_y^2 I_dim)) to L2(N(0, sigma_x^2 I_dim)), (Kg)(x) = E_y[k(x, y) g(y)]. The kernel
    has finite rank: k = sum over |alpha| <= degree of w_alpha x^alpha y^alpha with
    w_alpha = C(degree, |alpha|) coef0^(degree - |alpha|) gamma^|alpha| |alpha|! / alpha! (binomial, then multinomial
    theorem), so K = Phi_x diag(w) Phi_y^* on the monomials. With the moment matrices
    M_x[alpha, beta] = E[x^(alpha + beta)] = prod_d E[x_d^(alpha_d + beta_d)] (E[t^a] = sigma^a (a - 1)!! for even a, 0
    for odd a) and M_y likewise, M = R^T R, the non-zero singular values of K are those of R_x diag(w) R_y^T.
    Exact up to float64 rounding; numpy only."""
    degree, dim, n = int(degree), int(dim), int(n)
    if degree < 1 or dim < 1 or n < 1:
        raise ValueError("polynomial_cross_singular_values: degree, dim and n must be positive")
    if not (sigma_x > 0 and sigma_y > 0):
        raise ValueError("polynomial_cross_singular_values: sigma_x and sigma_y must be positive")
    idx = _multi_indices_up_to(dim, degree)
    tot = idx.sum(axis=1)
    w = np.array([math.comb(degree, int(t)) * float(coef0) ** (degree - int(t)) * float(gamma) ** int(t) *
                  math.factorial(int(t)) / np.prod([math.factorial(int(a)) for a in row])
                  for row, t in zip(idx, tot)], dtype=np.float64)

    def moment(sigma, a):  # E[t^a], t ~ N(0, sigma^2)
        if a % 2:
            return 0.0
        return float(sigma) ** a * float(np.prod(np.arange(a - 1, 0, -2, dtype=np.float64)))

    def root(sigma):
        """R with M = R^T R, from the eigendecomposition (M is PSD and badly scaled: eigh keeps its small modes)"""
        m1 = np.array([moment(sigma, a) for a in range(2 * degree + 1)], dtype=np.float64)
        s = idx[:, None, :] + idx[None, :, :]
        M = np.prod(m1[s], axis=2)
        # scale to a unit diagonal first: the monomials' norms span sigma^(2 degree) (2 degree - 1)!!
        d = np.sqrt(np.diag(M))
        lam, V = np.linalg.eigh(M / d[:, None] / d[None, :])
        return (np.sqrt(np.clip(lam, 0.0, None))[:, None] * V.T) * d[None, :]
    A = root(sigma_x) @ (w[:, None] * root(sigma_y).T)
    sv = np.linalg.svd(A, compute_uv=False)
    out = np.zeros(n, dtype=np.float64)
    m = min(n, len(sv))
    out[:m] = sv[:m]
    # values that are rounding noise of a rank-deficient product (coef0 = 0 drops every |alpha| < degree) are zeros
    out[out < 64 * np.finfo(np.float64).eps * max(out[0], np.finfo(np.float64).tiny)] = 0.0
    return out


@torch.no_grad()
def kernel_singular_values(op: MatrixFreeKernelOperator, fn_f, fn_g, x_eval: torch.Tensor, y_eval: torch.Tensor,
                           chunk: int = 4096):
    """Singular-value quotients of the column pairs of F = fn_f(x_eval) (nx, L) and G = fn_g(y_eval) (ny, L) under the
    operator's kernel and the EMPIRICAL measures of the two samples: cross = F^T (K G) / nx with
    K G = (1 / ny) k(x_eval, y_eval) G from op.apply_raw, `chunk` rows of x_eval at a time, cov_f = F^T F / nx,
    cov_g = G^T G / ny; products and sums in float64 (nsvd_spectrum_accumulate_f64, used as kernel_spectrum uses it).
    Returns dict(svals = diag(cross) / sqrt(diag(cov_f) diag(cov_g)), norms_f, norms_g, cross, cov_f, cov_g) as float64
    numpy arrays. L <= 64."""
    if not x_eval.is_cuda or not y_eval.is_cuda:
        raise H.NsvdError("kernel_singular_values: x_eval and y_eval must live on the GPU (no CPU path)")
    x_eval, y_eval = x_eval.float().contiguous(), y_eval.float().contiguous()
    nx, ny, dev = x_eval.shape[0], y_eval.shape[0], x_eval.device
    F = torch.cat([fn_f(x_eval[i:i + chunk]).float() for i in range(0, nx, chunk)]).contiguous()
    G = torch.cat([fn_g(y_eval[i:i + chunk]).float() for i in range(0, ny, chunk)]).contiguous()
    L = F.shape[1]
    if G.shape[1] != L:
        raise H.NsvdError("kernel_singular_values: fn_f and fn_g must return the same number of columns")
    cov_f = torch.zeros((L, L), dtype=torch.float64, device=dev)
    cross, cov_g, unused = torch.zeros_like(cov_f), torch.zeros_like(cov_f), torch.zeros_like(cov_f)
    # (the constant coordinate column and lim = 1/2: kernel_spectrum's note on the accumulation kernel's weight)
    ones = torch.ones((min(chunk, max(nx, ny)), 1), dtype=torch.float32, device=dev)
    ws = None
    for i in range(0, nx, chunk):
        xc, fc = x_eval[i:i + chunk], F[i:i + chunk]
        if ws is None or len(xc) != min(chunk, nx):
            ws = op.workspace(len(xc), ny, L, dev)
        KG = op.apply(xc, y_eval, G, ws=ws)
        H.spectrum_accumulate(fc, KG, ones[:len(xc)], 1.0, False, 0.5, cov_f, cross)
    for i in range(0, ny, chunk):
        gc = G[i:i + chunk]
        H.spectrum_accumulate(gc, gc, ones[:len(gc)], 1.0, False, 0.5, cov_g, unused)
    cf, cg, cr = (cov_f / nx).cpu().numpy(), (cov_g / ny).cpu().numpy(), (cross / nx).cpu().numpy()
    nf, ng = np.diag(cf).copy(), np.diag(cg).copy()
    return dict(svals=np.diag(cr) / np.sqrt(nf * ng), norms_f=nf, norms_g=ng, cross=cr, cov_f=cf, cov_g=cg)


@torch.no_grad()
def kernel_spectrum(op: MatrixFreeKernelOperator, fn, x_eval: torch.Tensor, chunk: int = 4096):
    """Rayleigh quotients of the columns of Phi = fn(x_eval) under the operator's kernel and the EMPIRICAL measure of
    x_eval (n, dim): cov = Phi^T Phi / n, quad = Phi^T (K Phi) / n with K Phi = (1 / n) k(x_eval, x_eval) Phi from
    op.apply_raw (nsvd_rbf_apply / nsvd_dot_apply) against the whole evaluation set, `chunk` rows at a time; products and sums in float64
    (nsvd_spectrum_accumulate_f64, unweighted). Returns dict(eigvals = diag(quad) / diag(cov), norms = diag(cov), cov,
    quad) as float64 numpy arrays. fn maps (m, dim) float32 GPU coordinates to (m, L) values, L <= 64."""
    if not x_eval.is_cuda:
        raise H.NsvdError("kernel_spectrum: x_eval must live on the GPU (no CPU path)")
    x_eval = x_eval.float().contiguous()
    n = x_eval.shape[0]
    phi = torch.cat([fn(x_eval[i:i + chunk]).float() for i in range(0, n, chunk)]).contiguous()
    L = phi.shape[1]
    cov = torch.zeros((L, L), dtype=torch.float64, device=x_eval.device)
    quad = torch.zeros_like(cov)
    # the accumulation kernel's weight is 1 / sqrt(p_val) of the uniform box [-lim, lim]^D: lim = 1/2 makes it 1; it
    # also drops the operator rows of samples AT the origin (a rule of the PDE problems): it is given a constant
    # coordinate column instead of x_eval
    ones = torch.ones((min(chunk, n), 1), dtype=torch.float32, device=x_eval.device)
    ws = None
    for i in range(0, n, chunk):
        xc, pc = x_eval[i:i + chunk], phi[i:i + chunk]
        if ws is None or len(xc) != min(chunk, n):
            ws = op.workspace(len(xc), n, L, x_eval.device)
        Kphi = op.apply(xc, x_eval, phi, ws=ws)
        H.spectrum_accumulate(pc, Kphi, ones[:len(xc)], 1.0, False, 0.5, cov, quad)
    cov64, quad64 = (cov / n).cpu().numpy(), (quad / n).cpu().numpy()
    return dict(eigvals=np.diag(quad64) / np.diag(cov64), norms=np.diag(cov64).copy(), cov=cov64, quad=quad64)


class FusedKernelTrainer:
    """The kernel-operator training step (NestedLoRA.compute_loss_kernel with split_batch = False on a
    DenseKernelOperator, then loss.backward(); RMSprop (+ cosine schedule); EMA - reference methods/nestedlora.py:230-252
    with the optimiser of examples/utils.py:50-57) as a fixed sequence of C-ABI calls on flat parameter buffers: index
    batch -> gather of the coordinates -> model evaluation (nsvd_model_forward) -> Kf = K[x][:, x] f / B
    (nsvd_kernel_apply) -> moments (nsvd_evd_moments) -> d loss / d f, backward and the optimiser step inside
    the backward kernels (nsvd_model_backward_evd_step). No torch autograd, no torch.optim; what torch still does is
    draw the indices and gather the coordinates. The counterpart of trainer.FusedTrainer for BASELINE configs[3].

    Multi-GPU (comm: parallel.Communicator with world > 1): HEADS sharded, as trainer.FusedTrainer's "hp". Rank r owns
    the heads [r L / W, (r + 1) L / W) - weights, gradients, optimiser state: nothing replicated, no gradient traffic.
    Every rank draws the same index batch (equal generator seeds), evaluates its heads on it, and applies K to ITS
    columns of f only (Kf[:, l] = K[x][:, x] f[:, l] / B needs no other head): the MFMA work of the step is split W
    ways. One all-gather of the packed (2, B, L / W) block [f | Kf] per step (any L >= W: the first L % W ranks own one head more) (2 B L floats in total: 4 MB at cfg4) is
    the only exchange; moments, loss gradient and backward of the local heads are then local.

    With a RadialKernelOperator or a DotKernelOperator the batch is a COORDINATE batch (drawn as sigma * randn, or given):
    the model is evaluated on it directly and Kf = k(x, x) f / B comes from the operator's apply_raw (nsvd_rbf_apply /
    nsvd_dot_apply) in place of nsvd_kernel_apply; everything
    after Kf is the same sequence. Single GPU only (comm raises NotImplementedError)."""

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192,
                 sequential: bool = False, step: int = 1, lr: float = 1e-4, rmsprop_decay: float = 0.99,
                 rmsprop_eps: float = 1e-8, ema_decay: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05,
                 hard_mul_const: float = 1.0, seed: int = 0, index_seed: int = 1, comm=None):
        from .nested_lowrank import nesting_masks
        from .trainer import FlatParams, reference_init
        self.op = op
        self.coords = isinstance(op, MatrixFreeKernelOperator)  # coordinate batches (radial or dot-product kernel)
        if self.coords and comm is not None:
            raise NotImplementedError("FusedKernelTrainer: sharded runs (comm) are not built for "
                                      + type(op).__name__)
        dev = op.device if self.coords else op.K.device
        self.device = dev
        D = op.dim if self.coords else op.points.shape[1]
        self.comm = comm if comm is not None and comm.multi else None
        world = self.comm.world if self.comm is not None else 1
        rank = self.comm.rank if self.comm is not None else 0
        # any L >= world: L // world heads each, the first L % world ranks one more (parallel.head_range)
        from .parallel import head_block, head_range
        self.world, self.Lg = world, L
        self.l_off, Ll = head_range(L, rank, world)
        Lb = head_block(L, world)
        self.full_shape = H.ModelShape(L=L, D=D, m=m, hidden=tuple(hidden), has_exp_mask=False)
        self.shape = H.ModelShape(L=Ll, D=D, m=m, hidden=tuple(hidden), has_exp_mask=False)
        self.B = int(batch_size)
        if any(h != 128 for h in hidden) or self.B % 32 != 0 or not 1 <= D <= 64 or (2 * m) % 128 != 0:
            raise H.NsvdError("FusedKernelTrainer needs the MFMA model kernels: 128-wide hidden layers, batch % 32 == 0, "
                              "2 m % 128 == 0, input dimension <= 64 (nsvd_model_backward_evd_step)")
        self.P = FlatParams(self.shape, dev)
        fB0, ws0, bs0, _ = reference_init(self.full_shape, fourier_scale, None, seed)
        sl = slice(self.l_off, self.l_off + Ll)  # this rank's heads of the (identically seeded) full model
        self.P.load(fB0, [w[sl] for w in ws0], [b[sl] for b in bs0], None)
        if self.comm is not None:
            self.comm.broadcast(self.P.fourier_B, 0)  # the frozen Fourier matrix is shared whatever the ranks drew
        self._params = self.P.pack(self.P.flat, True)
        self._sq = self.P.pack(self.P.sq, False)
        self._ema = self.P.pack(self.P.ema, True) if ema_decay > 0 else None
        self.vector_mask, self.matrix_mask, self.mask_kind = nesting_masks(L, sequential, step)
        cust = self.mask_kind == H.MASK_CUSTOM
        self.v = self.vector_mask.to(dev) if cust else None
        self.M = self.matrix_mask.to(dev).contiguous() if cust else None
        self.lr, self.alpha, self.eps, self.ema_decay, self.num_iters = lr, rmsprop_decay, rmsprop_eps, ema_decay, num_iters
        self.c = float(hard_mul_const)
        self.ws = H.model_workspace(self.shape, self.B, dev)
        if self.coords:
            self.ka_ws = op.workspace(self.B, self.B, Ll, dev)
        else:
            self.ka_ws = torch.empty(H._lib.load().nsvd_kernel_apply_workspace_bytes(int(op.N), self.B, Ll),
                                     dtype=torch.uint8, device=dev)
        # this rank's outputs packed [f | Kf] so that one all-gather moves both
        # (the all-gather block, as long as the largest rank's, begins with it: nsvd_evd_gather_head_blocks)
        self._blk = torch.zeros(2 * self.B * Lb, dtype=torch.float32, device=dev)
        self.fKf_loc = self._blk[:2 * self.B * Ll].view(2, self.B, Ll)
        self.f_loc, self.Kf_loc = self.fKf_loc[0], self.fKf_loc[1]
        if self.comm is not None:
            self.gath = torch.empty((world, 2 * self.B * Lb), dtype=torch.float32, device=dev)
            self.fKf = torch.empty((2, self.B, L), dtype=torch.float32, device=dev)
            self.f, self.Kf = self.fKf[0], self.fKf[1]
        else:
            self.f, self.Kf = self.f_loc, self.Kf_loc
        self.moments = torch.empty(2 * L * L + 1, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(3, dtype=torch.float32, device=dev)
        self.scratch = H.evd_scratch(self.B, L, dev)
        self.gen = torch.Generator(device=dev).manual_seed(index_seed)  # the same stream on every rank
        self.probe = None  # parallel.CommProbe while bench.py measures the exposed wait of the all-gather
        self.t = 0

    def step(self, idx: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the index batch idx (or a fresh draw; sharded runs: the SAME batch on every rank) -
        with a RadialKernelOperator: on the (B, D) coordinate batch given in its place, or a fresh draw;
        returns the device loss triple (no sync)"""
        from .trainer import coordinate_batch, cosine_lr
        if self.coords:
            x = self.op.sample(self.B, self.gen) if idx is None else idx
            x = coordinate_batch(x, self.B, self.op.dim, "FusedKernelTrainer.step: the batch")
            H.model_forward(self.shape, self._params, x, self.c, self.ws, save_for_backward=True, out=self.f_loc)
            self.op.apply_raw(x, x, self.f_loc, 1.0 / self.B, ws=self.ka_ws, out=self.Kf_loc)
        else:
            if idx is None:
                idx = self.op.sample_indices(self.B, self.gen)
            idx = idx.to(torch.int64).contiguous()
            x = self.op.points.index_select(0, idx)
            H.model_forward(self.shape, self._params, x, self.c, self.ws, save_for_backward=True, out=self.f_loc)
            H.kernel_apply(self.op.K, self.op.N, idx, idx, self.f_loc, 1.0 / self.B, ws=self.ka_ws, out=self.Kf_loc)
        if self.comm is not None:
            if self.probe is not None:
                with self.probe.span("f_Kf_all_gather_wait"):
                    self.comm.all_gather(self.gath, self._blk)  # blocking: on the compute stream (parallel.dp_step)
            else:
                self.comm.all_gather(self.gath, self._blk)
            H.evd_gather_head_blocks(self.gath, self.Lg, self.f, self.Kf, self.mask_kind, self.v)
        # the reduced moment vector (partials + one reduction launch): at B = 8192 every workgroup of the backward
        # summing the 128 per-chunk partials of its 2 L moments itself would cost 3 x the reduction
        H.evd_moments(self.f, self.Kf, self.mask_kind, self.v, self.moments, self.scratch)
        lr = cosine_lr(self.lr, self.t, self.num_iters) if self.num_iters > 0 else self.lr
        decay = min(self.ema_decay, (2 + self.t) / (11 + self.t)) if self._ema is not None else 0.0
        opt = H.rmsprop_state(self._sq, self._ema, lr, self.alpha, self.eps, decay)
        H.model_backward_evd_step(self.shape, self._params, x, self.f, self.Kf, self.mask_kind, self.v, self.M,
                                  self.moments, True, None, self.loss, None, opt, self.ws, l_offset=self.l_off)
        if self.probe is not None:
            self.probe.step_done()
        self.t += 1
        return self.loss
