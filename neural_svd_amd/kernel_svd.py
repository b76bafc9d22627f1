"""Kernel SVD: the singular functions of a cross-domain kernel k(x, y), x ~ p_x, y ~ p_y, learned with two models.

The SVD form of the nested low-rank loss (``NestedLoRALossFunctionSVD(f, Tg, g, Tadjf)``, reference
methods/nestedlora.py:114-164, which has no caller there) needs ``Tg = K g`` together with ``Tadjf = K^T f``; a
``MatrixFreeKernelOperator`` produces the two with ``apply_pair_raw`` (``RadialKernelOperator``: one
``nsvd_rbf_apply_pair`` call, ``DotKernelOperator``: one ``nsvd_dot_apply_pair`` call, every kernel value evaluated
once; the base class: two ``apply_raw`` calls).

- ``PairedFunctions(f_model, g_model)``: the model of a NestedLoRA method that learns a pair;
- ``NestedLoRA.compute_loss_kernel_svd(svd_op, x, y)`` (defined here, bound in nested_lowrank.py): the class path,
  differentiable through both models;
- ``KernelSvdTrainer``: the same step as a fixed sequence of C-ABI calls on two flat parameter buffers.

For the Gaussian kernel between two Gaussian measures the singular values are known in closed form
(``kernel_ops.gaussian_cross_singular_values``), and so are those of the polynomial kernel
(``kernel_ops.polynomial_cross_singular_values``); ``kernel_ops.kernel_singular_values`` evaluates the quotients of any
pair of function families on samples."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import hip_ops as H
from ._lib import NsvdError
from .kernel_ops import DenseCrossOperator, MatrixFreeKernelOperator


class PairedFunctions(nn.Module):
    """The two function families of a kernel SVD: ``.f`` takes x (the left singular functions), ``.g`` takes y."""

    def __init__(self, f_model: nn.Module, g_model: nn.Module):
        super().__init__()
        self.f, self.g = f_model, g_model

    def forward(self, x, y):
        return self.f(x), self.g(y)


def compute_loss_kernel_svd(method, svd_op, x, y, importance=None):
    """NestedLoRA.compute_loss_kernel_svd: ``svd_op(model_f, model_g, x, y, importance) -> (Tg, f, Tadjf, g)``
    (``op.get_approx_kernel_svd_op()``) on the method's PairedFunctions, then the SVD loss on the HIP kernels.
    Returns (loss, dict(f, g, Tg, Tadjf, eigvals=None)); loss.backward() reaches both models."""
    if not isinstance(method.model, PairedFunctions):
        raise NsvdError("compute_loss_kernel_svd: the method's model must be a PairedFunctions(f_model, g_model)")
    if method.sort_indices is not None:
        raise NsvdError("compute_loss_kernel_svd: register_eigvals (sorted heads) is not built for a pair of models")
    if not callable(svd_op):
        raise NsvdError("compute_loss_kernel_svd: svd_op must be callable as svd_op(model_f, model_g, x, y, importance)")
    if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0]:
        raise NsvdError(f"compute_loss_kernel_svd: x {tuple(x.shape)} and y {tuple(y.shape)} must be two 2-D batches of "
                        "the same number of rows (NestedLoRALossFunctionSVD on the HIP kernels takes B1 == B2)")
    Tg, f, Tadjf, g = svd_op(method.model.f, method.model.g, x, y, importance=importance)
    L = method.neigs
    for t, n in ((f, "f"), (g, "g"), (Tg, "Tg"), (Tadjf, "Tadjf")):
        if t.dim() != 2 or tuple(t.shape) != (x.shape[0], L):
            raise NsvdError(f"compute_loss_kernel_svd: svd_op returned {n} {tuple(t.shape)}: expected "
                            f"({x.shape[0]}, {L})")
    f, g = f.float().contiguous(), g.float().contiguous()
    loss = method._compute_loss(f, Tg.detach().float().contiguous(), g, Tadjf.detach().float().contiguous(), evd=False)
    return loss, dict(f=f, g=g, Tg=Tg, Tadjf=Tadjf, eigvals=None)


class _SvdStep:
    """What the two SVD trainers share: the constraints of the MFMA model kernels, two FlatModels (f on the x side, g on
    the y side, seeded ``seed`` and ``seed + 1``, one optimiser rule), the nesting masks, the buffers of a step and the
    step's tail on (X, TX)."""

    def _check_model_kernels(self, hidden, m):
        if any(h != 128 for h in hidden) or self.B % 32 != 0 or (2 * int(m)) % 128 != 0:
            raise NsvdError(f"{type(self).__name__} needs the MFMA model kernels: 128-wide hidden layers, "
                            "batch % 32 == 0, 2 m % 128 == 0 (nsvd_model_backward)")

    def _build(self, shapes, sequential, step, lr, optimizer, rmsprop_decay, rmsprop_eps, momentum, num_iters,
               fourier_scale, hard_mul_const, seed, index_seed):
        """shapes: the ModelShapes of the f and the g model (the same L)"""
        from .nested_lowrank import nesting_masks
        from .trainer import FlatModel
        dev, B, L = self.device, self.B, shapes[0].L
        self.c = float(hard_mul_const)
        self.models = tuple(FlatModel(sh, dev, s, fourier_scale, hard_mul_const, optimizer, lr, rmsprop_decay,
                                      rmsprop_eps, momentum, num_iters) for sh, s in zip(shapes, (seed, seed + 1)))
        self.Pf, self.Pg = self.models[0].P, self.models[1].P
        self.vector_mask, self.matrix_mask, self.mask_kind = nesting_masks(int(L), bool(sequential), step)
        cust = self.mask_kind == H.MASK_CUSTOM
        self.v = self.vector_mask.to(dev).float().contiguous() if cust else None
        self.M = self.matrix_mask.to(dev).float().contiguous() if cust else None
        self.model_ws = (H.model_workspace(shapes[0], B, dev), H.model_workspace(shapes[1], B, dev))
        self.pair_ws = self.op.workspace_pair(B, B, int(L), dev)
        self.X = torch.empty((2 * B, L), dtype=torch.float32, device=dev)
        self.TX = torch.empty_like(self.X)
        self.dX = torch.empty_like(self.X)
        self.moments = torch.empty(2 * L * L + 1, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(3, dtype=torch.float32, device=dev)
        self.scratch = H.evd_scratch(2 * B, int(L), dev)
        self.gen = torch.Generator(device=dev).manual_seed(index_seed)
        self.t = 0

    def _finish(self, x, y) -> torch.Tensor:
        """the step behind the two-sided product: X = [f; g] and TX = [Tg; Tadjf] are written, x and y are the models'
        inputs of the forward calls"""
        B, (mf, mg) = self.B, self.models
        H.evd_moments(self.X, self.TX, self.mask_kind, self.v, self.moments, self.scratch)
        H.evd_loss_grad(self.X, self.TX, self.mask_kind, self.v, self.M, self.moments, 1.0, True, loss=self.loss,
                        df=self.dX)
        mf.backward(x, self.dX[:B], self.model_ws[0])
        mg.backward(y, self.dX[B:], self.model_ws[1])
        mf.opt_step(self.t)
        mg.opt_step(self.t)
        self.t += 1
        return self.loss

    def f(self, x: torch.Tensor) -> torch.Tensor:
        """the left functions at the coordinates x (n, Dx): (n, L)"""
        return self.models[0].evaluate(x)

    def g(self, y: torch.Tensor) -> torch.Tensor:
        """the right functions at the coordinates y (n, Dy): (n, L)"""
        return self.models[1].evaluate(y)


class KernelSvdTrainer(_SvdStep):
    """The kernel SVD training step (NestedLoRA.compute_loss_kernel_svd on a PairedFunctions, loss.backward(), one
    optimiser over both models) as a fixed sequence of C-ABI calls on two flat parameter buffers: two
    nsvd_model_forward (f on x, g on y, written into the halves of X = [f; g]) -> op.apply_pair_raw into the halves of
    TX = [Tg; Tadjf] -> nsvd_evd_moments + nsvd_evd_loss_grad on (X, TX) (the identity in NestedLoRALossFunctionSVD's
    docstring: d loss / d X = [d loss / d f; d loss / d g]) -> two nsvd_model_backward -> two nsvd_opt_step. No torch
    autograd, no torch.optim; torch draws the two batches. The SpinKernelTrainer pattern and its constraints: 128-wide
    hidden layers, 2 m % 128 == 0, batch % 32 == 0; single GPU.

    x ~ N(0, sigma_x^2 I), y ~ N(0, sigma_y^2 I) (defaults: the operator's sigma for both). The g model is seeded with
    seed + 1. ``loss`` = nsvd_evd_loss_grad's triple on (X, TX) after a step: loss[0] is the SVD loss - its operator
    term -2 mean over the 2 B rows of sum_l v_l X TX is -2 mean_b sum_l v_l f Tg because
    sum_b f_b . Tg_b = f^T K g / B = sum_b g_b . Tadjf_b."""

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192, sigma_x: float = None,
                 sigma_y: float = None, sequential: bool = False, step: int = 1, lr: float = 1e-4,
                 optimizer: str = "rmsprop", rmsprop_decay: float = 0.99, rmsprop_eps: float = 1e-8,
                 momentum: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05, hard_mul_const: float = 1.0,
                 seed: int = 0, index_seed: int = 1):
        if not isinstance(op, MatrixFreeKernelOperator):
            raise NotImplementedError("KernelSvdTrainer: a MatrixFreeKernelOperator (radial or dot-product kernel)")
        self.op, self.device = op, op.device
        self.B = int(batch_size)
        self._check_model_kernels(hidden, m)
        self.shape = H.ModelShape(L=int(L), D=op.dim, m=int(m), hidden=tuple(hidden), has_exp_mask=False)
        self.sigma_x = float(op.sigma if sigma_x is None else sigma_x)
        self.sigma_y = float(op.sigma if sigma_y is None else sigma_y)
        if not (self.sigma_x > 0 and self.sigma_y > 0):
            raise ValueError("KernelSvdTrainer: sigma_x and sigma_y must be positive")
        self._build((self.shape, self.shape), sequential, step, lr, optimizer, rmsprop_decay, rmsprop_eps, momentum,
                    num_iters, fourier_scale, hard_mul_const, seed, index_seed)

    def sample(self):
        D = self.op.dim
        x = self.sigma_x * torch.randn(self.B, D, device=self.device, generator=self.gen)
        y = self.sigma_y * torch.randn(self.B, D, device=self.device, generator=self.gen)
        return x, y

    def step(self, x: torch.Tensor = None, y: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the (B, D) coordinate batches x and y (or a fresh draw of both); returns ``loss``
        (no sync)"""
        from .trainer import coordinate_batch
        if (x is None) != (y is None):
            raise NsvdError("KernelSvdTrainer.step: give both x and y, or neither")
        if x is None:
            x, y = self.sample()
        B, (mf, mg) = self.B, self.models
        x = coordinate_batch(x, B, self.op.dim, "KernelSvdTrainer.step: x")
        y = coordinate_batch(y, B, self.op.dim, "KernelSvdTrainer.step: y")
        f, g = self.X[:B], self.X[B:]
        mf.forward(x, self.model_ws[0], out=f)
        mg.forward(y, self.model_ws[1], out=g)
        self.op.apply_pair_raw(x, y, g, f, 1.0 / B, 1.0 / B, ws=self.pair_ws, out_x=self.TX[:B], out_y=self.TX[B:])
        return self._finish(x, y)


class DenseSvdTrainer(_SvdStep):
    """KernelSvdTrainer's step for a stored matrix (``kernel_ops.DenseCrossOperator``): the singular functions of A as
    an operator between the uniform measures on its column and row points. Torch draws the two INDEX batches and gathers
    the coordinates (index_select); two nsvd_model_forward (f on points_x[idx_x], g on points_y[idx_y]) into the halves
    of X = [f; g] -> op.apply_pair_raw on the indices (one nsvd_kernel_apply_pair call, no transposed copy of A) into
    the halves of TX = [Tg; Tadjf] -> nsvd_evd_moments + nsvd_evd_loss_grad on (X, TX) -> two nsvd_model_backward -> two
    nsvd_opt_step. The same options and constraints as KernelSvdTrainer (128-wide hidden layers, 2 m % 128 == 0,
    batch % 32 == 0; single GPU) without the sigmas; the two models have input dimensions Dx and Dy. The g model is
    seeded with seed + 1. ``loss``: as KernelSvdTrainer's."""

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192, sequential: bool = False,
                 step: int = 1, lr: float = 1e-4, optimizer: str = "rmsprop", rmsprop_decay: float = 0.99,
                 rmsprop_eps: float = 1e-8, momentum: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05,
                 hard_mul_const: float = 1.0, seed: int = 0, index_seed: int = 1):
        if not isinstance(op, DenseCrossOperator):
            raise NotImplementedError("DenseSvdTrainer: a DenseCrossOperator (a stored matrix on two point sets)")
        self.op, self.device = op, op.device
        self.B = int(batch_size)
        self._check_model_kernels(hidden, m)
        self.shapes = tuple(H.ModelShape(L=int(L), D=D, m=int(m), hidden=tuple(hidden), has_exp_mask=False)
                            for D in (op.dim_x, op.dim_y))
        self._build(self.shapes, sequential, step, lr, optimizer, rmsprop_decay, rmsprop_eps, momentum, num_iters,
                    fourier_scale, hard_mul_const, seed, index_seed)

    def sample(self):
        return self.op.sample_indices(self.B, self.gen)

    def step(self, idx_x: torch.Tensor = None, idx_y: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the (B,) int64 index batches idx_x (rows of A) and idx_y (columns), or a fresh draw of
        both; returns ``loss`` (no sync)"""
        if (idx_x is None) != (idx_y is None):
            raise NsvdError("DenseSvdTrainer.step: give both idx_x and idx_y, or neither")
        if idx_x is None:
            idx_x, idx_y = self.sample()
        B, (mf, mg) = self.B, self.models
        for t, n in ((idx_x, "idx_x"), (idx_y, "idx_y")):
            if not t.is_cuda or t.dtype != torch.int64 or tuple(t.shape) != (B,):
                raise NsvdError(f"DenseSvdTrainer.step: {n} must be a ({B},) int64 index batch on the GPU")
        idx_x, idx_y = idx_x.contiguous(), idx_y.contiguous()
        x, y = self.op.points_x.index_select(0, idx_x), self.op.points_y.index_select(0, idx_y)
        f, g = self.X[:B], self.X[B:]
        mf.forward(x, self.model_ws[0], out=f)
        mg.forward(y, self.model_ws[1], out=g)
        self.op.apply_pair_raw(idx_x, idx_y, g, f, 1.0 / B, 1.0 / B, ws=self.pair_ws, out_x=self.TX[:B],
                               out_y=self.TX[B:])
        return self._finish(x, y)

    def quotients(self):
        """op.quotients on the two models as they stand"""
        return self.op.quotients(self.f, self.g)
