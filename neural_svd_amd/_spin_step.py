"""What SpIN (spin.py) and SpINx (spinx.py) share on the matrix-free kernel operators: the per-shape device buffers
of a step, its two ends (model forward + Kphi; the swapped-argument product + model backward), the refusals of the
two class paths with their common nn.Module base, and the base of the two trainers on flat buffers - whose
method-independent part, KernelTrainer, is also the base of NeuralEF's trainer (neuralef.py). Each method keeps its own
moments, solve and cotangents."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import hip_ops as H
from ._lib import NsvdError
from .kernel_ops import MatrixFreeKernelOperator
from .trainer import FlatModel, coordinate_batch


def chunk_rows(B: int, split_batch: bool):
    """(B1, B2): rows that carry Kphi / reference rows, as torch.chunk(x, 2) splits them"""
    if not split_batch:
        return B, B
    B1 = (B + 1) // 2
    if B - B1 < 1:
        raise NsvdError("SpIN: split_batch needs at least 2 rows")
    return B1, B - B1


class StepBuffers:
    """the device buffers of one step shape (B rows, split or not) that both methods use; _SpinWork and _SpinxWork
    add their own. A trainer builds one for good, a class path one per call."""

    def __init__(self, op, shape, B: int, split: bool, dev):
        self.op, self.L, self.B, self.split = op, shape.L, B, split
        self.B1, self.B2 = B1, B2 = chunk_rows(B, split)
        L = shape.L
        self.model_ws = H.model_workspace(shape, B, dev)
        self.ka_ws = op.workspace(B1, B2, L, dev)
        self.phi_all = torch.empty((B, L), dtype=torch.float32, device=dev)
        self.Kphi = torch.empty((B1, L), dtype=torch.float32, device=dev)
        self.dK = torch.empty((B1, L), dtype=torch.float32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ka_ws_back = self.dout = None

    def with_backward(self):
        """adds what only the backward half touches (a class path: not before its backward runs)"""
        if self.dout is None:
            self.ka_ws_back = self.op.workspace(self.B2, self.B1, self.L, self.dK.device)
            self.dout = torch.empty_like(self.phi_all)
        return self


def forward_product(model, x, w: StepBuffers) -> None:
    """model(x) on all B rows into w.phi_all (saved for the backward) and Kphi = k(x[:B1], x_ref) phi(x_ref) / B2 into
    w.Kphi; model: a trainer.PackedModel"""
    B1 = w.B1
    model.forward(x, w.model_ws, out=w.phi_all)
    if w.split:
        w.op.apply_raw(x[:B1], x[B1:], w.phi_all[B1:], 1.0 / w.B2, ws=w.ka_ws, out=w.Kphi)
    else:
        w.op.apply_raw(x, x, w.phi_all, 1.0 / w.B2, ws=w.ka_ws, out=w.Kphi)


def swapped_product_backward(model, x, w: StepBuffers, ref_rows_filled: bool) -> None:
    """w.dK reaches model(x_ref) through the product with the arguments swapped, then ONE model backward (model.grads
    OVERWRITTEN). w.dout[:B1] holds the cotangent of phi. ref_rows_filled: with split_batch the rows [B1:] already
    hold a cotangent as well (SpINx: Phi T_s) and the product is added to it; otherwise it is written straight there."""
    B1 = w.B1
    x_ref, x_k = (x[B1:], x[:B1]) if w.split else (x, x)
    rows = w.dout[B1:] if w.split else w.dout
    if w.split and not ref_rows_filled:
        w.op.apply_raw(x_ref, x_k, w.dK, 1.0 / w.B2, ws=w.ka_ws_back, out=rows)
    else:
        rows.add_(w.op.apply_raw(x_ref, x_k, w.dK, 1.0 / w.B2, ws=w.ka_ws_back))
    model.backward(x, w.dout, w.model_ws)


# ---- the class paths ------------------------------------------------------------------------------------------------
def check_op(who: str, get_approx_kernel_op, importance):
    op = getattr(get_approx_kernel_op, "__self__", None)
    if not isinstance(op, MatrixFreeKernelOperator) or \
            getattr(get_approx_kernel_op, "__func__", None) is not MatrixFreeKernelOperator.get_approx_kernel_op:
        raise NotImplementedError(f"{who} (HIP): get_approx_kernel_op must be the bound method of a "
                                  "MatrixFreeKernelOperator (the gradient into Kphi is taken through the operator's "
                                  "own matrix-free product); foreign callables are not built")
    if importance is not None:
        raise NotImplementedError(f"{who} (HIP): importance-weighted kernel operators are not built")
    return op


def check_x(who: str, x, op):
    if not x.is_cuda:
        raise NsvdError(f"{who}: x must live on the GPU (no CPU path)")
    x = x.detach().reshape(x.shape[0], -1).float().contiguous()
    if x.shape[1] != op.dim:
        raise NsvdError(f"{who}: x must be (B, {op.dim}) for this operator")
    return x


def check_model(who: str, model, neigs, decay) -> None:
    from .models import WaveFunctions
    if not isinstance(model, WaveFunctions):
        raise NotImplementedError(f"{who} (HIP): model must be this package's WaveFunctions(ParallelMLP)")
    if model.has_exp_mask or model.box is not None:
        raise NotImplementedError(f"{who} (HIP): models with an exponential or box mask are not built (the "
                                  "kernel-operator models have none)")
    if int(neigs) != model.base.num_copies:
        raise ValueError(f"{who}: neigs = {neigs} but the model has {model.base.num_copies} heads")
    if not 2 <= int(neigs) <= H.SPIN_MAX_L:
        # (the reference's own SpIN fails at neigs = 1: spin_step receives a 0-D pi)
        raise ValueError(f"{who}: neigs must be in 2..{H.SPIN_MAX_L}")
    if not 0.0 <= float(decay) <= 1.0:
        raise ValueError(f"{who}: decay must be in [0, 1]")


class WhitenedMethod(nn.Module):
    """what the modules SpIN and SpINx share: the model, the moving average of sigma and its Cholesky factor (in this
    order: the reference's state-dict keys and named_parameters order), and the orthonormalised forward"""

    def __init__(self, name: str, who: str, model, neigs, decay):
        """
        :param decay:
            0.0 = the moving average is constant (less update)
            1.0 = the moving average has no memory (more update)
        """
        self.name = name
        super().__init__()
        check_model(who, model, neigs, decay)
        self.model = model
        self.neigs = int(neigs)
        self.decay = decay
        self.sigma_avg = nn.Parameter(torch.zeros(neigs, neigs), requires_grad=False)
        self.chol = nn.Parameter(torch.zeros(neigs, neigs), requires_grad=False)

    def forward(self, x):
        # a wrapper to output orthonormalized eigenfunction (methods/spin.py:209-215, methods/spinx.py:185-191)
        return torch.linalg.solve_triangular(self.chol, self.model(x).T, upper=False).T


# ---- the trainers on flat buffers -------------------------------------------------------------------------------------
class KernelTrainer:
    """what every method's trainer on a matrix-free kernel operator shares (SpIN, SpINx here, NeuralEF in neuralef.py):
    the refusals, one FlatModel, the batch and the optimiser step; a subclass sets ``loss``, what step() returns.
    dims = (L, m, hidden), L within MIN_L..MAX_L; model_kw: FlatModel's arguments after the device."""
    MIN_L, MAX_L = 1, 64

    def __init__(self, op, dims, batch_size: int, index_seed: int, **model_kw):
        who = type(self).__name__
        L, m, hidden = dims
        if not isinstance(op, MatrixFreeKernelOperator):
            raise NotImplementedError(f"{who}: a MatrixFreeKernelOperator (radial or dot-product kernel)")
        if not self.MIN_L <= int(L) <= self.MAX_L:
            raise ValueError(f"{who}: L must be in {self.MIN_L}..{self.MAX_L}")
        self.op, self.device, self.B = op, op.device, int(batch_size)
        self.shape = H.ModelShape(L=int(L), D=op.dim, m=int(m), hidden=tuple(hidden), has_exp_mask=False)
        self.model = FlatModel(self.shape, self.device, **model_kw)
        self.P, self.c = self.model.P, self.model.c
        self.gen = torch.Generator(device=self.device).manual_seed(index_seed)
        self.t = 0

    def _batch(self, x, what: str):
        x = self.op.sample(self.B, self.gen) if x is None else x
        return coordinate_batch(x, self.B, self.op.dim, f"{type(self).__name__}.{what}: x")

    def _opt_step(self) -> torch.Tensor:
        self.model.opt_step(self.t)
        self.t += 1
        return self.loss


class WhitenedKernelTrainer(KernelTrainer):
    """what SpinKernelTrainer and SpinxKernelTrainer add: sigma_avg / chol, the buffers of the step shape (``Work``, a
    StepBuffers subclass whose ``loss`` is what step() returns), check() and the orthonormalised forward."""
    MIN_L, MAX_L = 2, H.SPIN_MAX_L
    Work = None
    FAILED = ""  # what check() reports

    def __init__(self, op, dims, batch_size: int, decay: float, split_batch: bool, index_seed: int, **model_kw):
        super().__init__(op, dims, batch_size, index_seed, **model_kw)
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"{type(self).__name__}: decay must be in [0, 1]")
        self.decay, dev, L = float(decay), self.device, self.shape.L
        self.work = w = self.Work(op, self.shape, self.B, bool(split_batch), dev)
        self.sigma_avg = torch.zeros((L, L), dtype=torch.float32, device=dev)
        self.chol = torch.zeros((L, L), dtype=torch.float32, device=dev)
        w.with_backward()
        self.B1, self.B2, self.split = w.B1, w.B2, w.split
        self.status, self.loss, self.phi = w.status, w.loss, w.phi_all[:w.B1]

    def check(self) -> None:
        """raise if any step since the last check failed a Cholesky factorisation (one small device read)"""
        bits = int(self.status.item())
        self.status.zero_()
        if bits:
            raise NsvdError(f"{type(self).__name__}: {self.FAILED} in a step since the last check")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """the orthonormalised eigenfunctions (SpIN.forward / SpINx.forward): chol^-1 applied to model(x)"""
        return torch.linalg.solve_triangular(self.chol, self.model.evaluate(x).T, upper=False).T

    __call__ = forward
