"""NeuralEF (mu-EigenGame), the paper's comparison baseline, with the reference's names and argument meaning, backed by
the HIP C ABI:

    NeuralEigenfunctions(model, neigs, batchnorm_mode, sort, unbiased, include_diag)   methods/neuralef.py:65-152
    NeuralEigenfunctionsLossFunction.apply(phi, Tphi, phi1, Tphi1, phi2, Tphi2, unbiased, diagonal)  :13-62
    BatchL2NormalizedFunctions(base_model, neigs, momentum, batchnorm_mode)         methods/utils.py:36-86

``compute_loss_operator(operator, x, importance)`` takes the fused HIP path (nsvd_nef_operator_forward / _backward)
when ``operator`` is this package's OperatorWrapper with Gaussian or no importance: one operator forward that stops at
the raw head outputs, the per-stencil-point batch norms and running-norm updates on the device, phi / Tphi with 1 / n_e
folded into the even / odd stencil. Any other density or callable runs the reference's op sequence
through ``BatchL2NormalizedFunctions.forward`` around the HIP model. The loss is the HIP kernel nsvd_nef_loss in
every case. There is no CPU / eager fallback.

    NefKernelTrainer(op, L, m, hidden, batch_size, split_batch, ...)   compute_loss_kernel's step on a matrix-free kernel
                                                                       operator on flat buffers, no torch autograd
                                                                       (nsvd_nef_rows_forward / _backward)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import hip_ops as H
from ._lib import NsvdError
from ._spin_step import KernelTrainer


def _flat(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 2:
        raise NsvdError(f"NeuralEigenfunctionsLossFunction (HIP): {name} must be (B, L) (the (B, L, O) form of the "
                        f"reference is not on this path), got {tuple(t.shape)}")
    return t.detach().float().contiguous()


class NeuralEigenfunctionsLossFunction(torch.autograd.Function):
    """loss = sum(phi variance) + (sum(phi1 align_1) + sum(phi2 align_2)) / 2 on the HIP kernels (nsvd_nef_loss);
    the pseudo-gradient 4 variance to phi, 2 align_h to phi_h, none to the Tphi's, grad_output ignored - all as the
    reference (methods/neuralef.py:37-62). phi1, phi2 = torch.chunk(phi, 2) (what compute_loss_operator passes) is one
    fused kernel pass and one gradient to phi; independent halves of any row counts take the general form."""

    @staticmethod
    def forward(ctx, phi, Tphi, phi1, Tphi1, phi2, Tphi2, unbiased, diagonal):
        tensors = [_flat(t, n) for t, n in ((phi, "phi"), (Tphi, "Tphi"), (phi1, "phi1"), (Tphi1, "Tphi1"),
                                            (phi2, "phi2"), (Tphi2, "Tphi2"))]
        loss, dphi, d1, d2 = H.nef_loss(*tensors, bool(unbiased), int(diagonal))
        ctx.chunked = d1 is None
        ctx.save_for_backward(dphi, *(() if ctx.chunked else (d1, d2)))
        return loss[0].to(phi.dtype)

    @staticmethod
    def backward(ctx, *grad_outputs):
        if ctx.chunked:
            (dphi,) = ctx.saved_tensors
            return dphi, None, None, None, None, None, None, None
        dphi, d1, d2 = ctx.saved_tensors
        return dphi, None, d1, None, d2, None, None, None


class _NefOperatorFn(torch.autograd.Function):
    """(Tphi, phi) = operator(BatchL2NormalizedFunctions(model), x, importance) in training mode through
    nsvd_nef_operator_forward (running norms updated on the device); the backward is nsvd_nef_operator_backward
    (through phi's centre evaluation and its batch norm only)."""

    @staticmethod
    def forward(ctx, x, bn, prob, path, *params):
        model = bn.base_model
        shape = model.shape
        packed = model.packed_params()
        ws = H.new_workspace(shape, x.shape[0], x.device)
        phi, Tphi, saved = H.nef_operator_forward(shape, packed, prob, x, ws, bn._norm_biased.data,
                                                  bn._norm_unbiased.data, bn._flag(x.device), bn.momentum, path)
        ctx.model, ctx.prob, ctx.path, ctx.ws, ctx.saved = model, prob, path, ws, saved
        ctx.save_for_backward(x)
        ctx.mark_non_differentiable(Tphi)
        return Tphi, phi

    @staticmethod
    def backward(ctx, dTphi, dphi):
        (x,) = ctx.saved_tensors
        model = ctx.model
        grads = model.grad_buffers()
        H.nef_operator_backward(model.shape, model.packed_params(), ctx.prob, x, dphi.contiguous(), ctx.saved,
                                grads.packed, ctx.ws, ctx.path)
        return (None, None, None, None) + tuple(grads.tensors)


def _check_fusable(operator, importance):
    from .operators import OperatorWrapper
    if isinstance(operator, OperatorWrapper) and float(operator.operator.laplacian_eps) <= 0:
        # the reference's exact Laplacian differentiates through BatchL2NormalizedFunctions' batch norm: every sample's
        # Laplacian picks up cross-sample terms of n(x_1 .. x_B) that the per-sample jets here do not carry
        raise NotImplementedError("NeuralEF with batch normalisation and the exact Laplacian (laplacian_eps <= 0): the "
                                  "reference's autograd Laplacian includes cross-sample terms of the batch norm; not "
                                  "built (use laplacian_eps > 0 or batchnorm_mode='none')")


class BatchL2NormalizedFunctions(nn.Module):
    """methods/utils.py:36-86. Same parameters and state_dict keys (``_norm_biased``, ``_norm_unbiased``: (1, neigs),
    requires_grad=False); ``initialized`` is not state, as in the reference. Its value lives in a device int so that a
    training step can be captured in a HIP graph; reading the attribute synchronises."""

    def __init__(self, base_model, neigs, momentum=0.9, batchnorm_mode="unbiased"):
        super().__init__()
        self.base_model = base_model
        self.momentum = momentum
        assert batchnorm_mode in ["biased", "unbiased"]
        self._init_dev = None
        self.batchnorm_mode = batchnorm_mode
        self._norm_biased = nn.Parameter(torch.ones(1, neigs), requires_grad=False)
        self._norm_unbiased = nn.Parameter(torch.ones(1, neigs), requires_grad=False)

    def _flag(self, device) -> torch.Tensor:
        if self._init_dev is None or self._init_dev.device != torch.device(device):
            prev = 0 if self._init_dev is None else int(self._init_dev.item())
            self._init_dev = torch.full((1,), prev, dtype=torch.int32, device=device)
        return self._init_dev

    @property
    def initialized(self) -> bool:
        return self._init_dev is not None and bool(self._init_dev.item())

    @initialized.setter
    def initialized(self, value: bool) -> None:
        self._flag(self._norm_biased.device).fill_(int(bool(value)))

    def forward(self, x):
        """the reference's op sequence around the HIP model (foreign operators, method(x))"""
        output = self.base_model(x).squeeze()
        norm_dims = (0,) if len(output.shape) == 2 else (0, -1)
        if self.training:
            norm = batch_l2norm = output.norm(dim=norm_dims, keepdim=True) / np.sqrt(output.shape[0])
            self.update_norm(batch_l2norm)
        else:
            # (utils.py:55 tests the mode STRING: the biased norm in either mode)
            norm = self._norm_biased if self.batchnorm_mode else self._norm_unbiased
        return output / norm

    @torch.no_grad()
    def update_norm(self, batch_l2norm):
        n = batch_l2norm.detach().reshape(self._norm_biased.shape).to(self._norm_biased.dtype)
        first = self._flag(n.device) == 0
        m = self.momentum
        rb = torch.where(first, n, m * self._norm_biased.data + (1 - m) * n)
        ru = torch.where(first, n, torch.sqrt(m * self._norm_unbiased.data ** 2 + (1 - m) * n ** 2))
        self._norm_biased.data.copy_(rb)
        self._norm_unbiased.data.copy_(ru)
        self._init_dev.fill_(1)

    def register_norm(self, data):
        batch_size = len(data)
        while True:
            try:
                self.register_norm_batch(data, batch_size)
                break
            except Exception:  # noqa: BLE001 (the reference halves the batch on any failure, e.g. out of memory)
                if batch_size <= 1:
                    raise
                batch_size = batch_size // 2

    @torch.no_grad()
    def register_norm_batch(self, data, batch_size):
        num_iters = len(data) // batch_size + (len(data) % batch_size != 0)
        squared_norm = 0.
        for it in range(num_iters):
            idx = range(batch_size * it, min(batch_size * (it + 1), len(data)))
            squared_norm += self.base_model(data[idx]).norm(dim=0) ** 2
        self._norm_biased.data = self._norm_unbiased.data = torch.sqrt(squared_norm / len(data)).reshape(1, -1)

    def apply_operator(self, operator, x, importance=None, path: int = H.PATH_AUTO):
        """Tphi, phi = operator(self, x, importance): fused for OperatorWrapper with Gaussian or no importance in
        training mode; evaluation mode divides the operator's (Tf, f) by the biased running norm (the scale is per head,
        the operator linear); any other density or callable: the reference's op sequence through forward()."""
        from .operators import OperatorWrapper, UniformImportance, fused_problem_of
        if not isinstance(operator, OperatorWrapper):
            if not callable(operator):
                raise NsvdError("compute_loss_operator: operator must be callable as operator(model, x, importance)")
            return operator(self, x, importance=importance) if importance is not None else operator(self, x)
        # (the uniform density is in the operator kernels' epilogue, not in nsvd_nef_operator_forward's)
        if not operator.fused(importance) or (self.training and isinstance(importance, UniformImportance)):
            Tphi, phi = operator.apply_stencil(self, x, importance)
            return Tphi.contiguous(), phi.contiguous()
        model = self.base_model
        prob = fused_problem_of(operator, importance, model)
        x = x.reshape(x.shape[0], -1).float().contiguous()
        if not self.training:
            f, Tf = H.operator_forward(model.shape, model.packed_params(), prob, x,
                                       H.new_workspace(model.shape, x.shape[0], x.device), save_for_backward=False,
                                       path=path)
            H.nef_scale_heads(f, Tf, self._norm_biased.data.contiguous())
            return Tf, f
        _check_fusable(operator, importance)
        return _NefOperatorFn.apply(x, self, prob, path, *model.trainable_tensors())


class NeuralEigenfunctions(nn.Module):
    def __init__(self, model, neigs, batchnorm_mode, sort=False, unbiased=False, include_diag=False,
                 path: int = H.PATH_AUTO):
        self.name = "neuralef"
        super().__init__()
        if batchnorm_mode != "none":
            self.model = BatchL2NormalizedFunctions(model, neigs, batchnorm_mode=batchnorm_mode)
        else:
            self.model = model
        self.unbiased = unbiased  # if True, becomes mu-EigenGame
        self.diagonal = 0 if include_diag else 1
        self.sort = sort
        self.eigvals = None
        self.sort_indices = None
        self.neigs = neigs
        self.path = path

    def forward(self, *args):
        output = self.model(*args)
        if self.sort_indices is not None and self.training:
            return output[:, self.sort_indices, ...]
        return output

    def register_eigvals(self, eigvals):
        self.eigvals = torch.Tensor(eigvals)
        self.sort_indices = torch.sort(self.eigvals)[1].flip(0)

    def reset_eigvals(self):
        self.eigvals = None
        self.sort_indices = None

    def _compute_loss(self, phi, Tphi, phi1, Tphi1, phi2, Tphi2):
        return NeuralEigenfunctionsLossFunction.apply(phi, Tphi, phi1, Tphi1, phi2, Tphi2, self.unbiased, self.diagonal)

    def compute_loss_kernel(self, get_approx_kernel_op, x, importance, split_batch: bool, *args, **kwargs):
        """methods/neuralef.py:108-134: ``get_approx_kernel_op(x)(model, x, importance)`` returns (Kphi, phi) built from
        ``self.model(x)`` (the HIP model); the loss runs on nsvd_nef_loss."""
        model = self.model
        if split_batch:
            x1, x2 = torch.chunk(x, 2)
            Kphi1, phi1 = get_approx_kernel_op(x2)(model, x1, importance=importance)
            Kphi2, phi2 = get_approx_kernel_op(x1)(model, x2, importance=importance)
            phi = torch.cat([phi1, phi2])
            Kphi = torch.cat([Kphi1, Kphi2])
            loss = self._compute_loss(phi, Kphi, phi1, Kphi1, phi2, Kphi2)
        else:
            Kphi, phi = get_approx_kernel_op(x)(model, x, importance=importance)
            loss = self._compute_loss(phi, Kphi, phi, Kphi, phi, Kphi)
        return loss, dict(f=phi, Tf=Kphi, eigvals=None)

    def compute_loss_operator(self, operator, x, importance=None, *args, **kwargs):
        Tphi, phi = self.apply_operator(operator, x, importance)
        phi1, phi2 = torch.chunk(phi, 2)
        Tphi1, Tphi2 = torch.chunk(Tphi, 2)
        loss = self._compute_loss(phi, Tphi, phi1, Tphi1, phi2, Tphi2)
        return loss, dict(f=phi, Tf=Tphi, eigvals=None)

    def apply_operator(self, operator, x, importance=None):
        """Tphi, phi = operator(self.model, x, importance) (methods/neuralef.py:147): self.model is the
        BatchL2NormalizedFunctions (its apply_operator), or with batchnorm_mode 'none' the WaveFunctions itself (the
        operator forward / backward of NestedLoRA's path). Like the reference, no column permutation here."""
        if isinstance(self.model, BatchL2NormalizedFunctions):
            return self.model.apply_operator(operator, x, importance, path=self.path)
        from .nested_lowrank import _OperatorFn
        from .operators import OperatorWrapper, fused_problem_of
        if not isinstance(operator, OperatorWrapper):
            if not callable(operator):
                raise NsvdError("compute_loss_operator: operator must be callable as operator(model, x, importance)")
            return operator(self.model, x, importance=importance) if importance is not None else operator(self.model, x)
        if not operator.fused(importance):
            Tf, f = operator.apply_stencil(self.model, x, importance)
            return Tf.contiguous(), f.contiguous()
        prob = fused_problem_of(operator, importance, self.model)
        x = x.reshape(x.shape[0], -1).float().contiguous()
        return _OperatorFn.apply(x, self, operator, prob, *self.model.trainable_tensors())


_BN_MODES = ("biased", "unbiased", "none")


class NefKernelTrainer(KernelTrainer):
    """NeuralEF's training step on a matrix-free kernel operator (NeuralEigenfunctions.compute_loss_kernel, loss.backward(),
    optimiser - methods/neuralef.py:108-134 with the optimiser of examples/utils.py:48-72) as a fixed sequence of C-ABI
    calls on flat buffers: nsvd_model_forward ONCE on all B rows -> nsvd_nef_rows_forward (the batch norms of the one or
    two segments, phi = u / n in place, the running-norm updates; skipped for batchnorm_mode 'none') -> Kphi, one
    matrix-free product (not split: op.apply_raw(x, x, phi, 1 / B); split: x1, x2 = chunk(x, 2) and ONE
    op.apply_pair_raw(x1, x2, phi2, phi1, 1 / B2, 1 / B1) into the two row ranges of Kphi, every kernel value evaluated
    once) -> nsvd_nef_loss (split: the chunked form; not split: phi1 = phi2 = phi as independent halves) ->
    nsvd_nef_rows_backward (the three cotangents added, then back through u / n(u)) -> nsvd_model_backward ONCE ->
    nsvd_opt_step. No torch autograd, no torch.optim; torch draws the batch. The loss sends no gradient into Kphi
    (neuralef.py:61-62), so there is no swapped-argument product. Single GPU.

    The running norms are updated in the order MatrixFreeKernelOperator.get_approx_kernel_op evaluates the model
    (model(x) first, model(x_ref) only when x_ref is another batch): segment 0 once, or with split_batch segments
    0, 1, 1, 0.

    ``loss`` (1,), ``phi`` and ``Kphi`` (B, L), ``norm_biased`` / ``norm_unbiased`` (L) and ``initialized`` (int32)
    live on the device; nothing is read back in a step."""

    MIN_L, MAX_L = 1, H.NEF_MAX_L

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192, split_batch: bool = False,
                 unbiased: bool = False, include_diag: bool = False, batchnorm_mode: str = "unbiased",
                 bn_momentum: float = 0.9, lr: float = 1e-4, optimizer: str = "rmsprop", rmsprop_decay: float = 0.99,
                 rmsprop_eps: float = 1e-10, momentum: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05,
                 hard_mul_const: float = 1.0, seed: int = 0, index_seed: int = 1):
        if batchnorm_mode not in _BN_MODES:
            raise ValueError(f"NefKernelTrainer: batchnorm_mode must be one of {_BN_MODES}")
        if split_batch and int(batch_size) < 2:
            raise ValueError("NefKernelTrainer: split_batch needs at least 2 rows")
        super().__init__(op, (L, m, hidden), batch_size, index_seed, seed=seed, fourier_scale=fourier_scale,
                         hard_mul_const=hard_mul_const, optimizer=optimizer, lr=lr, rmsprop_decay=rmsprop_decay,
                         rmsprop_eps=rmsprop_eps, momentum=momentum, num_iters=num_iters)
        B, dev, f32 = self.B, self.device, torch.float32
        self.split, self.unbiased, self.diagonal = bool(split_batch), bool(unbiased), 0 if include_diag else 1
        self.batchnorm_mode, self.bn_momentum = batchnorm_mode, float(bn_momentum)
        self.B1 = (B + 1) // 2 if self.split else B  # as torch.chunk splits
        self.B2 = B - self.B1 if self.split else B
        self.order = (0, 1, 1, 0) if self.split else (0,)
        self.model_ws = H.model_workspace(self.shape, B, dev)
        self.ka_ws = op.workspace_pair(self.B1, self.B2, L, dev) if self.split else op.workspace(B, B, L, dev)
        self.phi = torch.empty((B, L), dtype=f32, device=dev)
        self.Kphi = torch.empty_like(self.phi)
        self.dphi = torch.empty_like(self.phi)
        # (not split: the loss returns three gradients for the one phi; nsvd_nef_rows_backward adds them)
        self.dphi1, self.dphi2 = (None, None) if self.split else (torch.empty_like(self.phi), torch.empty_like(self.phi))
        self.loss = torch.zeros(1, dtype=f32, device=dev)
        self.loss_ws = H.nef_loss_scratch(B, self.B1, self.B2, L, dev)
        self.rows_ws = H.nef_rows_workspace(B, L, dev)
        self.stats = torch.ones((2, L), dtype=f32, device=dev) if batchnorm_mode != "none" else None
        self.norm_biased = torch.ones(L, dtype=f32, device=dev)
        self.norm_unbiased = torch.ones(L, dtype=f32, device=dev)
        self.initialized = torch.zeros(1, dtype=torch.int32, device=dev)

    def step(self, x: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the (B, D) coordinate batch x (or a fresh draw); returns ``loss`` (no sync)"""
        x = self._batch(x, "step")
        B1, phi, Kphi = self.B1, self.phi, self.Kphi
        self.model.forward(x, self.model_ws, out=phi)
        if self.stats is not None:
            H.nef_rows_forward(phi, B1, self.norm_biased, self.norm_unbiased, self.initialized, self.bn_momentum,
                               self.order, ws=self.rows_ws, out=phi, stats=self.stats)
        if self.split:
            self.op.apply_pair_raw(x[:B1], x[B1:], phi[B1:], phi[:B1], 1.0 / self.B2, 1.0 / B1, ws=self.ka_ws,
                                   out_x=Kphi[:B1], out_y=Kphi[B1:])
            halves = (phi[:B1], Kphi[:B1], phi[B1:], Kphi[B1:])
        else:
            self.op.apply_raw(x, x, phi, 1.0 / self.B2, ws=self.ka_ws, out=Kphi)
            halves = (phi, Kphi, phi, Kphi)
        H.nef_loss(phi, Kphi, *halves, self.unbiased, self.diagonal,
                   out=(self.loss, self.dphi, self.dphi1, self.dphi2), scratch=self.loss_ws)
        H.nef_rows_backward(phi, self.stats, B1, self.dphi, self.dphi1, self.dphi2, ws=self.rows_ws, out=self.dphi)
        self.model.backward(x, self.dphi, self.model_ws)
        return self._opt_step()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """the evaluation-mode model (NeuralEigenfunctions.forward under eval()): model(x) / norm_biased with either
        batchnorm_mode (utils.py:55 tests the mode string: DESIGN.md 3.9), model(x) itself with 'none'"""
        u = self.model.evaluate(x)
        return u if self.stats is None else u / self.norm_biased

    __call__ = forward

    @torch.no_grad()
    def register_norm(self, data: torch.Tensor) -> None:
        """BatchL2NormalizedFunctions.register_norm (utils.py:70-86): both running norms become the model's column
        norms over ``data`` (n, D), evaluated in batches that are halved whenever one fails"""
        if self.stats is None:
            raise NsvdError("NefKernelTrainer.register_norm: batchnorm_mode 'none' keeps no norms")
        batch_size = len(data)
        while True:
            try:
                sq = sum(self.model.evaluate(data[i:i + batch_size]).norm(dim=0) ** 2
                         for i in range(0, len(data), batch_size))
                break
            except Exception:  # noqa: BLE001 (the reference halves the batch on any failure, e.g. out of memory)
                if batch_size <= 1:
                    raise
                batch_size = batch_size // 2
        self.norm_biased.copy_(torch.sqrt(sq / len(data)))
        self.norm_unbiased.copy_(self.norm_biased)
