"""SpIN (Spectral Inference Networks), the third learned method of the paper's comparison, on the matrix-free kernel
operators - with the reference's names and argument meaning (methods/spin.py), backed by the HIP C ABI:

    SpIN(model, neigs, decay, use_vmap=True)                          methods/spin.py:103-215
    SpinKernelTrainer(op, L, m, hidden, batch_size, decay, ...)       the same step on flat buffers, no torch autograd

One step (phi = model(x) at the rows that carry Kphi, B1 of them; phi_sigma = all rows):

    1. sigma = phi_sigma^T phi_sigma / len(phi_sigma), pi = phi^T Kphi / B1          H.tsgram_f64 (float64)
    2. sigma_avg <- (1 - decay) sigma_avg + decay sigma (zeros at the start, no bias correction)
    3. chol = cholesky(sigma_avg + 1e-3 I), Ci = chol^-1
    4. Lambda = Ci pi Ci^T, eigvals = diag(Lambda), loss = trace(Lambda)
    5. gsigma = Ci^T triu(Lambda diag(diag Ci)), gpi = -Ci^T diag(diag Ci)           2-5: H.spin_solve (one workgroup)
    6. term 1 (what loss.backward() accumulates): dphi = Kphi gpi / B1, dKphi = phi gpi / B1   H.ts_rotate
       Kphi = k(x, x_ref) model(x_ref) / B2 with a symmetric k, so dKphi reaches model(x_ref) through one more matrix-free
       product with the arguments swapped, op.apply_raw(x_ref, x, dKphi, 1 / B2); then ONE H.model_backward
    7. term 2 (assigned to p.grad before the backward): j_new[a, c] = (2 / B1) sum_b phi[b, a] d phi_c(x_b) / d p,
       j_avg <- (1 - decay) j_avg + decay j_new, p.grad = sum_{a, c} gsigma[a, c] j_avg[a, c]   H.spin_jac_step

split_batch=True: x1, x2 = chunk(x, 2) (x1 the longer one for an odd batch), Kphi1 = k(x1, x2) phi2 / B2,
phi_sigma = cat[phi1, phi2], Jacobians and pi on x1; split_batch=False: everything on x, x_ref = x.

The reference keeps j_avg as one (L, L, *p.shape) tensor per parameter tensor and takes the per-sample Jacobians with
vmap(jacrev(functional_call)). Head c of ParallelMLP depends on head c's parameters only, so of the L^3 h_i h_{i-1} floats
per layer only L^2 h_i h_{i-1} are ever non-zero: the state here is those alone (``j_avg``: (L, n_trainable), J[a] = one
parameter set), and ``expand_j_avg`` / ``load_j_avg`` convert to and from the reference's tensors.

Only the kernel-operator path exists. ``compute_loss_operator`` raises: Covariance.backward (methods/spin.py:76-100)
sends a gradient into Tphi, on the PDE path Tphi comes out of the 1 + 2D stencil, and the HIP backward does not go through
the stencil (nsvd_operator_backward: f is the only differentiable output). There is no CPU / eager fallback.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import hip_ops as H
from ._lib import NsvdError
from ._spin_step import (StepBuffers, WhitenedKernelTrainer, WhitenedMethod, check_op, check_x, forward_product,
                         swapped_product_backward)
from .trainer import PackedModel

_PDE_REASON = ("SpIN.compute_loss_operator is not built: Covariance.backward (methods/spin.py:76-100) sends a gradient "
               "into Tphi; on the PDE path Tphi comes out of the 1 + 2D stencil and the HIP backward does not go through "
               "the stencil (f is the only differentiable output of nsvd_operator_backward). Use compute_loss_kernel "
               "with a MatrixFreeKernelOperator")


class _SpinWork(StepBuffers):
    """+ SpIN's own: the raw moments, the solve's outputs, the Gram and Jacobian workspaces"""

    def __init__(self, op, shape, B, split, dev):
        super().__init__(op, shape, B, split, dev)
        L, f64 = shape.L, torch.float64
        self.S = torch.empty((L, L), dtype=f64, device=dev)
        self.Pi = torch.empty((L, L), dtype=f64, device=dev)
        self.le = self.loss = torch.empty(L + 1, dtype=f64, device=dev)
        self.gsigma = torch.empty((L, L), dtype=f64, device=dev)
        self.gpis = torch.empty((L, L), dtype=f64, device=dev)
        self.ws_all = H.tsgram_workspace(B, L, dev)
        self.ws_1 = H.tsgram_workspace(self.B1, L, dev)
        self.jac_ws = H.spin_jac_workspace(shape, self.B1, dev)


def _solve_half(model, x, w, decay, sigma_avg, chol):
    """steps 1-5 of one step: fills w.phi_all (B, L), w.Kphi (B1, L) and the solve's outputs in w, updates sigma_avg
    and chol in place"""
    B1 = w.B1
    forward_product(model, x, w)
    if w.split:
        H.tsgram_f64(w.phi_all, None, ws=w.ws_all, out_xtx=w.S)
        H.tsgram_f64(w.phi_all[:B1], w.Kphi, xtx=False, ws=w.ws_1, out_xty=w.Pi)
    else:
        H.tsgram_f64(w.phi_all, w.Kphi, ws=w.ws_all, out_xtx=w.S, out_xty=w.Pi)
    H.spin_solve(w.S, 1.0 / w.B, w.Pi, 1.0 / B1, decay, 1.0 / B1, sigma_avg, chol, w.le, w.gsigma, w.gpis, w.status)


def _term1(model, x, w):
    """step 6: the cotangents of phi and Kphi, the swapped-argument product, one model backward (grads OVERWRITTEN)"""
    B1 = w.B1
    H.ts_rotate(w.Kphi, w.gpis, w.L, out=w.dout[:B1])
    H.ts_rotate(w.phi_all[:B1], w.gpis, w.L, out=w.dK)
    swapped_product_backward(model, x, w, False)


def _term2(model, x, w, decay, j_avg):
    """step 7: the moving average of the Jacobian contraction, ADDED to the gradient buffers"""
    B1 = w.B1
    H.spin_jac_step(model.shape, model.params, x[:B1], w.phi_all[:B1], model.c, w.gsigma, decay, j_avg, model.grads,
                    ws=w.jac_ws)


class _SpinLossFn(torch.autograd.Function):
    """loss = trace(Lambda) of one SpIN step on a matrix-free kernel operator. The forward runs steps 1-5 and 7 (term 2
    goes to ``spin._term2``, assigned to the .grad's by the caller); the backward is step 6 and ignores its incoming
    gradient, as SpINFunction.backward does (methods/spin.py:61-73)."""

    @staticmethod
    def forward(ctx, x, spin, op, split_batch, *params):
        model = spin.model
        shape = model.shape
        w = _SpinWork(op, shape, x.shape[0], split_batch, x.device)
        term2 = [torch.zeros_like(t.data) for t in model.trainable_tensors()]
        nl = len(shape.dims)
        packed = PackedModel(shape, model.packed_params(), H.pack_params(shape, term2[:nl], term2[nl:], None, None),
                             model.hard_mul_const)
        _solve_half(packed, x, w, float(spin.decay), spin.sigma_avg.data, spin.chol.data)
        _term2(packed, x, w, float(spin.decay), spin.j_avg.data)
        if int(w.status.item()):
            raise NsvdError("SpIN: cholesky(sigma_avg + 1e-3 I) failed (non-positive or non-finite pivot); the step's "
                            "outputs are zero")
        spin._term2 = term2
        ctx.model, ctx.work = model, w
        ctx.save_for_backward(x)
        le = w.le.to(torch.float32)
        loss, eigvals, phi = le[0].clone(), le[1:].clone(), w.phi_all[:w.B1]
        ctx.mark_non_differentiable(phi, w.Kphi, eigvals)
        return loss, phi, w.Kphi, eigvals

    @staticmethod
    def backward(ctx, *grad_outputs):
        (x,) = ctx.saved_tensors
        model = ctx.model
        grads = model.grad_buffers()
        _term1(PackedModel(model.shape, model.packed_params(), grads.packed, model.hard_mul_const), x,
               ctx.work.with_backward())
        return (None, None, None, None) + tuple(grads.tensors)


class SpIN(WhitenedMethod):
    def __init__(self, model, neigs, decay, use_vmap=True):
        """decay: WhitenedMethod's. use_vmap is accepted and ignored: the Jacobian contraction is one HIP kernel either
        way."""
        super().__init__("spin", "SpIN", model, neigs, decay)
        self.use_vmap = use_vmap
        # the compact state: row a = one parameter set [ws.. | bs..], j_avg[a][..][c][..] = reference j_avg[a, c, c, ..]
        n = sum(t.numel() for t in model.trainable_tensors())
        self.j_avg = nn.Parameter(torch.zeros(neigs, n), requires_grad=False)
        self._term2 = None

    # ---- checkpoint interchange with the reference's j_avg.<name> tensors ------------------------------------------
    def _named(self):
        """(reference key, parameter) in named_parameters order of the model, the key with '.' -> '_'"""
        return [(n.replace(".", "_"), p) for n, p in self.model.named_parameters()]

    def _slices(self):
        """reference key -> (offset, head-major shape) of the trainable tensors inside one row of j_avg"""
        out, off = {}, 0
        key_of = {id(p): k for k, p in self._named()}
        for t in self.model.trainable_tensors():
            out[key_of[id(t)]] = (off, tuple(t.shape))
            off += t.numel()
        return out

    @torch.no_grad()
    def expand_j_avg(self):
        """the reference's ``j_avg`` ParameterDict contents: {key: (L, L, *p.shape)} (zeros outside head c's slice of
        index [a, c], and for the frozen Fourier matrix). L^2 times the parameter count: for small models only."""
        L, sl, out = self.neigs, self._slices(), {}
        for key, p in self._named():
            full = torch.zeros((L, L) + tuple(p.shape), dtype=self.j_avg.dtype, device=self.j_avg.device)
            if key in sl:
                off, shp = sl[key]
                blk = self.j_avg.data[:, off:off + math.prod(shp)].view((L,) + shp)  # (a, c, ...)
                idx = torch.arange(L, device=full.device)
                full[:, idx, idx] = blk
            out[key] = full
        return out

    @torch.no_grad()
    def load_j_avg(self, tensors):
        """the inverse: takes {key: (L, L, *p.shape)} (keys with or without the ``j_avg.`` prefix) and keeps the
        [a, c, c] slices; entries elsewhere must be zero (they are in every state the reference can reach)"""
        L = self.neigs
        tensors = {k[len("j_avg."):] if k.startswith("j_avg.") else k: v for k, v in tensors.items()}
        for key, (off, shp) in self._slices().items():
            full = tensors[key].to(self.j_avg.device, self.j_avg.dtype)
            if tuple(full.shape) != (L, L) + shp:
                raise NsvdError(f"load_j_avg: {key} must be {(L, L) + shp}, got {tuple(full.shape)}")
            idx = torch.arange(L, device=full.device)
            blk = full[:, idx, idx]  # (a, c, ...)
            rest = full.clone()
            rest[:, idx, idx] = 0
            if bool(rest.count_nonzero()):
                raise NsvdError(f"load_j_avg: {key} has non-zero entries outside the head-diagonal slices")
            self.j_avg.data[:, off:off + math.prod(shp)] = blk.reshape(L, -1)

    # ---- the loss -------------------------------------------------------------------------------------------------
    def compute_loss_kernel(self, get_approx_kernel_op, x, importance, split_batch: bool, *args, **kwargs):
        """methods/spin.py:171-193 for ``get_approx_kernel_op`` = the bound method of a MatrixFreeKernelOperator.
        Returns (loss, dict(f, Tf, eigvals)); assigns term 2 to the model's .grad's, loss.backward() adds term 1."""
        op = check_op("SpIN.compute_loss_kernel", get_approx_kernel_op, importance)
        x = check_x("SpIN", x, op)
        params = self.model.trainable_tensors()
        loss, phi, Kphi, eigvals = _SpinLossFn.apply(x, self, op, bool(split_batch), *params)
        for p, g in zip(params, self._term2):
            if p.requires_grad:
                p.grad = g
        self._term2 = None
        return loss, dict(f=phi, Tf=Kphi, eigvals=eigvals)

    def compute_loss_operator(self, operator, x, importance, *args, **kwargs):
        raise NotImplementedError(_PDE_REASON)


class SpinKernelTrainer(WhitenedKernelTrainer):
    """SpIN's training step on a matrix-free kernel operator (SpIN.compute_loss_kernel, loss.backward(), optimiser -
    methods/spin.py:130-193 with the optimiser of examples/utils.py:48-72) as a fixed sequence of C-ABI calls on flat
    buffers: nsvd_model_forward on all of x -> Kphi (op.apply_raw) -> moments (nsvd_tsgram_f64) -> nsvd_spin_solve ->
    cotangents (nsvd_ts_rotate), the swapped-argument product, nsvd_model_backward (term 1, overwrites the gradient) ->
    nsvd_spin_jac_step (adds term 2) -> nsvd_opt_step. No torch autograd, no torch.optim; torch draws the batch and, with
    split_batch = False, adds the two (B, L) cotangent blocks of term 1. The FusedKernelTrainer counterpart; single GPU.

    ``loss`` = [trace(Lambda) | eigvals] float64 on the device after a step; ``status`` accumulates the solve's failure
    bit (``check()`` reads it and raises)."""

    Work = _SpinWork
    FAILED = "cholesky(sigma_avg + 1e-3 I) failed"

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192, decay: float = 0.01,
                 split_batch: bool = False, lr: float = 1e-4, optimizer: str = "rmsprop", rmsprop_decay: float = 0.99,
                 rmsprop_eps: float = 1e-10, momentum: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05,
                 hard_mul_const: float = 1.0, seed: int = 0, index_seed: int = 1):
        super().__init__(op, (L, m, hidden), batch_size, decay, split_batch, index_seed, seed=seed,
                         fourier_scale=fourier_scale, hard_mul_const=hard_mul_const, optimizer=optimizer, lr=lr,
                         rmsprop_decay=rmsprop_decay, rmsprop_eps=rmsprop_eps, momentum=momentum, num_iters=num_iters)
        self.j_avg = torch.zeros((L, H.spin_state_floats(self.shape)), dtype=torch.float32, device=self.device)

    def step(self, x: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the (B, D) coordinate batch x (or a fresh draw); returns ``loss`` (no sync)"""
        x = self._batch(x, "step")
        # (term 1 overwrites the gradient buffer, term 2 is added to it: the order of the two launches is swapped
        # against the class path, the sum is the same)
        _solve_half(self.model, x, self.work, self.decay, self.sigma_avg, self.chol)
        _term1(self.model, x, self.work)
        _term2(self.model, x, self.work, self.decay, self.j_avg)
        return self._opt_step()
