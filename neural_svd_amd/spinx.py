"""SpINx, the fourth method of the reference's factory (methods/spinx.py), on the matrix-free kernel operators - with
the reference's names, state-dict keys and argument meaning, backed by the HIP C ABI:

    SpINx(model, neigs, decay)                                         methods/spinx.py:75-191
    SpinxKernelTrainer(op, L, m, hidden, batch_size, decay, ...)       the same step on flat buffers, no torch autograd

SpINx keeps SpIN's Cholesky whitening and drops SpIN's per-sample Jacobian contraction: it differentiates straight
through cholesky(sigma + 1e-3 I) of the BATCH sigma and adds one squared-residual loss per eigenfunction. The whole
loss is a function of four L x L moment matrices. One step (P = model(x) on the B1 rows that carry K = Kphi, Phi = all
B rows):

    1. S = Phi^T Phi, and P^T P, P^T K, K^T K                      H.tsgram_f64 (split only) + H.tsgram3_f64, float64
    2. A = cholesky(S / B + 1e-3 I)^-1, lambda_l = a_l^T Gpk a_l, losses = [sum tw_l lambda_l | qk_l - lambda_l^2 (2 - qp_l)],
       loss = sum_k weights_k losses_k / L, and the reverse mode down to five (L, L) matrices; the moving average
       sigma_avg and chol = cholesky(sigma_avg + 1e-3 I) on the side          H.spinx_solve (one workgroup)
    3. dP = P T_pp + K T_kp, dK = P T_pk + K T_kk                              H.ts_rotate2 twice
       split: dPhi[B1:] = Phi[B1:] T_s (+ the swapped product below)           H.ts_rotate
    4. K = k(x, x_ref) model(x_ref) / B2 with a symmetric k: dK reaches model(x_ref) through one more matrix-free
       product with the arguments swapped, op.apply_raw(x_ref, x, dK, 1 / B2); then ONE H.model_backward

split_batch as in SpIN: x1, x2 = chunk(x, 2), K1 = k(x1, x2) phi2 / B2, the sigma rows are cat[phi1, phi2].

Three deviations from the reference, each where the reference cannot be followed literally:
  * SpINx._compute_loss assigns plain tensors to ``sigma_avg`` / ``chol``, registered as nn.Parameter, and raises; the
    intent is SpIN's ``.data`` update (moving average from zeros, no bias correction), which is what runs here.
  * update_weights_operator calls the loss with two arguments and cannot run; only the kernel side exists here, and the
    PDE side raises for the reason below.
  * update_weights_kernel's Jacobian dictionary also holds the frozen Fourier matrix and trace_weights, neither of
    which the optimiser ever updates; the NTK norms here run over the trainable tensors (ws, bs) only.

Only the kernel-operator path exists: the loss sends a gradient into Tphi, on the PDE path Tphi comes out of the 1 + 2D
stencil, and the HIP backward does not go through the stencil. There is no CPU / eager fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import hip_ops as H
from ._lib import NsvdError
from ._spin_step import (StepBuffers, WhitenedKernelTrainer, WhitenedMethod, check_op, check_x, forward_product,
                         swapped_product_backward)
from .trainer import PackedModel

_PDE_REASON = ("SpINx on the PDE operator path is not built: the loss sends a gradient into Tphi (methods/spinx.py:13-23); "
               "on the PDE path Tphi comes out of the 1 + 2D stencil and the HIP backward does not go through the "
               "stencil (f is the only differentiable output of nsvd_operator_backward). Use compute_loss_kernel / "
               "update_weights_kernel with a MatrixFreeKernelOperator")
_FAILED = ("cholesky(sigma + 1e-3 I) failed (non-positive or non-finite pivot of the batch matrix or of the moving "
           "average); the step's outputs are zero")


class _SpinxWork(StepBuffers):
    """+ SpINx's own: the nine (L, L) matrices, the solve's scalars and the Gram workspaces"""

    def __init__(self, op, shape, B, split, dev):
        super().__init__(op, shape, B, split, dev)
        L, f64 = shape.L, torch.float64
        mats = torch.empty((9, L, L), dtype=f64, device=dev)
        self.Gpp, self.Gpk, self.Gkk = mats[1], mats[2], mats[3]
        self.S = mats[0] if split else self.Gpp  # not split: sigma and P^T P are one matrix, B = B1
        self.T_s, self.T_pp, self.T_kp, self.T_pk, self.T_kk = mats[4], mats[5], mats[6], mats[7], mats[8]
        self.out64 = self.loss = torch.empty(2 * L + 2, dtype=f64, device=dev)
        self.ws_all = H.tsgram_workspace(B, L, dev) if split else None
        self.ws_3 = H.tsgram3_workspace(self.B1, L, dev)


def _forward_and_moments(model, x, w):
    """fills w.phi_all (B, L), w.Kphi (B1, L) and the four raw Grams in w"""
    forward_product(model, x, w)
    if w.split:
        H.tsgram_f64(w.phi_all, None, ws=w.ws_all, out_xtx=w.S)
    H.tsgram3_f64(w.phi_all[:w.B1], w.Kphi, ws=w.ws_3, out_xtx=w.Gpp, out_xty=w.Gpk, out_yty=w.Gkk)


def _solve(w, weights, trace_w, decay, sigma_avg, chol, status):
    """sigma_avg and chol: the state to update, or None for neither"""
    H.spinx_solve(w.S, 1.0 / w.B, w.Gpp, w.Gpk, w.Gkk, 1.0 / w.B1, weights, trace_w, decay, sigma_avg is not None,
                  sigma_avg, chol, w.out64, w.T_s, w.T_pp, w.T_kp, w.T_pk, w.T_kk, status)


def _backward(model, x, w):
    """steps 3-4: the cotangents of phi and Kphi, the swapped-argument product, one model backward (grads OVERWRITTEN)"""
    B1, L = w.B1, w.L
    P = w.phi_all[:B1]
    H.ts_rotate2(P, w.T_pp, w.Kphi, w.T_kp, L, out=w.dout[:B1])
    H.ts_rotate2(P, w.T_pk, w.Kphi, w.T_kk, L, out=w.dK)
    if w.split:
        H.ts_rotate(w.phi_all[B1:], w.T_s, L, out=w.dout[B1:])
    swapped_product_backward(model, x, w, True)


def _ntk_weights(who, model, x, w, trace_w, grad_sq):
    """weights = sqrt(sum(ntk) / ntk) (methods/spinx.py:114-132) on the batch x: one forward, one product and the Grams
    once, then per loss k = 0..L the solve with w = L e_k (no state update), the cotangents, the swapped product and one
    model backward; ntk_k = grad_sq(), the squared norm of the gradient model.backward has just written (a 0-D device
    tensor). (L + 1) float64 on the device; a failed solve or a zero norm raises and nothing is stored."""
    L = w.L
    _forward_and_moments(model, x, w)
    e = torch.zeros(L + 1, dtype=torch.float64, device=x.device)
    status = torch.zeros_like(w.status)  # (its own: a failure here raises here and is not left for check())

    def one_hot_grad_sq(k):
        e.zero_()
        e[k] = float(L)
        _solve(w, e, trace_w, 0.0, None, None, status)
        _backward(model, x, w)
        return grad_sq()

    ntk = torch.stack([one_hot_grad_sq(k) for k in range(L + 1)]).double()
    if not bool(((ntk > 0) & torch.isfinite(ntk)).all()):
        raise NsvdError("SpINx.update_weights: an NTK norm is zero or not finite (the weight would be inf); the weights "
                        "are unchanged")
    if int(status.item()):
        raise NsvdError(f"{who}: {_FAILED}; the weights are unchanged")
    return torch.sqrt(ntk.sum() / ntk)


class _SpinxLossFn(torch.autograd.Function):
    """loss = sum_k weights_k losses_k / L of one SpINx step on a matrix-free kernel operator. The forward runs steps
    1-2 (the solve already holds the reverse mode of the small algebra); the backward is steps 3-4, scaled by the
    incoming gradient: ordinary autograd, unlike SpIN's."""

    @staticmethod
    def forward(ctx, x, spinx, op, split_batch, *params):
        model, dev = spinx.model, x.device
        w = _SpinxWork(op, model.shape, x.shape[0], split_batch, dev)
        _forward_and_moments(PackedModel(model.shape, model.packed_params(), None, model.hard_mul_const), x, w)
        _solve(w, spinx.weights.to(dev, torch.float64).contiguous(), spinx._trace_weights_f64(dev), float(spinx.decay),
               spinx.sigma_avg.data, spinx.chol.data, w.status)
        if int(w.status.item()):
            raise NsvdError("SpINx: " + _FAILED)
        ctx.model, ctx.work = model, w
        ctx.save_for_backward(x)
        loss, phi = w.out64[0].to(torch.float32), w.phi_all[:w.B1]
        ctx.mark_non_differentiable(phi, w.Kphi)
        return loss, phi, w.Kphi

    @staticmethod
    def backward(ctx, gloss, *unused):
        (x,) = ctx.saved_tensors
        model = ctx.model
        grads = model.grad_buffers()
        _backward(PackedModel(model.shape, model.packed_params(), grads.packed, model.hard_mul_const), x,
                  ctx.work.with_backward())
        return (None, None, None, None) + tuple(g * gloss.to(g.dtype) for g in grads.tensors)


class SpINxLossFunction(nn.Module):
    """holds ``trace_weights`` under the reference's state-dict key (methods/spinx.py:7-11); the loss itself is
    nsvd_spinx_solve"""

    def __init__(self, neigs):
        super().__init__()
        self.neigs = neigs
        self.trace_weights = nn.Parameter(torch.ones(neigs), requires_grad=False)


class SpINx(WhitenedMethod):
    def __init__(self, model, neigs, decay):
        """decay: WhitenedMethod's"""
        super().__init__("spinx", "SpINx", model, neigs, decay)
        self.spinx_loss_ftn = SpINxLossFunction(self.neigs)
        self.weights = torch.ones(self.neigs + 1)
        self.phi = self.Tphi = None

    def _trace_weights_f64(self, dev):
        return self.spinx_loss_ftn.trace_weights.data.to(dev, torch.float64).contiguous()

    def compute_loss_kernel(self, get_approx_kernel_op, x, importance, split_batch: bool, *args, **kwargs):
        """methods/spinx.py:148-169 for ``get_approx_kernel_op`` = the bound method of a MatrixFreeKernelOperator.
        Returns (loss, dict(f, Tf, eigvals=None)); loss.backward() fills the model's .grad's."""
        op = check_op("SpINx.compute_loss_kernel", get_approx_kernel_op, importance)
        x = check_x("SpINx", x, op)
        loss, phi, Kphi = _SpinxLossFn.apply(x, self, op, bool(split_batch), *self.model.trainable_tensors())
        self.phi, self.Tphi = phi, Kphi
        return loss, dict(f=phi, Tf=Kphi, eigvals=None)

    @torch.no_grad()
    def update_weights_kernel(self, get_approx_kernel_op, x, importance, split_batch):
        """methods/spinx.py:120-132 with the NTK norms over the trainable tensors: one forward, one product and the
        Grams once, then per loss k the solve with w = L e_k (no state update), the cotangents, the swapped product and
        one model backward. Changes ``weights`` only."""
        op = check_op("SpINx.update_weights_kernel", get_approx_kernel_op, importance)
        x = check_x("SpINx", x, op)
        model = self.model
        grads = model.grad_buffers()
        w = _SpinxWork(op, model.shape, x.shape[0], bool(split_batch), x.device).with_backward()
        packed = PackedModel(model.shape, model.packed_params(), grads.packed, model.hard_mul_const)
        weights = _ntk_weights("SpINx.update_weights_kernel", packed, x, w, self._trace_weights_f64(x.device),
                               lambda: sum((g.double() ** 2).sum() for g in grads.tensors))
        self.weights = weights.to(torch.float32).cpu()

    def compute_loss_operator(self, operator, x, importance, *args, **kwargs):
        raise NotImplementedError(_PDE_REASON)

    def compute_losses_operator(self, operator, x, importance, *args, **kwargs):
        raise NotImplementedError(_PDE_REASON)

    def update_weights_operator(self, operator, x, importance, split_batch):
        raise NotImplementedError(_PDE_REASON)


class SpinxKernelTrainer(WhitenedKernelTrainer):
    """SpINx's training step on a matrix-free kernel operator (SpINx.compute_loss_kernel, loss.backward(), optimiser -
    methods/spinx.py:92-99, 148-169 with the optimiser of examples/utils.py:48-72) as a fixed sequence of C-ABI calls on
    flat buffers: nsvd_model_forward on all of x -> Kphi (op.apply_raw) -> nsvd_tsgram_f64 on all rows (split only) ->
    nsvd_tsgram3_f64(P, K) -> nsvd_spinx_solve -> nsvd_ts_rotate2 twice -> nsvd_ts_rotate on rows [B1:] (split only) ->
    the swapped-argument product -> nsvd_model_backward -> nsvd_opt_step. No torch autograd, no torch.optim; torch draws
    the batch and adds the swapped product's (rows, L) block to the cotangent. The SpinKernelTrainer counterpart; single
    GPU.

    ``loss`` = [loss | losses (L + 1) | eigvals (L)] float64 on the device after a step; ``weights`` (L + 1) float64 on
    the device, ones until ``update_weights``; ``trace_weights`` (L) or None for ones; ``status`` accumulates the solve's failure bit (``check()`` reads it)."""

    Work = _SpinxWork
    FAILED = _FAILED

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192, decay: float = 0.01,
                 split_batch: bool = False, lr: float = 1e-4, optimizer: str = "rmsprop", rmsprop_decay: float = 0.99,
                 rmsprop_eps: float = 1e-10, momentum: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05,
                 hard_mul_const: float = 1.0, seed: int = 0, index_seed: int = 1, trace_weights=None):
        super().__init__(op, (L, m, hidden), batch_size, decay, split_batch, index_seed, seed=seed,
                         fourier_scale=fourier_scale, hard_mul_const=hard_mul_const, optimizer=optimizer, lr=lr,
                         rmsprop_decay=rmsprop_decay, rmsprop_eps=rmsprop_eps, momentum=momentum, num_iters=num_iters)
        self.weights = torch.ones(L + 1, dtype=torch.float64, device=self.device)
        # (L) float64 on the device, None = the reference's ones. The loss is MINIMISED, so ones lead to the smallest
        # Rayleigh quotients; the reference reaches the top of a kernel's spectrum by handing the method the negated
        # operator (examples/operator/pde/others.py:30), which is this loss with trace_weights = -1
        self.trace_weights = None if trace_weights is None else \
            torch.as_tensor(trace_weights, dtype=torch.float64).reshape(-1).to(self.device).contiguous()
        if self.trace_weights is not None and self.trace_weights.numel() != L:
            raise ValueError("SpinxKernelTrainer: trace_weights must hold L values")

    def step(self, x: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the (B, D) coordinate batch x (or a fresh draw); returns ``loss`` (no sync)"""
        x = self._batch(x, "step")
        _forward_and_moments(self.model, x, self.work)
        _solve(self.work, self.weights, self.trace_weights, self.decay, self.sigma_avg, self.chol, self.status)
        _backward(self.model, x, self.work)
        return self._opt_step()

    def update_weights(self, x: torch.Tensor = None) -> torch.Tensor:
        """SpINx.update_weights_kernel on x (or a fresh draw): weights = sqrt(sum(ntk) / ntk) over the trainable
        tensors. Changes ``weights`` only (the gradient buffer and ``loss`` are scratch); one device read."""
        grad = self.P.grad
        self.weights.copy_(_ntk_weights("SpinxKernelTrainer.update_weights", self.model, self._batch(x, "update_weights"),
                                        self.work, self.trace_weights, lambda: (grad.double() ** 2).sum()))
        return self.weights
