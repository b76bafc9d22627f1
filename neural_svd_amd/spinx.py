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
from .kernel_ops import MatrixFreeKernelOperator
from .spin import _chunk_rows

_PDE_REASON = ("SpINx on the PDE operator path is not built: the loss sends a gradient into Tphi (methods/spinx.py:13-23); "
               "on the PDE path Tphi comes out of the 1 + 2D stencil and the HIP backward does not go through the "
               "stencil (f is the only differentiable output of nsvd_operator_backward). Use compute_loss_kernel / "
               "update_weights_kernel with a MatrixFreeKernelOperator")
_FAILED = ("cholesky(sigma + 1e-3 I) failed (non-positive or non-finite pivot of the batch matrix or of the moving "
           "average); the step's outputs are zero")


class _SpinxWork:
    """the device buffers of one step shape (B rows, split or not)"""

    def __init__(self, L, B, B1, split, dev):
        f32, f64 = torch.float32, torch.float64
        mats = torch.empty((9, L, L), dtype=f64, device=dev)
        self.Gpp, self.Gpk, self.Gkk = mats[1], mats[2], mats[3]
        self.S = mats[0] if split else self.Gpp  # not split: sigma and P^T P are one matrix, B = B1
        self.T_s, self.T_pp, self.T_kp, self.T_pk, self.T_kk = mats[4], mats[5], mats[6], mats[7], mats[8]
        self.out64 = torch.empty(2 * L + 2, dtype=f64, device=dev)
        self.ws_all = H.tsgram_workspace(B, L, dev) if split else None
        self.ws_3 = H.tsgram3_workspace(B1, L, dev)
        self.dK = torch.empty((B1, L), dtype=f32, device=dev)


def _forward_and_moments(op, shape, params, c, x, split, model_ws, ka_ws, work, phi_all, Kphi):
    """fills phi_all (B, L), Kphi (B1, L) and the four raw Grams in `work`"""
    B = x.shape[0]
    B1, B2 = _chunk_rows(B, split)
    H.model_forward(shape, params, x, c, model_ws, save_for_backward=True, out=phi_all)
    if split:
        op.apply_raw(x[:B1], x[B1:], phi_all[B1:], 1.0 / B2, ws=ka_ws, out=Kphi)
        H.tsgram_f64(phi_all, None, ws=work.ws_all, out_xtx=work.S)
    else:
        op.apply_raw(x, x, phi_all, 1.0 / B2, ws=ka_ws, out=Kphi)
    H.tsgram3_f64(phi_all[:B1], Kphi, ws=work.ws_3, out_xtx=work.Gpp, out_xty=work.Gpk, out_yty=work.Gkk)


def _solve(work, B, B1, weights, trace_w, decay, update_state, sigma_avg, chol, status):
    H.spinx_solve(work.S, 1.0 / B, work.Gpp, work.Gpk, work.Gkk, 1.0 / B1, weights, trace_w, decay, update_state,
                  sigma_avg, chol, work.out64, work.T_s, work.T_pp, work.T_kp, work.T_pk, work.T_kk, status)


def _backward(op, shape, params, x, split, grads, model_ws, ka_ws_back, work, phi_all, Kphi, dout):
    """steps 3-4: the cotangents of phi and Kphi, the swapped-argument product, one model backward (grads OVERWRITTEN)"""
    B = x.shape[0]
    B1, B2 = _chunk_rows(B, split)
    L = shape.L
    P = phi_all[:B1]
    H.ts_rotate2(P, work.T_pp, Kphi, work.T_kp, L, out=dout[:B1])
    H.ts_rotate2(P, work.T_pk, Kphi, work.T_kk, L, out=work.dK)
    if split:
        H.ts_rotate(phi_all[B1:], work.T_s, L, out=dout[B1:])
        dout[B1:].add_(op.apply_raw(x[B1:], x[:B1], work.dK, 1.0 / B2, ws=ka_ws_back))
    else:
        dout.add_(op.apply_raw(x, x, work.dK, 1.0 / B2, ws=ka_ws_back))
    H.model_backward(shape, params, x, dout, grads, model_ws)


class _SpinxLossFn(torch.autograd.Function):
    """loss = sum_k weights_k losses_k / L of one SpINx step on a matrix-free kernel operator. The forward runs steps
    1-2 (the solve already holds the reverse mode of the small algebra); the backward is steps 3-4, scaled by the
    incoming gradient: ordinary autograd, unlike SpIN's."""

    @staticmethod
    def forward(ctx, x, spinx, op, split_batch, *params):
        model = spinx.model
        shape, dev = model.shape, x.device
        B = x.shape[0]
        B1, B2 = _chunk_rows(B, split_batch)
        L = shape.L
        work = _SpinxWork(L, B, B1, split_batch, dev)
        model_ws = H.model_workspace(shape, B, dev)
        phi_all = torch.empty((B, L), dtype=torch.float32, device=dev)
        Kphi = torch.empty((B1, L), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _forward_and_moments(op, shape, model.packed_params(), float(model.hard_mul_const), x, split_batch, model_ws,
                             op.workspace(B1, B2, L, dev), work, phi_all, Kphi)
        _solve(work, B, B1, spinx.weights.to(dev, torch.float64).contiguous(),
               spinx.spinx_loss_ftn.trace_weights.data.to(dev, torch.float64).contiguous(), float(spinx.decay), True,
               spinx.sigma_avg.data, spinx.chol.data, status)
        if int(status.item()):
            raise NsvdError("SpINx: " + _FAILED)
        ctx.op, ctx.model, ctx.split, ctx.work, ctx.model_ws = op, model, split_batch, work, model_ws
        ctx.phi_all, ctx.Kphi = phi_all, Kphi
        ctx.save_for_backward(x)
        loss, phi = work.out64[0].to(torch.float32), phi_all[:B1]
        ctx.mark_non_differentiable(phi, Kphi)
        return loss, phi, Kphi

    @staticmethod
    def backward(ctx, gloss, *unused):
        (x,) = ctx.saved_tensors
        model, op = ctx.model, ctx.op
        shape = model.shape
        B = x.shape[0]
        B1, B2 = _chunk_rows(B, ctx.split)
        grads = model.grad_buffers()
        dout = torch.empty((B, shape.L), dtype=torch.float32, device=x.device)
        _backward(op, shape, model.packed_params(), x, ctx.split, grads.packed, ctx.model_ws,
                  op.workspace(B2, B1, shape.L, x.device), ctx.work, ctx.phi_all, ctx.Kphi, dout)
        return (None, None, None, None) + tuple(g * gloss.to(g.dtype) for g in grads.tensors)


class SpINxLossFunction(nn.Module):
    """holds ``trace_weights`` under the reference's state-dict key (methods/spinx.py:7-11); the loss itself is
    nsvd_spinx_solve"""

    def __init__(self, neigs):
        super().__init__()
        self.neigs = neigs
        self.trace_weights = nn.Parameter(torch.ones(neigs), requires_grad=False)


def _check_op(who, get_approx_kernel_op, importance):
    op = getattr(get_approx_kernel_op, "__self__", None)
    if not isinstance(op, MatrixFreeKernelOperator) or \
            getattr(get_approx_kernel_op, "__func__", None) is not MatrixFreeKernelOperator.get_approx_kernel_op:
        raise NotImplementedError(f"{who} (HIP): get_approx_kernel_op must be the bound method of a "
                                  "MatrixFreeKernelOperator (the gradient into Kphi is taken through the operator's "
                                  "own matrix-free product); foreign callables are not built")
    if importance is not None:
        raise NotImplementedError(f"{who} (HIP): importance-weighted kernel operators are not built")
    return op


def _check_x(x, op):
    if not x.is_cuda:
        raise NsvdError("SpINx: x must live on the GPU (no CPU path)")
    x = x.detach().reshape(x.shape[0], -1).float().contiguous()
    if x.shape[1] != op.dim:
        raise NsvdError(f"SpINx: x must be (B, {op.dim}) for this operator")
    return x


def _ntk_weights(L, one_hot_grad_sq):
    """weights = sqrt(sum(ntk) / ntk) from ntk_k = one_hot_grad_sq(k) (a 0-D device tensor), k = 0..L
    (methods/spinx.py:114-118); a zero norm raises and stores nothing"""
    ntk = torch.stack([one_hot_grad_sq(k) for k in range(L + 1)]).double()
    if not bool(((ntk > 0) & torch.isfinite(ntk)).all()):
        raise NsvdError("SpINx.update_weights: an NTK norm is zero or not finite (the weight would be inf); the weights "
                        "are unchanged")
    return torch.sqrt(ntk.sum() / ntk)


class SpINx(nn.Module):
    def __init__(self, model, neigs, decay):
        """
        :param decay:
            0.0 = the moving average is constant (less update)
            1.0 = the moving average has no memory (more update)
        """
        self.name = "spinx"
        super().__init__()
        from .models import WaveFunctions
        if not isinstance(model, WaveFunctions):
            raise NotImplementedError("SpINx (HIP): model must be this package's WaveFunctions(ParallelMLP)")
        if model.has_exp_mask or model.box is not None:
            raise NotImplementedError("SpINx (HIP): models with an exponential or box mask are not built (the "
                                      "kernel-operator models have none)")
        if int(neigs) != model.base.num_copies:
            raise ValueError(f"SpINx: neigs = {neigs} but the model has {model.base.num_copies} heads")
        if not 2 <= int(neigs) <= H.SPIN_MAX_L:
            raise ValueError(f"SpINx: neigs must be in 2..{H.SPIN_MAX_L}")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError("SpINx: decay must be in [0, 1]")
        self.model = model
        self.neigs = int(neigs)
        self.decay = decay
        self.sigma_avg = nn.Parameter(torch.zeros(neigs, neigs), requires_grad=False)
        self.chol = nn.Parameter(torch.zeros(neigs, neigs), requires_grad=False)
        self.spinx_loss_ftn = SpINxLossFunction(self.neigs)
        self.weights = torch.ones(self.neigs + 1)
        self.phi = self.Tphi = None

    def compute_loss_kernel(self, get_approx_kernel_op, x, importance, split_batch: bool, *args, **kwargs):
        """methods/spinx.py:148-169 for ``get_approx_kernel_op`` = the bound method of a MatrixFreeKernelOperator.
        Returns (loss, dict(f, Tf, eigvals=None)); loss.backward() fills the model's .grad's."""
        op = _check_op("SpINx.compute_loss_kernel", get_approx_kernel_op, importance)
        x = _check_x(x, op)
        loss, phi, Kphi = _SpinxLossFn.apply(x, self, op, bool(split_batch), *self.model.trainable_tensors())
        self.phi, self.Tphi = phi, Kphi
        return loss, dict(f=phi, Tf=Kphi, eigvals=None)

    @torch.no_grad()
    def update_weights_kernel(self, get_approx_kernel_op, x, importance, split_batch):
        """methods/spinx.py:120-132 with the NTK norms over the trainable tensors: one forward, one product and the
        Grams once, then per loss k the solve with w = L e_k (no state update), the cotangents, the swapped product and
        one model backward. Changes ``weights`` only."""
        op = _check_op("SpINx.update_weights_kernel", get_approx_kernel_op, importance)
        x = _check_x(x, op)
        model, split = self.model, bool(split_batch)
        shape, dev = model.shape, x.device
        B, L = x.shape[0], shape.L
        B1, B2 = _chunk_rows(B, split)
        work = _SpinxWork(L, B, B1, split, dev)
        model_ws = H.model_workspace(shape, B, dev)
        phi_all = torch.empty((B, L), dtype=torch.float32, device=dev)
        Kphi = torch.empty((B1, L), dtype=torch.float32, device=dev)
        dout = torch.empty((B, L), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        params, grads = model.packed_params(), model.grad_buffers()
        ka_back = op.workspace(B2, B1, L, dev)
        tw = self.spinx_loss_ftn.trace_weights.data.to(dev, torch.float64).contiguous()
        _forward_and_moments(op, shape, params, float(model.hard_mul_const), x, split, model_ws,
                             op.workspace(B1, B2, L, dev), work, phi_all, Kphi)
        e = torch.zeros(L + 1, dtype=torch.float64, device=dev)

        def grad_sq(k):
            e.zero_()
            e[k] = float(L)
            _solve(work, B, B1, e, tw, 0.0, False, None, None, status)
            _backward(op, shape, params, x, split, grads.packed, model_ws, ka_back, work, phi_all, Kphi, dout)
            return sum((g.double() ** 2).sum() for g in grads.tensors)

        w = _ntk_weights(L, grad_sq)
        if int(status.item()):
            raise NsvdError("SpINx.update_weights_kernel: " + _FAILED + "; the weights are unchanged")
        self.weights = w.to(torch.float32).cpu()

    def compute_loss_operator(self, operator, x, importance, *args, **kwargs):
        raise NotImplementedError(_PDE_REASON)

    def compute_losses_operator(self, operator, x, importance, *args, **kwargs):
        raise NotImplementedError(_PDE_REASON)

    def update_weights_operator(self, operator, x, importance, split_batch):
        raise NotImplementedError(_PDE_REASON)

    def forward(self, x):
        # a wrapper to output orthonormalized eigenfunction (methods/spinx.py:185-191)
        return torch.linalg.solve_triangular(self.chol, self.model(x).T, upper=False).T


class SpinxKernelTrainer:
    """SpINx's training step on a matrix-free kernel operator (SpINx.compute_loss_kernel, loss.backward(), optimiser -
    methods/spinx.py:92-99, 148-169 with the optimiser of examples/utils.py:48-72) as a fixed sequence of C-ABI calls on
    flat buffers: nsvd_model_forward on all of x -> Kphi (op.apply_raw) -> nsvd_tsgram_f64 on all rows (split only) ->
    nsvd_tsgram3_f64(P, K) -> nsvd_spinx_solve -> nsvd_ts_rotate2 twice -> nsvd_ts_rotate on rows [B1:] (split only) ->
    the swapped-argument product -> nsvd_model_backward -> nsvd_opt_step. No torch autograd, no torch.optim; torch draws
    the batch and adds the swapped product's (rows, L) block to the cotangent. The SpinKernelTrainer counterpart; single
    GPU.

    ``loss`` = [loss | losses (L + 1) | eigvals (L)] float64 on the device after a step; ``weights`` (L + 1) float64 on
    the device, ones until ``update_weights``; ``trace_weights`` (L) or None for ones; ``status`` accumulates the solve's failure bit (``check()`` reads it)."""

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192, decay: float = 0.01,
                 split_batch: bool = False, lr: float = 1e-4, optimizer: str = "rmsprop", rmsprop_decay: float = 0.99,
                 rmsprop_eps: float = 1e-10, momentum: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05,
                 hard_mul_const: float = 1.0, seed: int = 0, index_seed: int = 1, trace_weights=None):
        from .trainer import FlatParams, reference_init
        if not isinstance(op, MatrixFreeKernelOperator):
            raise NotImplementedError("SpinxKernelTrainer: a MatrixFreeKernelOperator (radial or dot-product kernel)")
        if not 2 <= int(L) <= H.SPIN_MAX_L:
            raise ValueError(f"SpinxKernelTrainer: L must be in 2..{H.SPIN_MAX_L}")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError("SpinxKernelTrainer: decay must be in [0, 1]")
        self.op, self.device = op, op.device
        dev = self.device
        self.shape = H.ModelShape(L=int(L), D=op.dim, m=int(m), hidden=tuple(hidden), has_exp_mask=False)
        self.B, self.split = int(batch_size), bool(split_batch)
        self.B1, self.B2 = _chunk_rows(self.B, self.split)
        self.decay, self.c = float(decay), float(hard_mul_const)
        self.lr, self.num_iters = float(lr), int(num_iters)
        self.cfg = H.opt_config(optimizer, lr, alpha=rmsprop_decay, eps=rmsprop_eps, momentum=momentum)
        uses_sq, uses_mom = H.opt_uses(self.cfg)
        self.P = FlatParams(self.shape, dev, with_state=True, with_mom=uses_mom)
        self._sq = self.P.sq if uses_sq else None
        fB0, ws0, bs0, _ = reference_init(self.shape, fourier_scale, None, seed)
        self.P.load(fB0, ws0, bs0, None)
        self._params = self.P.pack(self.P.flat, True)
        self._grads = self.P.pack(self.P.grad, False)
        self.sigma_avg = torch.zeros((L, L), dtype=torch.float32, device=dev)
        self.chol = torch.zeros((L, L), dtype=torch.float32, device=dev)
        self.weights = torch.ones(L + 1, dtype=torch.float64, device=dev)
        # (L) float64 on the device, None = the reference's ones. The loss is MINIMISED, so ones lead to the smallest
        # Rayleigh quotients; the reference reaches the top of a kernel's spectrum by handing the method the negated
        # operator (examples/operator/pde/others.py:30), which is this loss with trace_weights = -1
        self.trace_weights = None if trace_weights is None else \
            torch.as_tensor(trace_weights, dtype=torch.float64).reshape(-1).to(dev).contiguous()
        if self.trace_weights is not None and self.trace_weights.numel() != L:
            raise ValueError("SpinxKernelTrainer: trace_weights must hold L values")
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.work = _SpinxWork(L, self.B, self.B1, self.split, dev)
        self.loss = self.work.out64
        self.model_ws = H.model_workspace(self.shape, self.B, dev)
        self.ka_ws = op.workspace(self.B1, self.B2, L, dev)
        self.ka_ws_back = op.workspace(self.B2, self.B1, L, dev)
        self.phi_all = torch.empty((self.B, L), dtype=torch.float32, device=dev)
        self.Kphi = torch.empty((self.B1, L), dtype=torch.float32, device=dev)
        self.dout = torch.empty((self.B, L), dtype=torch.float32, device=dev)
        self.gen = torch.Generator(device=dev).manual_seed(index_seed)
        self.t = 0

    @property
    def phi(self) -> torch.Tensor:
        return self.phi_all[:self.B1]

    def _batch(self, x, who):
        x = self.op.sample(self.B, self.gen) if x is None else x
        if not x.is_cuda or tuple(x.shape) != (self.B, self.op.dim):
            raise NsvdError(f"SpinxKernelTrainer.{who}: a ({self.B}, {self.op.dim}) coordinate batch on the GPU")
        return x.float().contiguous()

    def _gradient(self, x, weights, update_state, status):
        _solve(self.work, self.B, self.B1, weights, self.trace_weights, self.decay, update_state,
               self.sigma_avg if update_state else None, self.chol if update_state else None, status)
        _backward(self.op, self.shape, self._params, x, self.split, self._grads, self.model_ws, self.ka_ws_back, self.work,
                  self.phi_all, self.Kphi, self.dout)

    def step(self, x: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the (B, D) coordinate batch x (or a fresh draw); returns ``loss`` (no sync)"""
        from .trainer import cosine_lr
        x = self._batch(x, "step")
        _forward_and_moments(self.op, self.shape, self._params, self.c, x, self.split, self.model_ws, self.ka_ws,
                             self.work, self.phi_all, self.Kphi)
        self._gradient(x, self.weights, True, self.status)
        lr = cosine_lr(self.lr, self.t, self.num_iters) if self.num_iters > 0 else self.lr
        H.opt_step(self.cfg, self.P.flat, self.P.grad, self._sq, self.P.mom, None, self.t, lr=lr)
        self.t += 1
        return self.loss

    def update_weights(self, x: torch.Tensor = None) -> torch.Tensor:
        """SpINx.update_weights_kernel on x (or a fresh draw): weights = sqrt(sum(ntk) / ntk) over the trainable
        tensors. Changes ``weights`` only (the gradient buffer and ``loss`` are scratch); one device read."""
        x = self._batch(x, "update_weights")
        L = self.shape.L
        _forward_and_moments(self.op, self.shape, self._params, self.c, x, self.split, self.model_ws, self.ka_ws,
                             self.work, self.phi_all, self.Kphi)
        e = torch.zeros(L + 1, dtype=torch.float64, device=self.device)
        status = torch.zeros_like(self.status)  # (its own: a failure here raises here and is not left for check())

        def grad_sq(k):
            e.zero_()
            e[k] = float(L)
            self._gradient(x, e, False, status)
            return (self.P.grad.double() ** 2).sum()

        w = _ntk_weights(L, grad_sq)
        if int(status.item()):
            raise NsvdError("SpinxKernelTrainer.update_weights: " + _FAILED + "; the weights are unchanged")
        self.weights.copy_(w)
        return self.weights

    def check(self) -> None:
        """raise if any step since the last check failed a Cholesky factorisation (one small device read)"""
        bits = int(self.status.item())
        self.status.zero_()
        if bits:
            raise NsvdError("SpinxKernelTrainer: " + _FAILED + " in a step since the last check")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """the orthonormalised eigenfunctions (SpINx.forward): chol^-1 applied to model(x)"""
        x = x.float().contiguous()
        f = H.model_forward(self.shape, self._params, x, self.c, H.model_workspace(self.shape, x.shape[0], x.device))
        return torch.linalg.solve_triangular(self.chol, f.T, upper=False).T

    __call__ = forward
