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
from .kernel_ops import MatrixFreeKernelOperator

_PDE_REASON = ("SpIN.compute_loss_operator is not built: Covariance.backward (methods/spin.py:76-100) sends a gradient "
               "into Tphi; on the PDE path Tphi comes out of the 1 + 2D stencil and the HIP backward does not go through "
               "the stencil (f is the only differentiable output of nsvd_operator_backward). Use compute_loss_kernel "
               "with a MatrixFreeKernelOperator")


def _chunk_rows(B: int, split_batch: bool):
    """(B1, B2): rows that carry Kphi / reference rows, as torch.chunk(x, 2) splits them"""
    if not split_batch:
        return B, B
    B1 = (B + 1) // 2
    if B - B1 < 1:
        raise NsvdError("SpIN: split_batch needs at least 2 rows")
    return B1, B - B1


class _SpinWork:
    """the device buffers of one step shape (B rows, split or not)"""

    def __init__(self, L, B, B1, dev):
        f32, f64 = torch.float32, torch.float64
        self.S = torch.empty((L, L), dtype=f64, device=dev)
        self.Pi = torch.empty((L, L), dtype=f64, device=dev)
        self.le = torch.empty(L + 1, dtype=f64, device=dev)
        self.gsigma = torch.empty((L, L), dtype=f64, device=dev)
        self.gpis = torch.empty((L, L), dtype=f64, device=dev)
        self.ws_all = H.tsgram_workspace(B, L, dev)
        self.ws_1 = H.tsgram_workspace(B1, L, dev)
        self.dK = torch.empty((B1, L), dtype=f32, device=dev)


def _spin_solve_half(op, shape, params, c, x, split_batch, decay, sigma_avg, chol, status, model_ws, ka_ws, work,
                     phi_all, Kphi):
    """steps 1-5 of one step: fills phi_all (B, L), Kphi (B1, L) and the solve's outputs in `work`, updates sigma_avg and
    chol in place"""
    B = x.shape[0]
    B1, B2 = _chunk_rows(B, split_batch)
    H.model_forward(shape, params, x, c, model_ws, save_for_backward=True, out=phi_all)
    if split_batch:
        op.apply_raw(x[:B1], x[B1:], phi_all[B1:], 1.0 / B2, ws=ka_ws, out=Kphi)
        H.tsgram_f64(phi_all, None, ws=work.ws_all, out_xtx=work.S)
        H.tsgram_f64(phi_all[:B1], Kphi, xtx=False, ws=work.ws_1, out_xty=work.Pi)
    else:
        op.apply_raw(x, x, phi_all, 1.0 / B2, ws=ka_ws, out=Kphi)
        H.tsgram_f64(phi_all, Kphi, ws=work.ws_all, out_xtx=work.S, out_xty=work.Pi)
    H.spin_solve(work.S, 1.0 / B, work.Pi, 1.0 / B1, decay, 1.0 / B1, sigma_avg, chol, work.le, work.gsigma, work.gpis,
                 status)


def _spin_term1(op, shape, params, x, split_batch, grads, model_ws, ka_ws_back, work, phi_all, Kphi, dout):
    """step 6: the cotangents of phi and Kphi, the swapped-argument product, one model backward (grads OVERWRITTEN)"""
    B = x.shape[0]
    B1, B2 = _chunk_rows(B, split_batch)
    L = shape.L
    H.ts_rotate(Kphi, work.gpis, L, out=dout[:B1])
    H.ts_rotate(phi_all[:B1], work.gpis, L, out=work.dK)
    if split_batch:
        op.apply_raw(x[B1:], x[:B1], work.dK, 1.0 / B2, ws=ka_ws_back, out=dout[B1:])
    else:
        back = op.apply_raw(x, x, work.dK, 1.0 / B2, ws=ka_ws_back)
        dout.add_(back)
    H.model_backward(shape, params, x, dout, grads, model_ws)


class _SpinLossFn(torch.autograd.Function):
    """loss = trace(Lambda) of one SpIN step on a matrix-free kernel operator. The forward runs steps 1-5 and 7 (term 2
    goes to ``spin._term2``, assigned to the .grad's by the caller); the backward is step 6 and ignores its incoming
    gradient, as SpINFunction.backward does (methods/spin.py:61-73)."""

    @staticmethod
    def forward(ctx, x, spin, op, split_batch, *params):
        model = spin.model
        shape, dev = model.shape, x.device
        B = x.shape[0]
        B1, B2 = _chunk_rows(B, split_batch)
        L = shape.L
        packed = model.packed_params()
        work = _SpinWork(L, B, B1, dev)
        model_ws = H.model_workspace(shape, B, dev)
        ka_ws = op.workspace(B1, B2, L, dev)
        phi_all = torch.empty((B, L), dtype=torch.float32, device=dev)
        Kphi = torch.empty((B1, L), dtype=torch.float32, device=dev)
        term2 = [torch.zeros_like(t.data) for t in model.trainable_tensors()]
        nl = len(shape.dims)
        g2 = H.pack_params(shape, term2[:nl], term2[nl:], None, None)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        c = float(model.hard_mul_const)
        _spin_solve_half(op, shape, packed, c, x, split_batch, float(spin.decay), spin.sigma_avg.data, spin.chol.data,
                         status, model_ws, ka_ws, work, phi_all, Kphi)
        H.spin_jac_step(shape, packed, x[:B1], phi_all[:B1], c, work.gsigma, float(spin.decay), spin.j_avg.data, g2)
        if int(status.item()):
            raise NsvdError("SpIN: cholesky(sigma_avg + 1e-3 I) failed (non-positive or non-finite pivot); the step's "
                            "outputs are zero")
        spin._term2 = term2
        ctx.op, ctx.model, ctx.split, ctx.work, ctx.model_ws = op, model, split_batch, work, model_ws
        ctx.phi_all, ctx.Kphi = phi_all, Kphi
        ctx.save_for_backward(x)
        le = work.le.to(torch.float32)
        loss, eigvals, phi = le[0].clone(), le[1:].clone(), phi_all[:B1]
        ctx.mark_non_differentiable(phi, Kphi, eigvals)
        return loss, phi, Kphi, eigvals

    @staticmethod
    def backward(ctx, *grad_outputs):
        (x,) = ctx.saved_tensors
        model, op = ctx.model, ctx.op
        shape = model.shape
        B = x.shape[0]
        B1, B2 = _chunk_rows(B, ctx.split)
        grads = model.grad_buffers()
        dout = torch.empty((B, shape.L), dtype=torch.float32, device=x.device)
        _spin_term1(op, shape, model.packed_params(), x, ctx.split, grads.packed, ctx.model_ws,
                    op.workspace(B2, B1, shape.L, x.device), ctx.work, ctx.phi_all, ctx.Kphi, dout)
        return (None, None, None, None) + tuple(grads.tensors)


class SpIN(nn.Module):
    def __init__(self, model, neigs, decay, use_vmap=True):
        """
        :param decay:
            0.0 = the moving average is constant (less update)
            1.0 = the moving average has no memory (more update)
        use_vmap is accepted and ignored: the Jacobian contraction is one HIP kernel either way.
        """
        self.name = "spin"
        super().__init__()
        from .models import WaveFunctions
        if not isinstance(model, WaveFunctions):
            raise NotImplementedError("SpIN (HIP): model must be this package's WaveFunctions(ParallelMLP)")
        if model.has_exp_mask or model.box is not None:
            raise NotImplementedError("SpIN (HIP): models with an exponential or box mask are not built (the "
                                      "kernel-operator models have none)")
        if int(neigs) != model.base.num_copies:
            raise ValueError(f"SpIN: neigs = {neigs} but the model has {model.base.num_copies} heads")
        if not 2 <= int(neigs) <= H.SPIN_MAX_L:
            # (the reference's own class fails at neigs = 1: spin_step receives a 0-D pi)
            raise ValueError(f"SpIN: neigs must be in 2..{H.SPIN_MAX_L}")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError("SpIN: decay must be in [0, 1]")
        self.model = model
        self.neigs = int(neigs)
        self.decay = decay
        self.use_vmap = use_vmap
        self.sigma_avg = nn.Parameter(torch.zeros(neigs, neigs), requires_grad=False)
        self.chol = nn.Parameter(torch.zeros(neigs, neigs), requires_grad=False)
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
        op = getattr(get_approx_kernel_op, "__self__", None)
        if not isinstance(op, MatrixFreeKernelOperator) or \
                getattr(get_approx_kernel_op, "__func__", None) is not MatrixFreeKernelOperator.get_approx_kernel_op:
            raise NotImplementedError("SpIN.compute_loss_kernel (HIP): get_approx_kernel_op must be the bound method of a "
                                      "MatrixFreeKernelOperator (the gradient into Kphi is taken through the operator's "
                                      "own matrix-free product); foreign callables are not built")
        if importance is not None:
            raise NotImplementedError("SpIN.compute_loss_kernel (HIP): importance-weighted kernel operators are not built")
        if not x.is_cuda:
            raise NsvdError("SpIN: x must live on the GPU (no CPU path)")
        x = x.detach().reshape(x.shape[0], -1).float().contiguous()
        if x.shape[1] != op.dim:
            raise NsvdError(f"SpIN: x must be (B, {op.dim}) for this operator")
        params = self.model.trainable_tensors()
        loss, phi, Kphi, eigvals = _SpinLossFn.apply(x, self, op, bool(split_batch), *params)
        for p, g in zip(params, self._term2):
            if p.requires_grad:
                p.grad = g
        self._term2 = None
        return loss, dict(f=phi, Tf=Kphi, eigvals=eigvals)

    def compute_loss_operator(self, operator, x, importance, *args, **kwargs):
        raise NotImplementedError(_PDE_REASON)

    def forward(self, x):
        # a wrapper to output orthonormalized eigenfunction (methods/spin.py:209-215)
        return torch.linalg.solve_triangular(self.chol, self.model(x).T, upper=False).T


class SpinKernelTrainer:
    """SpIN's training step on a matrix-free kernel operator (SpIN.compute_loss_kernel, loss.backward(), optimiser -
    methods/spin.py:130-193 with the optimiser of examples/utils.py:48-72) as a fixed sequence of C-ABI calls on flat
    buffers: nsvd_model_forward on all of x -> Kphi (op.apply_raw) -> moments (nsvd_tsgram_f64) -> nsvd_spin_solve ->
    cotangents (nsvd_ts_rotate), the swapped-argument product, nsvd_model_backward (term 1, overwrites the gradient) ->
    nsvd_spin_jac_step (adds term 2) -> nsvd_opt_step. No torch autograd, no torch.optim; torch draws the batch and, with
    split_batch = False, adds the two (B, L) cotangent blocks of term 1. The FusedKernelTrainer counterpart; single GPU.

    ``loss`` = [trace(Lambda) | eigvals] float64 on the device after a step; ``status`` accumulates the solve's failure
    bit (``check()`` reads it and raises)."""

    def __init__(self, op, L: int, m: int, hidden=(128, 128), batch_size: int = 8192, decay: float = 0.01,
                 split_batch: bool = False, lr: float = 1e-4, optimizer: str = "rmsprop", rmsprop_decay: float = 0.99,
                 rmsprop_eps: float = 1e-10, momentum: float = 0.0, num_iters: int = 0, fourier_scale: float = 0.05,
                 hard_mul_const: float = 1.0, seed: int = 0, index_seed: int = 1):
        from .trainer import FlatParams, reference_init
        if not isinstance(op, MatrixFreeKernelOperator):
            raise NotImplementedError("SpinKernelTrainer: a MatrixFreeKernelOperator (radial or dot-product kernel)")
        if not 2 <= int(L) <= H.SPIN_MAX_L:
            raise ValueError(f"SpinKernelTrainer: L must be in 2..{H.SPIN_MAX_L}")
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
        self.j_avg = torch.zeros((L, H.spin_state_floats(self.shape)), dtype=torch.float32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.work = _SpinWork(L, self.B, self.B1, dev)
        self.loss = self.work.le
        self.model_ws = H.model_workspace(self.shape, self.B, dev)
        self.ka_ws = op.workspace(self.B1, self.B2, L, dev)
        self.ka_ws_back = op.workspace(self.B2, self.B1, L, dev)
        self.jac_ws = H.spin_jac_workspace(self.shape, self.B1, dev)
        self.phi_all = torch.empty((self.B, L), dtype=torch.float32, device=dev)
        self.Kphi = torch.empty((self.B1, L), dtype=torch.float32, device=dev)
        self.dout = torch.empty((self.B, L), dtype=torch.float32, device=dev)
        self.gen = torch.Generator(device=dev).manual_seed(index_seed)
        self.t = 0

    @property
    def phi(self) -> torch.Tensor:
        return self.phi_all[:self.B1]

    def step(self, x: torch.Tensor = None) -> torch.Tensor:
        """one optimiser step on the (B, D) coordinate batch x (or a fresh draw); returns ``loss`` (no sync)"""
        from .trainer import cosine_lr
        x = self.op.sample(self.B, self.gen) if x is None else x
        if not x.is_cuda or tuple(x.shape) != (self.B, self.op.dim):
            raise NsvdError(f"SpinKernelTrainer.step: a ({self.B}, {self.op.dim}) coordinate batch on the GPU")
        x = x.float().contiguous()
        # (term 1 overwrites the gradient buffer, term 2 is added to it: the order of the two launches is swapped
        # against the class path, the sum is the same)
        B1, w = self.B1, self.work
        _spin_solve_half(self.op, self.shape, self._params, self.c, x, self.split, self.decay, self.sigma_avg, self.chol,
                         self.status, self.model_ws, self.ka_ws, w, self.phi_all, self.Kphi)
        _spin_term1(self.op, self.shape, self._params, x, self.split, self._grads, self.model_ws, self.ka_ws_back, w,
                    self.phi_all, self.Kphi, self.dout)
        H.spin_jac_step(self.shape, self._params, x[:B1], self.phi_all[:B1], self.c, w.gsigma, self.decay, self.j_avg, self._grads,
                        ws=self.jac_ws)
        lr = cosine_lr(self.lr, self.t, self.num_iters) if self.num_iters > 0 else self.lr
        H.opt_step(self.cfg, self.P.flat, self.P.grad, self._sq, self.P.mom, None, self.t, lr=lr)
        self.t += 1
        return self.loss

    def check(self) -> None:
        """raise if any step since the last check failed its Cholesky factorisation (one small device read)"""
        bits = int(self.status.item())
        self.status.zero_()
        if bits:
            raise NsvdError("SpinKernelTrainer: cholesky(sigma_avg + 1e-3 I) failed in a step since the last check")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """the orthonormalised eigenfunctions (SpIN.forward): chol^-1 applied to model(x)"""
        x = x.float().contiguous()
        f = H.model_forward(self.shape, self._params, x, self.c, H.model_workspace(self.shape, x.shape[0], x.device))
        return torch.linalg.solve_triangular(self.chol, f.T, upper=False).T

    __call__ = forward
