"""The non-parametric baseline of the kernel SVD operators (``kernel_svd``): the top ``dim`` <= 64 singular triplets of
the empirical cross operator C = k(xs, ys) / sqrt(n_x n_y), matrix-free - the counterpart of ``nystrom.Nystrom`` for a
kernel between two samples (the reference has no such baseline; its methods/nystrom.py is the model of the interface).

A two-sided block iteration on bases U (n_x, m), V (n_y, m), m = min(n_x, n_y, dim + oversample) <= 80, float32 with
orthonormal columns:

    U0, V0 = randn (seeded device generator), each orthonormalised as ``Nystrom`` does (``nystrom.orthonormalize``:
    H.tsgram_f64, H.ritz_step_f64 with A = None, H.ts_rotate); then per iteration
    1. (P, R) = (C V, C^T U)    ONE apply_pair_raw(xs, ys, g=V, f=U, 1 / sqrt(n_x n_y), ...) of a matrix-free operator
                                (``RadialKernelOperator``, ``DotKernelOperator``: every kernel value evaluated once; the
                                base class: two products) - C is never stored; any other callable kernel(a, b) or a
                                given emp_kernel: two library matmuls on the stored float32 matrix (not the hot path: the
                                yardstick of the GPU tests)
    2. Sp = P^T P, PtU = P^T U, Cu = U^T U;  Sr = R^T R, RtV = R^T V, Cv = V^T V      two H.tsgram3_f64, float64
    3. Hl = PtU^T, Hr = RtV (both U^T C V up to the float32 rounding of P and R), (Hl + Hr) / 2 = A diag(sigma) B^T,
       Mp = B^T Sp B, Mr = A^T Sr A,
       rl_k = sqrt(max(Mp_kk - 2 sigma_k (A^T Hl B)_kk + sigma_k^2 (A^T Cu A)_kk, 0)) = |P b_k - sigma_k U a_k|,
       rr_k = sqrt(max(Mr_kk - 2 sigma_k (A^T Hr B)_kk + sigma_k^2 (B^T Cv B)_kk, 0)) = |R a_k - sigma_k V b_k|,
       Tu = B chol(Mp)^-1, Tv = A chol(Mr)^-1          one workgroup, float64            H.svd_ritz_step_f64
       (the three-term residuals are identities for ANY U, A, B. The short form Mp_kk - sigma_k^2 assumes an orthonormal U
       and H = U^T P exactly; with U stored in float32 and H an average of two float32-derived matrices its square root
       stalls at ~1e-4 sigma_0 and never reaches tol = 1e-5)
    4. U <- P Tu, V <- R Tv     orthonormal bases of span(P), span(R), the Ritz directions leading     H.ts_rotate

until max_{k < dim} max(rl_k, rr_k) <= tol * sigma_0 or ``max_iters``; then left = U_prev A[:, :dim],
right = V_prev B[:, :dim], svals = sigma[:dim], and left and right are orthonormalised once more among themselves
(``nystrom.orthonormalize`` on the dim stored columns: chol(Mp) in float64 leaves U = P Tu
orthonormal to eps64 cond(P)^2 only, 1e-4 in the trailing columns of a dim = 56 block on a fast-decaying spectrum; the
correction is upper triangular and of that size, so it reaches those columns alone). The host reads sigma | rl | rr | status in ONE small copy every
``check_every`` iterations; nothing else in the loop synchronises. A flat spectrum converges slowly, and the object says
so (``converged``, ``residuals``, a warning) instead of hiding it.
"""
from __future__ import annotations

import math
import time
import warnings

import torch

from . import hip_ops as H
from .kernel_ops import MatrixFreeKernelOperator
from .nystrom import orthonormalize

MAX_DIM = 64


class _Solve:
    """svals (dim,) / left (n_x, dim) / right (n_y, dim) float32 on the device, iterations, relative residuals (dim,),
    converged"""

    def __init__(self, apply_pair, nx, ny, dim, device, oversample, tol, max_iters, check_every, seed):
        m = min(nx, ny, dim + int(oversample))
        if m > H.NYSTROM_MAX_BLOCK:
            raise H.NsvdError(f"NystromSVD: dim + oversample = {dim + int(oversample)} exceeds the block limit "
                              f"{H.NYSTROM_MAX_BLOCK}")
        if max_iters < 1 or check_every < 1:
            raise ValueError("NystromSVD: max_iters and check_every must be at least 1")
        f32, f64 = torch.float32, torch.float64
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        P = torch.randn((nx, m), dtype=f32, device=device, generator=gen)
        R = torch.randn((ny, m), dtype=f32, device=device, generator=gen)
        U, Un, V, Vn = torch.empty_like(P), torch.empty_like(P), torch.empty_like(R), torch.empty_like(R)
        Sp, PtU, Cu, Sr, RtV, Cv, A, B, Tu, Tv = (torch.empty((m, m), dtype=f64, device=device) for _ in range(10))
        # sigma | resid_l | resid_r | status in one buffer: one device-to-host copy per check
        small = torch.zeros(3 * m + 1, dtype=f64, device=device)
        sigma, rl, rr, status = small[:m], small[m:2 * m], small[2 * m:3 * m], small[3 * m:].view(torch.int32)
        ws_u, ws_v = H.tsgram3_workspace(nx, m, device), H.tsgram3_workspace(ny, m, device)
        # U = U0 chol(U0^T U0)^-1, V = V0 chol(V0^T V0)^-1
        for X0, X, n in ((P, U, nx), (R, V, ny)):
            orthonormalize(X0, status, H.tsgram_workspace(n, m, device), Sp, sigma, rl, A, Tu, out=X)
        self.iterations, self.converged = 0, False
        host = None
        for it in range(1, max_iters + 1):
            apply_pair(V, U, P, R)
            H.tsgram3_f64(P, U, ws=ws_u, out_xtx=Sp, out_xty=PtU, out_yty=Cu)
            H.tsgram3_f64(R, V, ws=ws_v, out_xtx=Sr, out_xty=RtV, out_yty=Cv)
            H.svd_ritz_step_f64(PtU, RtV, Sp, Sr, status, Cu, Cv, sigma, rl, rr, A, B, Tu, Tv)
            H.ts_rotate(P, Tu, m, out=Un)
            H.ts_rotate(R, Tv, m, out=Vn)
            self.iterations = it
            if it % check_every == 0 or it == max_iters:
                host = small.cpu()
                bits = int(host[3 * m:].view(torch.int32)[0])
                if bits:
                    raise H.NsvdError(f"NystromSVD: the small solve failed at iteration <= {it} (status {bits}: "
                                      + ", ".join(s for b, s in ((H.RITZ_BAD_PIVOT, "non-positive Cholesky pivot"),
                                                                 (H.RITZ_SWEEP_CAP, "Jacobi sweep cap")) if bits & b)
                                      + ")")
                s0 = float(host[0])
                worst = float(torch.maximum(host[m:m + dim], host[2 * m:2 * m + dim]).max())
                if s0 > 0.0 and worst <= tol * s0:
                    self.converged = True
                    break
            if it < max_iters:
                U, Un, V, Vn = Un, U, Vn, V
        # (U, V are still the bases sigma, the residuals, A and B of the last iteration belong to.) The Ritz vectors, then
        # one more orthonormalisation among themselves: the float64 Cholesky of Mp leaves U = P Tu orthonormal to
        # eps64 cond(P)^2 only, and cond(P) reaches 1e6 when dim is large on a fast-decaying spectrum - 1e-4 in the
        # trailing columns. The correction is upper triangular and of that size: it touches those columns alone.
        self.left, self.right = (orthonormalize(H.ts_rotate(X, Q, dim), status) for X, Q in ((U, A), (V, B)))
        if int(status[0]):
            raise H.NsvdError("NystromSVD: the final orthonormalisation met a non-positive Cholesky pivot")
        self.svals = sigma[:dim].to(f32)
        s0 = float(host[0])
        worst = torch.maximum(host[m:m + dim], host[2 * m:2 * m + dim])
        self.residuals = (worst / s0 if s0 > 0.0 else torch.full((dim,), float("inf"), dtype=f64)).clone()
        torch.cuda.synchronize(device)
        if not self.converged:
            warnings.warn(f"NystromSVD: not converged after {self.iterations} iterations: worst relative residual "
                          f"{float(self.residuals.max()):.3e} > tol {tol:.1e} (the rate is sigma_(m+1) / sigma_dim per "
                          f"iteration: raise oversample or max_iters)", RuntimeWarning, stacklevel=3)


class NystromSVD:
    """only for fixed kernels. kernel: a ``MatrixFreeKernelOperator`` (matrix-free through ``apply_pair_raw``) or any
    callable kernel(a, b) -> (len(a), len(b)) matrix on the device; xs: (n_x, D), ys: (n_y, D) on the GPU;
    1 <= dim <= 64 triplets, dim <= min(n_x, n_y); emp_kernel: k(xs, ys) (n_x, n_y) given instead of computed.
    Attributes: svals (dim,) float32 descending singular values of k(xs, ys) / sqrt(n_x n_y), left (n_x, dim) and
    right (n_y, dim) with unit columns, training_time; and iterations, residuals (relative:
    max(|C v - s u|, |C^T u - s v|) / s_0, length dim), converged.

    ``left_functions(xnew)`` = k(xnew, ys) @ right / svals / sqrt(n_y) and ``right_functions(ynew)`` =
    k(ynew, xs) @ left / svals / sqrt(n_x) are the empirical singular functions, normalised to unit mean square on the
    sample: on the sample itself they return sqrt(n) x the stored vectors, up to the residual.

    oversample: the bases have m = min(n_x, n_y, dim + oversample) columns. A cross Gram of FINITE RANK r - a polynomial
    kernel (gamma x.y + coef0)^degree on D coordinates has r = C(D + degree, degree), e.g. 10 at (3, 2) and 20 at (3, 3) -
    must be given m <= r: with dim + oversample above the rank, P = C V has rank r < m, P^T P is rank deficient and the
    small solve reports a non-positive Cholesky pivot (``NsvdError`` names it). Lower ``oversample`` (or ``dim``) so
    that m <= r; the solver is not changed to hide it."""

    def __init__(self, kernel, xs, ys, dim, emp_kernel=None, *, oversample=8, tol=1e-5, max_iters=200, check_every=4,
                 seed=0):
        self.kernel = kernel
        self.dim = int(dim)
        self.xs, self.ys = self._check(xs, ys, kernel, self.dim)
        start = time.time()
        sol = self._solve(self.xs, self.ys, kernel, self.dim, emp_kernel, oversample, tol, max_iters, check_every, seed)
        self.training_time = time.time() - start
        self.svals, self.left, self.right = sol.svals, sol.left, sol.right
        self.iterations, self.residuals, self.converged = sol.iterations, sol.residuals, sol.converged

    @staticmethod
    def _check(xs, ys, kernel, dim):
        for t, name in ((xs, "xs"), (ys, "ys")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise H.NsvdError(f"NystromSVD: {name} must live on the GPU (no CPU path)")
            if t.dim() != 2:
                raise H.NsvdError(f"NystromSVD: {name} must be (n, dim_x)")
        if xs.shape[1] != ys.shape[1] or xs.device != ys.device:
            raise H.NsvdError("NystromSVD: xs and ys must share the input dimension and the device")
        if not 1 <= dim <= MAX_DIM:
            raise H.NsvdError(f"NystromSVD: dim must be in 1..{MAX_DIM}")
        if dim > min(xs.shape[0], ys.shape[0]):
            raise H.NsvdError(f"NystromSVD: dim = {dim} exceeds the number of points "
                              f"{min(xs.shape[0], ys.shape[0])} of the smaller sample")
        if isinstance(kernel, MatrixFreeKernelOperator) and xs.shape[1] != kernel.dim:
            raise H.NsvdError(f"NystromSVD: xs and ys must be (n, {kernel.dim}) for this operator")
        return xs.detach().float().contiguous(), ys.detach().float().contiguous()

    @staticmethod
    @torch.no_grad()
    def _solve(xs, ys, kernel, dim, emp_kernel, oversample, tol, max_iters, check_every, seed):
        nx, ny = xs.shape[0], ys.shape[0]
        scale = 1.0 / math.sqrt(nx * ny)
        if isinstance(kernel, MatrixFreeKernelOperator) and emp_kernel is None:
            m = min(nx, ny, dim + int(oversample))
            ws = kernel.workspace_pair(nx, ny, m, xs.device)

            def apply_pair(V, U, P, R):
                kernel.apply_pair_raw(xs, ys, V, U, scale, scale, ws=ws, out_x=P, out_y=R)
        else:
            if emp_kernel is None:
                assert kernel is not None, "If emp_kernel is not provided, kernel must be provided"
                emp_kernel = kernel(xs, ys)  # (n_x, n_y)
            if not emp_kernel.is_cuda or tuple(emp_kernel.shape) != (nx, ny):
                raise H.NsvdError("NystromSVD: emp_kernel must be (n_x, n_y) on the GPU (no CPU path)")
            K = emp_kernel.detach().float().contiguous()
            Kt = K.T.contiguous()

            def apply_pair(V, U, P, R):
                torch.matmul(K, V, out=P)
                P.mul_(scale)
                torch.matmul(Kt, U, out=R)
                R.mul_(scale)
        return _Solve(apply_pair, nx, ny, dim, xs.device, oversample, tol, max_iters, check_every, seed)

    def _project(self, new, pts, vecs, name):
        if isinstance(self.kernel, MatrixFreeKernelOperator):
            if not isinstance(new, torch.Tensor) or not new.is_cuda:
                raise H.NsvdError(f"NystromSVD: {name} must live on the GPU (no CPU path)")
            with torch.no_grad():
                kv = self.kernel.apply_raw(new.detach().float().contiguous(), pts, vecs, 1.0)
        else:
            if self.kernel is None:
                raise H.NsvdError("NystromSVD: the singular functions need the kernel (only emp_kernel was given)")
            kv = self.kernel(new, pts) @ vecs
        return kv / self.svals / math.sqrt(pts.shape[0])

    def left_functions(self, xnew):
        """k(xnew, ys) @ right / svals / sqrt(n_y): (len(xnew), dim)"""
        return self._project(xnew, self.ys, self.right, "xnew")

    def right_functions(self, ynew):
        """k(ynew, xs) @ left / svals / sqrt(n_x): (len(ynew), dim) (every kernel served is symmetric in its arguments)"""
        return self._project(ynew, self.xs, self.left, "ynew")
