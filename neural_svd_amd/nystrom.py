"""The Nystrom baseline (reference methods/nystrom.py:8-47: ``Nystrom``, ``Nystrom.evd``, ``run_nystrom``) on the GPU.

The reference forms the n x n matrix k(xs, xs), copies it to the host and calls ``np.linalg.eigh`` on it - O(n^3), and
the matrix has to fit. Only the top ``dim`` <= 64 eigenpairs of G = k(xs, xs) / n are kept, so here they come from
block subspace iteration with Rayleigh-Ritz on a basis V of m = min(n, dim + oversample) <= 80 columns:

    V0 = randn(n, m) (seeded device generator), orthonormalised by steps 2-4 with Q = I; then per iteration
    1. W = G V             a matrix-free operator (``RadialKernelOperator``: H.rbf_apply(xs, xs, V, kind, ell, 1 / n);
                           ``DotKernelOperator``: H.dot_apply likewise), through its apply_raw - G is never stored;
                           any other callable kernel(a, b): emp_kernel @ V / n, a library matmul (not the hot path: the
                           reference's own route around the same solver, and the yardstick of the GPU tests)
    2. S = W^T W, A = V^T W, C = V^T V          (m, m) float64                       H.tsgram_f64
    3. eigh(sym(A)) = Q diag(theta) Q^T (descending), M = Q^T S Q,
       r_k = sqrt(max(M_kk - theta_k^2 (2 - q_k^T C q_k), 0)) = |W q_k - theta_k V q_k| for the Ritz pair,
       R = chol(M), T = Q R^-1                  one workgroup, float64               H.ritz_step_f64
       (for an orthonormal V, C = I and r_k^2 = M_kk - theta_k^2; the V that is stored is float32, orthonormal to
       ~1e-8, and the square root of that difference would put a floor of ~1e-4 theta_k under every residual)
    4. V <- W T    the orthonormal basis of span(W), leading columns = Ritz directions  H.ts_rotate

until max_{k < dim} r_k <= tol * theta_0 or ``max_iters``; then eigvecs = V_prev Q[:, :dim], eigvals = theta[:dim]. The
host reads theta, the residuals and the device status in ONE small copy every ``check_every`` iterations; nothing else
in the loop synchronises. The convergence rate is lambda_{m+1} / lambda_dim per iteration: a flat spectrum converges
slowly, and the object says so (``converged``, ``residuals``, a warning) instead of hiding it.
"""
from __future__ import annotations

import math
import time
import warnings

import numpy as np
import torch

from . import hip_ops as H
from .kernel_ops import MatrixFreeKernelOperator

MAX_DIM = 64


def orthonormalize(X, status, ws=None, S=None, theta=None, resid=None, Q=None, T=None, out=None):
    """X chol(X^T X)^-1: the (n, k) float32 block X with its columns orthonormalised among themselves (an upper
    triangular correction; Gram and Cholesky in float64): H.tsgram_f64, H.ritz_step_f64 with A = None, H.ts_rotate.
    status as for H.ritz_step_f64; ws, S (k, k), theta, resid (k), Q, T (k, k) and out (n, k) are the caller's buffers,
    allocated where None."""
    S = H.tsgram_f64(X, None, ws=ws, out_xtx=S)[0]
    T = H.ritz_step_f64(S, None, status, theta, resid, Q, T)[3]
    return H.ts_rotate(X, T, X.shape[1], out=out)


class _Solve:
    """eigvals (dim,) / eigvecs (n, dim) float32 on the device, iterations, relative residuals (dim,), converged"""

    def __init__(self, apply, n, dim, device, oversample, tol, max_iters, check_every, seed):
        m = min(n, dim + int(oversample))
        if m > H.NYSTROM_MAX_BLOCK:
            raise H.NsvdError(f"Nystrom: dim + oversample = {dim + int(oversample)} exceeds the block limit "
                              f"{H.NYSTROM_MAX_BLOCK}")
        if max_iters < 1 or check_every < 1:
            raise ValueError("Nystrom: max_iters and check_every must be at least 1")
        f32, f64 = torch.float32, torch.float64
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        W = torch.randn((n, m), dtype=f32, device=device, generator=gen)
        V, Vn = torch.empty_like(W), torch.empty_like(W)
        S, At = torch.empty((m, m), dtype=f64, device=device), torch.empty((m, m), dtype=f64, device=device)
        Q, T, C = torch.empty_like(S), torch.empty_like(S), torch.empty_like(S)
        # theta | resid | status in one buffer: one device-to-host copy per check
        small = torch.zeros(2 * m + 1, dtype=f64, device=device)
        theta, resid, status = small[:m], small[m:2 * m], small[2 * m:].view(torch.int32)
        ws = H.tsgram_workspace(n, m, device)
        orthonormalize(W, status, ws, S, theta, resid, Q, T, out=V)  # V = V0 chol(V0^T V0)^-1
        H.tsgram_f64(V, None, ws=ws, out_xtx=C)
        self.iterations, self.converged = 0, False
        host = None
        for it in range(1, max_iters + 1):
            apply(V, W)
            H.tsgram_f64(W, V, ws=ws, out_xtx=S, out_xty=At)  # (W^T V = A^T: the solve symmetrises it)
            H.ritz_step_f64(S, At, status, theta, resid, Q, T, C=C)
            H.ts_rotate(W, T, m, out=Vn)
            self.iterations = it
            if it % check_every == 0 or it == max_iters:
                host = small.cpu()
                bits = int(host[2 * m:].view(torch.int32)[0])
                if bits:
                    raise H.NsvdError(f"Nystrom: the small solve failed at iteration <= {it} (status {bits}: "
                                      + ", ".join(s for b, s in ((H.RITZ_BAD_PIVOT, "non-positive Cholesky pivot"),
                                                                 (H.RITZ_SWEEP_CAP, "Jacobi sweep cap")) if bits & b)
                                      + ")")
                th0 = float(host[0])
                worst = float(host[m:m + dim].max())
                if th0 > 0.0 and worst <= tol * th0:
                    self.converged = True
                    break
            if it < max_iters:
                V, Vn = Vn, V
                H.tsgram_f64(V, None, ws=ws, out_xtx=C)
        # (V is still the basis theta, resid and Q of the last iteration belong to)
        self.eigvecs = H.ts_rotate(V, Q, dim)
        self.eigvals = theta[:dim].to(f32)
        th0 = float(host[0])
        self.residuals = (host[m:m + dim] / th0 if th0 > 0.0 else torch.full((dim,), float("inf"), dtype=f64)).clone()
        torch.cuda.synchronize(device)
        if not self.converged:
            warnings.warn(f"Nystrom: not converged after {self.iterations} iterations: worst relative residual "
                          f"{float(self.residuals.max()):.3e} > tol {tol:.1e} (the rate is lambda_(m+1) / lambda_dim "
                          f"per iteration: raise oversample or max_iters)", RuntimeWarning, stacklevel=3)


class Nystrom:
    """only for fixed kernels (the reference's words). kernel: a ``RadialKernelOperator`` or ``DotKernelOperator``
    (matrix-free) or any callable kernel(a, b) -> (len(a), len(b)) matrix on the device; xs: (n, dim_x) on the GPU;
    dim <= 64 eigenpairs.
    Attributes: eigvals (dim,) float32 descending eigenvalues of k(xs, xs) / n, eigvecs (n, dim) unit columns,
    training_time; and iterations, residuals (relative: |G v - theta v| / theta_0, length dim), converged.

    oversample: the basis has m = min(n, dim + oversample) columns. A Gram matrix of FINITE RANK r - a polynomial kernel
    (gamma x.y + coef0)^degree on D coordinates has r = C(D + degree, degree), e.g. 10 at (3, 2) and 20 at (3, 3) - must
    be given m <= r: with dim + oversample above the rank, W = G V has rank r < m, W^T W is rank deficient and the small
    solve reports a non-positive Cholesky pivot (``NsvdError`` names it). Lower ``oversample`` (or ``dim``) so that
    m <= r; the solver is not changed to hide it."""

    def __init__(self, kernel, xs, dim, emp_kernel=None, *, oversample=8, tol=1e-5, max_iters=200, check_every=4,
                 seed=0):
        self.kernel = kernel
        self.dim = int(dim)
        self.xs = self._check(xs, kernel, self.dim)
        start = time.time()
        sol = self._solve(self.xs, kernel, self.dim, emp_kernel, oversample, tol, max_iters, check_every, seed)
        self.training_time = time.time() - start
        self.eigvals, self.eigvecs = sol.eigvals, sol.eigvecs
        self.iterations, self.residuals, self.converged = sol.iterations, sol.residuals, sol.converged

    @staticmethod
    def _check(xs, kernel, dim):
        if not isinstance(xs, torch.Tensor) or not xs.is_cuda:
            raise H.NsvdError("Nystrom: xs must live on the GPU (no CPU path)")
        if xs.dim() != 2:
            raise H.NsvdError("Nystrom: xs must be (n, dim_x)")
        if not 1 <= dim <= MAX_DIM:
            raise H.NsvdError(f"Nystrom: dim must be in 1..{MAX_DIM}")
        if dim > xs.shape[0]:
            raise H.NsvdError(f"Nystrom: dim = {dim} exceeds the number of points {xs.shape[0]}")
        if isinstance(kernel, MatrixFreeKernelOperator) and xs.shape[1] != kernel.dim:
            raise H.NsvdError(f"Nystrom: xs must be (n, {kernel.dim}) for this operator")
        return xs.detach().float().contiguous()

    @staticmethod
    @torch.no_grad()
    def _solve(xs, kernel, dim, emp_kernel, oversample, tol, max_iters, check_every, seed):
        n = xs.shape[0]
        if isinstance(kernel, MatrixFreeKernelOperator) and emp_kernel is None:
            m = min(n, dim + int(oversample))
            ws = kernel.workspace(n, n, m, xs.device)

            def apply(V, W):
                kernel.apply_raw(xs, xs, V, 1.0 / n, ws=ws, out=W)
        else:
            if emp_kernel is None:
                assert kernel is not None, "If emp_kernel is not provided, kernel must be provided"
                emp_kernel = kernel(xs, xs)  # (B, B)
            if not emp_kernel.is_cuda or tuple(emp_kernel.shape) != (n, n):
                raise H.NsvdError("Nystrom: emp_kernel must be (n, n) on the GPU (no CPU path)")
            K = emp_kernel.detach().float().contiguous()

            def apply(V, W):
                torch.matmul(K, V, out=W)
                W.mul_(1.0 / n)
        return _Solve(apply, n, dim, xs.device, oversample, tol, max_iters, check_every, seed)

    def __call__(self, xnew):
        # projection via Nystrom approximation: kernel(xnew, xs) @ eigvecs / eigvals / sqrt(n)
        if isinstance(self.kernel, MatrixFreeKernelOperator):
            if not xnew.is_cuda:
                raise H.NsvdError("Nystrom: xnew must live on the GPU (no CPU path)")
            with torch.no_grad():
                kv = self.kernel.apply_raw(xnew.detach().float().contiguous(), self.xs, self.eigvecs, 1.0)
        else:
            kv = self.kernel(xnew, self.xs) @ self.eigvecs
        return kv / self.eigvals / math.sqrt(self.xs.shape[0])

    @staticmethod
    def evd(xs, kernel, dim, emp_kernel=None):
        """(eigvals, eigvecs, training_time) as numpy arrays, with the defaults of the constructor"""
        start = time.time()
        dim = int(dim)
        xs = Nystrom._check(xs, kernel, dim)
        sol = Nystrom._solve(xs, kernel, dim, emp_kernel, 8, 1e-5, 200, 4, 0)
        eigvals, eigvecs = sol.eigvals.cpu().numpy(), sol.eigvecs.cpu().numpy()
        return eigvals, eigvecs, time.time() - start


def run_nystrom(kernel, neigs, train_data, val_data, log_dir, emp_kernel=None):
    nystrom = Nystrom(kernel, train_data, neigs, emp_kernel)
    eigvals = nystrom.eigvals.cpu().numpy()
    eigfuncs = nystrom(val_data).cpu().numpy()
    np.savez(f'{log_dir}/eigvals.npz', eigvals=eigvals, eigfuncs=eigfuncs)
    return eigvals, eigfuncs, nystrom.training_time
