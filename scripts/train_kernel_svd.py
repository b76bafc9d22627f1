#!/usr/bin/env python3
"""Learn the singular functions of a cross-domain kernel with two models (neural_svd_amd.KernelSvdTrainer).

    python scripts/train_kernel_svd.py [--steps 20000 --dim 2 --sigma-x 1 --sigma-y 0.5 --ell 1.5 --L 10 --B 8192]
    python scripts/train_kernel_svd.py --kind polynomial --dim 3 --degree 2 --L 10 [--gamma 1 --coef0 1]
    python scripts/train_kernel_svd.py --kind arccos1 --dim 3
    python scripts/train_kernel_svd.py --kind exponential --baseline 8192
    python scripts/train_kernel_svd.py --kind relu_nngp --depth 3 --gamma 2 --coef0 0.1 --dim 3 --baseline 8192

--baseline N: draw N points a side from the two measures, run the matrix-free truncated SVD of their cross Gram
(neural_svd_amd.NystromSVD: the singular values of k(xs, ys) / N) and print its singular values as a comparison column -
the only one for the exponential and arccos1 kinds, an extra one beside the closed form otherwise - with the relative
error of the learned quotients against it; the record gains baseline_n, baseline_svals, baseline_iterations,
baseline_seconds, rel_err_vs_baseline. Without the flag the output and the record are as before.

--kind gaussian (the default, described below) | exponential (--ell) | polynomial (--gamma --coef0 --degree:
k = (gamma x.y + coef0)^degree) | arccos1 (the order-1 arc-cosine kernel) | relu_nngp, relu_ntk (the NNGP kernel and the
neural tangent kernel of a ReLU network --depth layers deep, weight variance --gamma, bias variance --coef0; --baseline
is their comparison column). The radial kinds run on nsvd_rbf_apply_pair,
the dot-product kinds on nsvd_dot_apply_pair; the two-call comparison trainer uses two nsvd_rbf_apply / nsvd_dot_apply
calls. The truth column comes from a closed form where one exists - gaussian: gaussian_cross_singular_values,
polynomial: polynomial_cross_singular_values (finite rank: zeros beyond it, where the relative error is not defined) -
and the other kinds print the learned quotients only. The default output file is profiles/kernel_svd_train.json for the
Gaussian kind and profiles/kernel_svd_train_<kind>.json for the others.

k(x, y) = exp(-|x - y|^2 / (2 ell^2)) as an operator from L2(N(0, sigma_y^2 I)) to L2(N(0, sigma_x^2 I)): x and y are
drawn fresh every step from the two measures, f takes x and g takes y, and one step is two model evaluations, one
two-sided kernel product (nsvd_rbf_apply_pair: K g and K^T f, every kernel value evaluated once), the SVD form of the
nested low-rank loss, two backward passes and two optimiser steps - all C-ABI calls on flat buffers.

Prints steps/s with the two-sided call and with the two-call base path (two nsvd_rbf_apply calls with swapped arguments:
--base-steps steps of a second trainer), and the learned singular-value quotients diag(F^T K G) / (|F_l| |G_l|) from
kernel_ops.kernel_singular_values on --n-eval held-out samples a side beside the closed form
(kernel_ops.gaussian_cross_singular_values). Writes the record to profiles/kernel_svd_train.json. The numbers are
reported as they come out."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import hip_ops as H  # noqa: E402
from neural_svd_amd.kernel_ops import (DotKernelOperator, MatrixFreeKernelOperator, RadialKernelOperator,  # noqa: E402
                                       gaussian_cross_singular_values, kernel_singular_values,
                                       polynomial_cross_singular_values)
from neural_svd_amd.kernel_svd import KernelSvdTrainer  # noqa: E402
from neural_svd_amd.nystrom_svd import NystromSVD  # noqa: E402


def two_call(op_class):
    """the same operator class with the base class's two-sided product: two apply_raw calls with swapped arguments"""
    return type("TwoCall" + op_class.__name__, (op_class,),
                dict(workspace_pair=MatrixFreeKernelOperator.workspace_pair,
                     apply_pair_raw=MatrixFreeKernelOperator.apply_pair_raw))


def timed_steps(trainer, n):
    for _ in range(10):  # code objects, allocator
        trainer.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n - 10):
        loss = trainer.step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--base-steps", type=int, default=2000, help="steps of the two-call trainer (timing only)")
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--sigma-x", type=float, default=1.0)
    ap.add_argument("--sigma-y", type=float, default=0.5)
    ap.add_argument("--kind", default="gaussian", choices=("gaussian", "exponential", "polynomial", "arccos1", "relu_nngp", "relu_ntk"))
    ap.add_argument("--ell", type=float, default=1.5, help="radial kinds: the length scale")
    ap.add_argument("--gamma", type=float, default=1.0, help="polynomial kind; relu kinds: the weight variance")
    ap.add_argument("--coef0", type=float, default=1.0, help="polynomial kind; relu kinds: the bias variance")
    ap.add_argument("--degree", type=int, default=2, help="polynomial kind")
    ap.add_argument("--depth", type=int, default=1, help="relu kinds: the number of layers, 1..8")
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--fourier-scale", type=float, default=0.3)
    ap.add_argument("--n-eval", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--baseline", type=int, default=None, metavar="N",
                    help="comparison column: NystromSVD on N fresh points a side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_kernel_svd.py needs a GPU (neural_svd_amd has no CPU path)")
    dev = "cuda:0"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles",
                             "kernel_svd_train.json" if a.kind == "gaussian" else f"kernel_svd_train_{a.kind}.json")
    radial = a.kind in ("gaussian", "exponential")
    base_class = RadialKernelOperator if radial else DotKernelOperator

    def make_op(op_class):
        if radial:
            return op_class(H.RBF_GAUSSIAN if a.kind == "gaussian" else H.RBF_EXPONENTIAL, a.ell, a.dim, a.sigma_x, dev)
        hkind = dict(polynomial=H.DOT_POLYNOMIAL, arccos1=H.DOT_ARCCOS1, relu_nngp=H.DOT_RELU_NNGP,
                     relu_ntk=H.DOT_RELU_NTK)[a.kind]
        return op_class(hkind, a.dim, gamma=a.gamma, coef0=a.coef0, degree=a.degree, depth=a.depth, sigma=a.sigma_x,
                        device=dev)

    def trainer(op_class, steps):
        op = make_op(op_class)
        return op, KernelSvdTrainer(op, L=a.L, m=a.m, hidden=(128, 128), batch_size=a.B, sigma_x=a.sigma_x,
                                    sigma_y=a.sigma_y, sequential=True, lr=a.lr, rmsprop_decay=0.999, rmsprop_eps=1e-10,
                                    num_iters=steps, fourier_scale=a.fourier_scale, seed=a.seed, index_seed=a.seed + 1)
    op, kt = trainer(base_class, a.steps)
    dt, loss = timed_steps(kt, a.steps)
    _, kt2 = trainer(two_call(base_class), a.base_steps)
    dt2, _ = timed_steps(kt2, a.base_steps)
    gen = torch.Generator(device=dev).manual_seed(a.seed + 1000)
    x_eval = a.sigma_x * torch.randn(a.n_eval, a.dim, device=dev, generator=gen)
    y_eval = a.sigma_y * torch.randn(a.n_eval, a.dim, device=dev, generator=gen)
    got = kernel_singular_values(op, kt.f, kt.g, x_eval, y_eval)
    if a.kind == "gaussian":
        s = gaussian_cross_singular_values(a.sigma_x, a.sigma_y, a.ell, a.dim, a.L)
    elif a.kind == "polynomial":
        s = polynomial_cross_singular_values(a.sigma_x, a.sigma_y, a.gamma, a.coef0, a.degree, a.dim, a.L)
    else:
        s = None  # no closed form: quotients only
    rec = dict(kind=a.kind, dim=a.dim, sigma_x=a.sigma_x, sigma_y=a.sigma_y, L=a.L, B=a.B, steps=a.steps,
               lr=a.lr, fourier_scale=a.fourier_scale, seconds=round(dt, 2),
               steps_per_s=round((a.steps - 10) / dt, 1),
               two_call_base_path_steps=a.base_steps, two_call_base_path_steps_per_s=round((a.base_steps - 10) / dt2, 1),
               loss=[float(v) for v in loss.cpu()], singular_learned=[float(v) for v in got["svals"]],
               norms_f=[float(v) for v in got["norms_f"]], norms_g=[float(v) for v in got["norms_g"]],
               n_eval=a.n_eval, device=torch.cuda.get_device_name(0))
    if radial:
        rec.update(ell=a.ell)
    elif a.kind == "polynomial":
        rec.update(gamma=a.gamma, coef0=a.coef0, degree=a.degree)
    elif a.kind in ("relu_nngp", "relu_ntk"):
        rec.update(gamma=a.gamma, coef0=a.coef0, depth=a.depth)
    names = ("nsvd_rbf_apply", "nsvd_rbf_apply_pair") if radial else ("nsvd_dot_apply", "nsvd_dot_apply_pair")
    print(f"steps/s {rec['steps_per_s']} (two {names[0]} calls in place of {names[1]}: "
          f"{rec['two_call_base_path_steps_per_s']})")
    base = None
    if a.baseline is not None:
        # a polynomial kernel has finite rank: the block may not be wider than it (NystromSVD's note on oversample)
        rank = math.comb(a.dim + a.degree, a.degree) if a.kind == "polynomial" else a.baseline
        bdim = min(a.L, rank, a.baseline)
        gen_b = torch.Generator(device=dev).manual_seed(a.seed + 2000)
        xs_b = a.sigma_x * torch.randn(a.baseline, a.dim, device=dev, generator=gen_b)
        ys_b = a.sigma_y * torch.randn(a.baseline, a.dim, device=dev, generator=gen_b)
        sol = NystromSVD(op, xs_b, ys_b, bdim, oversample=min(8, rank - bdim), seed=a.seed)
        base = np.full(a.L, np.nan)
        base[:bdim] = sol.svals.double().cpu().numpy()
        ok = np.isfinite(base) & (base > 0)
        rel_b = np.full(a.L, np.nan)
        rel_b[ok] = np.abs(got["svals"][ok] - base[ok]) / base[ok]
        rec.update(baseline_n=a.baseline, baseline_svals=[None if np.isnan(v) else float(v) for v in base],
                   baseline_iterations=sol.iterations, baseline_seconds=round(sol.training_time, 4),
                   baseline_converged=bool(sol.converged),
                   rel_err_vs_baseline=[None if np.isnan(v) else float(v) for v in rel_b])
    if s is not None:
        nz = s > 0  # (a polynomial kernel has finite rank: no relative error beyond it)
        rel = np.full(a.L, np.nan)
        rel[nz] = np.abs(got["svals"][nz] - s[nz]) / s[nz]
        rec.update(singular_closed_form=[float(v) for v in s], rel_err=[None if np.isnan(v) else float(v) for v in rel],
                   rel_err_leading_three=[float(v) for v in rel[:3][nz[:3]]], rel_err_mean=float(rel[nz].mean()),
                   rel_err_max=float(rel[nz].max()), rank_within_L=int(nz.sum()))
    def err(v):
        return "-       " if np.isnan(v) else f"{v:.2e}"
    if s is not None and base is not None:
        print(f"  k           learned       closed form   rel err   baseline n={a.baseline}   rel err")
        for k in range(a.L):
            print(f"{k:3d}  {got['svals'][k]:16.8e}  {s[k]:16.8e}  {err(rel[k])}  {base[k]:16.8e}  {err(rel_b[k])}")
    elif s is not None:
        print("  k           learned       closed form   rel err")
        for k in range(a.L):
            print(f"{k:3d}  {got['svals'][k]:16.8e}  {s[k]:16.8e}  " + (f"{rel[k]:.2e}" if nz[k] else "-"))
    elif base is not None:
        print(f"  k           learned   baseline n={a.baseline}   rel err   (no closed form for this kind)")
        for k in range(a.L):
            print(f"{k:3d}  {got['svals'][k]:16.8e}  {base[k]:16.8e}  {err(rel_b[k])}")
    else:
        print("  k           learned   (no closed form for this kind)")
        for k in range(a.L):
            print(f"{k:3d}  {got['svals'][k]:16.8e}")
    if base is not None:
        print(f"baseline: NystromSVD on {a.baseline} points a side, {rec['baseline_iterations']} iterations, "
              f"{rec['baseline_seconds']} s, converged {rec['baseline_converged']}")
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
