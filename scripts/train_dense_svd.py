#!/usr/bin/env python3
"""Learn the singular functions of a stored rectangular matrix with two models (neural_svd_amd.DenseSvdTrainer).

    python scripts/train_dense_svd.py [--steps 20000 --N1 4000 --N2 3000 --dim 2 --sigma-x 1 --sigma-y 0.5 --ell 1.5]

A[i][j] = exp(-|zx_i - zy_j|^2 / (2 ell^2)) on zx ~ N(0, sigma_x^2 I), zy ~ N(0, sigma_y^2 I) (seeded): a cross Gram the
script computes itself and hands over as a matrix - the trainer sees indices and the stored entries, nothing of the
formula. One step is two index draws, two coordinate gathers, two model evaluations, one two-sided product on the
gathered rows (nsvd_kernel_apply_pair: A g and A^T f, no transposed copy), the SVD form of the nested low-rank loss, two
backward passes and two optimiser steps.

Prints steps/s and the learned quotients (DenseCrossOperator.quotients: the models on ALL points) beside
numpy.linalg.svd(A)'s leading values / sqrt(N1 N2) - what the quotients estimate - and beside
kernel_ops.gaussian_cross_singular_values, the population limit of those as N1, N2 grow. Writes the record to
profiles/dense_svd_train.json. The numbers are reported as they come out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd.kernel_ops import DenseCrossOperator, gaussian_cross_singular_values  # noqa: E402
from neural_svd_amd.kernel_svd import DenseSvdTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--N1", type=int, default=4000)
    ap.add_argument("--N2", type=int, default=3000)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--sigma-x", type=float, default=1.0)
    ap.add_argument("--sigma-y", type=float, default=0.5)
    ap.add_argument("--ell", type=float, default=1.5)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--fourier-scale", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_svd_train.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_dense_svd.py needs a GPU (neural_svd_amd has no CPU path)")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(a.seed)
    zx = a.sigma_x * torch.randn(a.N1, a.dim, generator=gen, dtype=torch.float64)
    zy = a.sigma_y * torch.randn(a.N2, a.dim, generator=gen, dtype=torch.float64)
    A = torch.exp(-torch.cdist(zx, zy) ** 2 / (2.0 * a.ell ** 2))
    t0 = time.perf_counter()
    s_mat = np.linalg.svd(A.numpy(), compute_uv=False)[:a.L] / np.sqrt(a.N1 * a.N2)
    t_svd = time.perf_counter() - t0
    s_pop = gaussian_cross_singular_values(a.sigma_x, a.sigma_y, a.ell, a.dim, a.L)
    op = DenseCrossOperator(A.float().to(dev), zx.float().to(dev), zy.float().to(dev))
    kt = DenseSvdTrainer(op, L=a.L, m=a.m, hidden=(128, 128), batch_size=a.B, sequential=True, lr=a.lr,
                         rmsprop_decay=0.999, rmsprop_eps=1e-10, num_iters=a.steps, fourier_scale=a.fourier_scale,
                         seed=a.seed, index_seed=a.seed + 1)
    for _ in range(10):  # code objects, allocator
        kt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps - 10):
        loss = kt.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    got = kt.quotients()
    rel = np.abs(got["svals"] - s_mat) / s_mat
    rec = dict(N1=a.N1, N2=a.N2, dim=a.dim, sigma_x=a.sigma_x, sigma_y=a.sigma_y, ell=a.ell, L=a.L, B=a.B,
               steps=a.steps, lr=a.lr, fourier_scale=a.fourier_scale, seconds=round(dt, 2),
               steps_per_s=round((a.steps - 10) / dt, 1), loss=[float(v) for v in loss.cpu()],
               singular_learned=[float(v) for v in got["svals"]], norms_f=[float(v) for v in got["norms_f"]],
               norms_g=[float(v) for v in got["norms_g"]], singular_of_matrix=[float(v) for v in s_mat],
               numpy_svd_seconds=round(t_svd, 2), singular_population=[float(v) for v in s_pop],
               rel_err_vs_matrix=[float(v) for v in rel], rel_err_leading_three=[float(v) for v in rel[:3]],
               rel_err_mean=float(rel.mean()), rel_err_max=float(rel.max()), device=torch.cuda.get_device_name(0))
    print(f"steps/s {rec['steps_per_s']}   (numpy.linalg.svd of the {a.N1} x {a.N2} matrix: {rec['numpy_svd_seconds']} s)")
    print("  k           learned   svd(A) / sqrt(N1 N2)   rel err    population limit")
    for k in range(a.L):
        print(f"{k:3d}  {got['svals'][k]:16.8e}  {s_mat[k]:16.8e}  {rel[k]:.2e}  {s_pop[k]:16.8e}")
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
