#!/usr/bin/env python3
"""End-to-end run of the matrix-free kernel-operator path: FusedKernelTrainer on a RadialKernelOperator learns the top
eigenfunctions of the Gaussian kernel exp(-|x - y|^2 / (2 ell^2)) under N(0, sigma^2 I) from coordinate batches drawn
fresh every step, and the Rayleigh quotients of the learned functions on a held-out sample (kernel_spectrum) are
compared with the closed-form Mercer eigenvalues (gaussian_kernel_eigvals).

    python scripts/train_rbf_kernel.py [--steps 20000 --dim 2 --sigma 1 --ell 1.5 --L 10 --B 8192]
    python scripts/train_rbf_kernel.py --kind exponential --ell 2 --nystrom 8192
    python scripts/train_rbf_kernel.py --kind arccos1 --dim 3 --nystrom 8192
    python scripts/train_rbf_kernel.py --kind polynomial --gamma 0.5 --coef0 1 --degree 3 --dim 3 --nystrom 8192
    python scripts/train_rbf_kernel.py --kind relu_ntk --depth 3 --gamma 2 --coef0 0.1 --dim 3 --nystrom 8192

--kind polynomial / arccos1 train on a DotKernelOperator instead (k = (gamma x.y + coef0)^degree, or Cho & Saul's order-1
arc-cosine kernel; --ell unused) and write profiles/dot_kernel_train.json by default.
--kind relu_nngp / relu_ntk train on the NNGP kernel / the neural tangent kernel of a ReLU network --depth layers deep
(1..8) with weight variance --gamma and bias variance --coef0 (DotKernelOperator's recursion) and write
profiles/relu_kernel_train_<kind>.json by default; --nystrom is their comparison column.
--spin adds a SpIN column (neural_svd_amd.spin.SpinKernelTrainer: the same model, batch size and step count trained with
SpIN's loss; --spin-decay is its moving-average rate) with its own steps/s.
--spinx adds a SpINx column (neural_svd_amd.spinx.SpinxKernelTrainer, the same way; --spinx-decay its moving-average
rate, --spinx-lr its learning rate, --spinx-weight-freq N re-weights the L + 1 losses by their NTK norms every N steps,
0 = never) with its own steps/s (the weight updates are inside the timed loop).
--neuralef adds a NeuralEF column (neural_svd_amd.neuralef.NefKernelTrainer, the same way; --neuralef-unbiased makes
it mu-EigenGame, --neuralef-lr is its learning rate) with its own steps/s; its functions come out in no fixed order, so
the sorted quotients are the ones compared.
--nystrom N adds the Nystrom baseline (neural_svd_amd.Nystrom, matrix-free) on an N-point sample as a comparison
column: the only one the exponential and the two dot-product kinds have, since their spectra have no closed form here.
(A polynomial kernel has rank C(dim + degree, degree): keep L + 8 at or below it, see Nystrom's note on oversample.)

Prints steps/s and the relative errors; writes the record to profiles/rbf_kernel_train.json. The quotients are taken
under the EMPIRICAL measure of --n-eval samples: their own float64 sampling gap to lambda_k is reported beside them
(the analytic eigenfunctions through the same evaluation)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import hip_ops as H  # noqa: E402
from neural_svd_amd.kernel_ops import (DotKernelOperator, FusedKernelTrainer, RadialKernelOperator,  # noqa: E402
                                       gaussian_kernel_eigenfunctions, gaussian_kernel_eigvals, kernel_spectrum)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--ell", type=float, default=1.5)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--fourier-scale", type=float, default=0.3)
    ap.add_argument("--n-eval", type=int, default=16384)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kind", choices=("gaussian", "exponential", "polynomial", "arccos1", "relu_nngp", "relu_ntk"),
                    default="gaussian")
    ap.add_argument("--gamma", type=float, default=1.0, help="polynomial kind: k = (gamma x.y + coef0)^degree; relu kinds: the weight variance")
    ap.add_argument("--coef0", type=float, default=1.0, help="relu kinds: the bias variance")
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--depth", type=int, default=1, help="relu kinds: the number of layers, 1..8")
    ap.add_argument("--nystrom", type=int, default=0, metavar="N",
                    help="also print the Nystrom eigenvalues of an N-point sample (0: off)")
    ap.add_argument("--spin", action="store_true", help="also train SpIN on the same operator and print its column")
    ap.add_argument("--spin-decay", type=float, default=0.01)
    ap.add_argument("--spin-lr", type=float, default=None, help="default: --lr")
    ap.add_argument("--spinx", action="store_true", help="also train SpINx on the same operator and print its column")
    ap.add_argument("--spinx-decay", type=float, default=0.01)
    ap.add_argument("--spinx-lr", type=float, default=None, help="default: --lr")
    ap.add_argument("--spinx-weight-freq", type=int, default=0, metavar="N",
                    help="SpINx: update the loss weights every N steps (0: never)")
    ap.add_argument("--neuralef", action="store_true",
                    help="also train NeuralEF on the same operator and print its column")
    ap.add_argument("--neuralef-unbiased", action="store_true", help="NeuralEF: the mu-EigenGame form")
    ap.add_argument("--neuralef-lr", type=float, default=None, help="default: --lr")
    ap.add_argument("--out", default=None,
                    help="default: profiles/rbf_kernel_train.json (radial kinds) or profiles/dot_kernel_train.json")
    a = ap.parse_args()
    relu = a.kind in ("relu_nngp", "relu_ntk")
    dot = relu or a.kind in ("polynomial", "arccos1")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", f"relu_kernel_train_{a.kind}.json" if relu else
                             "dot_kernel_train.json" if dot else "rbf_kernel_train.json")
    if not torch.cuda.is_available():
        raise SystemExit("train_rbf_kernel.py needs a GPU (neural_svd_amd has no CPU path)")
    dev = "cuda:0"
    gaussian = a.kind == "gaussian"
    if a.kind == "polynomial":
        import math
        rank = math.comb(a.dim + a.degree, a.degree)
        need = a.L + 8 if a.nystrom else a.L
        if rank < need:
            raise SystemExit(f"train_rbf_kernel.py: (gamma x.y + coef0)^{a.degree} on {a.dim} coordinates has rank "
                             f"C({a.dim + a.degree}, {a.degree}) = {rank}, below " +
                             (f"L + 8 = {need} (the Nystrom basis, see Nystrom's note on oversample)" if a.nystrom
                              else f"L = {need}") + ": raise --dim or --degree, or lower --L")
    if dot:
        hkind = dict(polynomial=H.DOT_POLYNOMIAL, arccos1=H.DOT_ARCCOS1, relu_nngp=H.DOT_RELU_NNGP,
                     relu_ntk=H.DOT_RELU_NTK)[a.kind]
        op = DotKernelOperator(hkind, a.dim, gamma=a.gamma, coef0=a.coef0, degree=a.degree, depth=a.depth, sigma=a.sigma,
                               device=dev)
    else:
        op = RadialKernelOperator(H.RBF_GAUSSIAN if gaussian else H.RBF_EXPONENTIAL, a.ell, a.dim, a.sigma, dev)
    fk = FusedKernelTrainer(op, L=a.L, m=a.m, hidden=(128, 128), batch_size=a.B, sequential=True, lr=a.lr,
                            rmsprop_decay=0.999, rmsprop_eps=1e-10, num_iters=a.steps, fourier_scale=a.fourier_scale,
                            seed=a.seed, index_seed=a.seed + 1)
    for _ in range(10):  # code objects, allocator
        fk.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps - 10):
        loss = fk.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    x_eval = op.sample(a.n_eval, torch.Generator(device=dev).manual_seed(a.seed + 1000))
    chunk = 4096
    ws = H.model_workspace(fk.shape, chunk, dev)

    def learned(xe):
        if xe.shape[0] != chunk:
            return H.model_forward(fk.shape, fk._params, xe.contiguous(), fk.c, H.model_workspace(fk.shape, xe.shape[0], dev))
        return H.model_forward(fk.shape, fk._params, xe.contiguous(), fk.c, ws)

    got = kernel_spectrum(op, learned, x_eval, chunk)
    params = dict(gamma=a.gamma, coef0=a.coef0, degree=a.degree) if a.kind == "polynomial" else \
        dict(gamma=a.gamma, coef0=a.coef0, depth=a.depth) if relu else {} if dot else dict(ell=a.ell)
    rec = dict(kind=a.kind, dim=a.dim, sigma=a.sigma, **params, L=a.L, B=a.B, steps=a.steps, lr=a.lr,
               fourier_scale=a.fourier_scale, seconds=round(dt, 2), steps_per_s=round((a.steps - 10) / dt, 1),
               loss=[float(v) for v in loss.cpu()], rayleigh_learned=[float(v) for v in got["eigvals"]],
               n_eval=a.n_eval, device=torch.cuda.get_device_name(0))
    print(f"steps/s {rec['steps_per_s']}")
    columns = [("learned", got["eigvals"])]
    if gaussian:  # the closed form exists for the Gaussian kind only
        lam = gaussian_kernel_eigvals(a.sigma, a.ell, a.dim, a.L)
        exact = kernel_spectrum(op, lambda xe: gaussian_kernel_eigenfunctions(xe, a.sigma, a.ell, a.L), x_eval, chunk)
        rel = np.abs(got["eigvals"] - lam) / lam
        gap = np.abs(exact["eigvals"] - lam) / lam
        rec.update(eig_closed_form=[float(v) for v in lam], rel_err=[float(v) for v in rel],
                   rel_err_mean=float(rel.mean()), rel_err_max=float(rel.max()),
                   sampling_gap_of_the_analytic_eigenfunctions=[float(v) for v in gap])
        columns.append(("closed form", lam))
        print("relative error of the Rayleigh quotients: " + " ".join(f"{v:.2e}" for v in rel))
    if a.spin:
        from neural_svd_amd.spin import SpinKernelTrainer
        sp = SpinKernelTrainer(op, L=a.L, m=a.m, hidden=(128, 128), batch_size=a.B, decay=a.spin_decay,
                               lr=a.lr if a.spin_lr is None else a.spin_lr, rmsprop_decay=0.999, rmsprop_eps=1e-10,
                               num_iters=a.steps, fourier_scale=a.fourier_scale, seed=a.seed, index_seed=a.seed + 1)
        for _ in range(10):
            sp.step()
        sp.check()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps - 10):
            sp.step()
        torch.cuda.synchronize()
        dts = time.perf_counter() - t0
        sp.check()
        # Rayleigh quotients of the orthonormalised functions chol^-1 model(x), as for the other columns
        sp_vals = kernel_spectrum(op, sp.forward, x_eval, chunk)["eigvals"]
        rec.update(spin_decay=a.spin_decay, spin_steps_per_s=round((a.steps - 10) / dts, 1),
                   spin_rayleigh=[float(v) for v in sp_vals], spin_loss=float(sp.loss[0]),
                   spin_eigvals_running=[float(v) for v in sp.loss[1:].cpu()])
        if gaussian:
            rec.update(spin_rel_err=[float(v) for v in np.abs(sp_vals - lam) / lam])
        print(f"SpIN steps/s {rec['spin_steps_per_s']}")
        columns.append(("SpIN", sp_vals))
    if a.spinx:
        from neural_svd_amd.spinx import SpinxKernelTrainer
        sx = SpinxKernelTrainer(op, L=a.L, m=a.m, hidden=(128, 128), batch_size=a.B, decay=a.spinx_decay,
                                lr=a.lr if a.spinx_lr is None else a.spinx_lr, rmsprop_decay=0.999, rmsprop_eps=1e-10,
                                num_iters=a.steps, fourier_scale=a.fourier_scale, seed=a.seed, index_seed=a.seed + 1,
                                trace_weights=[-1.0] * a.L)  # the loss is minimised: -1 = the reference's negated operator

        def sx_steps(first, last):
            for t in range(first, last):
                if a.spinx_weight_freq > 0 and t > 0 and t % a.spinx_weight_freq == 0:
                    sx.update_weights()
                sx.step()

        sx_steps(0, 10)
        sx.check()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sx_steps(10, a.steps)
        torch.cuda.synchronize()
        dtx = time.perf_counter() - t0
        sx.check()
        sx_vals = kernel_spectrum(op, sx.forward, x_eval, chunk)["eigvals"]
        out64 = sx.loss.cpu()
        rec.update(spinx_decay=a.spinx_decay, spinx_lr=a.lr if a.spinx_lr is None else a.spinx_lr,
                   spinx_weight_freq=a.spinx_weight_freq, spinx_steps_per_s=round((a.steps - 10) / dtx, 1),
                   spinx_rayleigh=[float(v) for v in sx_vals], spinx_loss=float(out64[0]),
                   spinx_losses=[float(v) for v in out64[1:a.L + 2]],
                   spinx_eigvals_batch=[float(v) for v in out64[a.L + 2:]],
                   spinx_weights=[float(v) for v in sx.weights.cpu()])
        if gaussian:
            # (with equal trace weights nothing orders the L functions: each converges to an eigenfunction, in any
            # order - the sorted quotients are the ones to hold against the spectrum)
            rec.update(spinx_rel_err=[float(v) for v in np.abs(sx_vals - lam) / lam],
                       spinx_rel_err_sorted=[float(v) for v in np.abs(np.sort(sx_vals)[::-1] - lam) / lam])
            print("SpINx, sorted quotients, relative error: " + " ".join(f"{v:.2e}" for v in rec["spinx_rel_err_sorted"]))
        print(f"SpINx steps/s {rec['spinx_steps_per_s']}")
        columns.append(("SpINx", sx_vals))
    if a.neuralef:
        from neural_svd_amd.neuralef import NefKernelTrainer
        nef_lr = a.lr if a.neuralef_lr is None else a.neuralef_lr
        nf = NefKernelTrainer(op, L=a.L, m=a.m, hidden=(128, 128), batch_size=a.B, unbiased=a.neuralef_unbiased,
                              lr=nef_lr, rmsprop_decay=0.999, rmsprop_eps=1e-10, num_iters=a.steps,
                              fourier_scale=a.fourier_scale, seed=a.seed, index_seed=a.seed + 1)
        for _ in range(10):
            nf.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps - 10):
            nf.step()
        torch.cuda.synchronize()
        dtn = time.perf_counter() - t0
        # Rayleigh quotients of the evaluation-mode functions model(x) / norm_biased, as for the other columns
        nf_vals = kernel_spectrum(op, nf.forward, x_eval, chunk)["eigvals"]
        rec.update(neuralef_unbiased=bool(a.neuralef_unbiased), neuralef_lr=nef_lr,
                   neuralef_steps_per_s=round((a.steps - 10) / dtn, 1), neuralef_rayleigh=[float(v) for v in nf_vals],
                   neuralef_loss=float(nf.loss[0]), neuralef_norm_biased=[float(v) for v in nf.norm_biased.cpu()])
        if gaussian:
            rec.update(neuralef_rel_err=[float(v) for v in np.abs(nf_vals - lam) / lam],
                       neuralef_rel_err_sorted=[float(v) for v in np.abs(np.sort(nf_vals)[::-1] - lam) / lam])
            print("NeuralEF, sorted quotients, relative error: " +
                  " ".join(f"{v:.2e}" for v in rec["neuralef_rel_err_sorted"]))
        print(f"NeuralEF steps/s {rec['neuralef_steps_per_s']}")
        columns.append(("NeuralEF", np.sort(nf_vals)[::-1]))
    if a.nystrom:
        from neural_svd_amd import Nystrom
        ny = Nystrom(op, op.sample(a.nystrom, torch.Generator(device=dev).manual_seed(a.seed + 2000)), a.L)
        ny_vals = ny.eigvals.double().cpu().numpy()
        rec.update(nystrom_n=a.nystrom, nystrom_eigvals=[float(v) for v in ny_vals], nystrom_iterations=ny.iterations,
                   nystrom_converged=bool(ny.converged), nystrom_seconds=round(ny.training_time, 4),
                   rel_to_nystrom=[float(v) for v in np.abs(got["eigvals"] - ny_vals) / ny_vals])
        columns.append((f"Nystrom n={a.nystrom}", ny_vals))
    print("  k  " + "  ".join(f"{name:>16}" for name, _ in columns))
    for k in range(a.L):
        print(f"{k:3d}  " + "  ".join(f"{float(v[k]):16.8e}" for _, v in columns))
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
