"""The 2-D cosine Schroedinger problem (Han, Lu and Zhou 2020: V = sum_d cs[d] cos x_d on the periodic box [-pi, pi]^2)
through the REFERENCE API end to end: get_problem / get_wavefunctions / get_evd_method / get_dataloader /
train_operator -> FusedTrainer. Deterministic integer-harmonic Fourier features (--fourier_deterministic 1
--fourier_scale 1), uniform sampler with --sampling_scale pi, --lim pi, no boundary mask; --operator-shift 10 makes all
25 tabulated eigenvalues of -H + shift positive (with shift 0 the low-rank objective's optimum for the negative ones
is f = 0: README, infinite-well run). Evaluation by compute_spectrum_evd under the EMA weights inside train_operator;
mean and worst relative error of its last evaluation against the reference's table (problems.py:49-61).

    python scripts/train_cosine_dropin.py --steps 50000 --out profiles/cosine_train.json

--ndim 5 | 10 (and --problem fp at any of 1, 2, 5, 10) run the pair at the dimensions Han, Lu and Zhou designed it for:
args.high_dim_stencil is set, the step runs on the generic kernels with the direction-loop epilogue, and - there is no
validation grid above two dimensions - the evaluation is compute_spectrum_evd on --val-points points drawn uniformly
from the box. The reference tabulates the first eigenvalue only (0 for Fokker-Planck): the record holds it beside the
measured one.

    python scripts/train_cosine_dropin.py --ndim 5 --neigs 4 --fourier-mapping-size 4 --steps 20000
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_svd_amd.drop_in import train_operator
from neural_svd_amd.models import get_wavefunctions
from neural_svd_amd.nested_lowrank import get_evd_method
from neural_svd_amd.operators import get_dataloader, get_problem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50000)
    ap.add_argument("--eval-freq", type=int, default=None, help="default: once, after the last step")
    ap.add_argument("--sequential", action="store_true")
    ap.add_argument("--plain-loop", action="store_true", help="torch autograd loop body instead of the fused one")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--neigs", type=int, default=25, help="the reference tabulates 25 eigenvalues")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--fourier-mapping-size", type=int, default=32, help="harmonics 1 .. n per coordinate")
    ap.add_argument("--operator-shift", type=float, default=10.0,
                    help="above the largest tabulated energy (8.05): every wanted eigenvalue of -H + shift is positive")
    ap.add_argument("--ndim", type=int, default=2, choices=(1, 2, 5, 10))
    ap.add_argument("--problem", default="sch", choices=("sch", "fp"), help="fp: the linear Fokker-Planck operator")
    ap.add_argument("--hidden", default="128,128,128")
    ap.add_argument("--val-points", type=int, default=65536, help="ndim > 2: points of the sampled evaluation")
    ap.add_argument("--exact", action="store_true",
                    help="laplacian_eps 0: the exact Laplacian on the generic kernels' forward-mode jets "
                         "(args.generic_exact_laplacian -> PATH_GENERIC_EXACT) instead of the eps = 0.01 stencil")
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    high = o.ndim > 2
    dev = "cuda:0"
    pi = float(np.pi)
    a = argparse.Namespace(
        problem=o.problem, potential_type="cosine", charge=1.0, ndim=o.ndim, n_particles=1, neigs=o.neigs,
        laplacian_eps=0.0 if o.exact else 0.01,
        operator_scale=1.0, operator_shift=o.operator_shift, sampling_mode="uniform", sampling_scale=pi,
        batch_size=o.batch_size, lim=pi, val_eps=pi / 100.0, use_fourier_feature=True,
        fourier_mapping_size=o.fourier_mapping_size, fourier_scale=1.0, fourier_deterministic=True,
        fourier_append_raw=False, mlp_hidden_dims=o.hidden, parallel=1, nonlinearity="softplus", apply_exp_mask=0,
        exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0, boundary_mode="dir_box_sqrt", sort=0,
        optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0, adam_eps=1e-7, num_iters=o.steps,
        ema_decay=0.995, use_lr_scheduler=True, print_freq=10 ** 9, eval_freq=o.eval_freq or o.steps, log_dir=None,
        fused_loop=not o.plain_loop, high_dim_stencil=high, generic_exact_laplacian=o.exact)
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=o.sequential))
    torch.manual_seed(o.seed)
    operator, gt = get_problem(a, dev)
    model = get_wavefunctions(a)
    make_batch, val_data, batch_ftn_val, imp_train, imp_val = get_dataloader(a, dev)
    method = get_evd_method(a, "neuralsvd", model).to(dev)
    t0 = time.perf_counter()
    eigs, norms = train_operator(a, method, operator, make_batch, val_data, batch_ftn_val, None, None, dev, imp_train,
                                 imp_val, ground_truth_spectrum=gt)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if not eigs:  # no grid above two dimensions: one evaluation on points drawn uniformly from the box
        from neural_svd_amd.operators import UniformBoxImportance
        from neural_svd_amd.spectrum import compute_spectrum_evd
        pts = pi * (2 * torch.rand((o.val_points, o.ndim), device=dev, generator=torch.Generator(dev).manual_seed(1)) - 1)
        method.eval()
        out = compute_spectrum_evd(method, dataloader=((pts[i:i + 8192], 0.0) for i in range(0, len(pts), 8192)),
                                   operator=operator, importance_train=imp_train,
                                   importance_val=UniformBoxImportance(pi, o.ndim), normalize=True, device=dev)
        eigs, norms = [out["eigvals"]], [out["norms"]]
    ev = np.asarray(eigs[-1], dtype=np.float64)
    gt = np.asarray(gt, dtype=np.float64)[:a.neigs]
    if high or o.problem == "fp":  # only the first eigenvalue is tabulated (0 for Fokker-Planck): compared alone
        ev_c, gt_c = ev[:1], gt[:1]
    else:
        ev_c, gt_c = ev, gt
    rel = np.abs(ev_c - gt_c) / np.abs(gt_c)
    with np.errstate(divide="ignore", invalid="ignore"):
        energy = np.abs(ev_c - gt_c) / np.abs(gt_c - o.operator_shift)
    rec = dict(api="drop_in.train_operator (fused loop body)" if a.fused_loop else "drop_in.train_operator (plain loop body)",
               problem="cosine" if o.problem == "sch" else "fokker_planck", ndim=o.ndim, hidden=o.hidden,
               first_eigenvalue=float(ev[0] - o.operator_shift), first_eigenvalue_tabulated=float(gt[0] - o.operator_shift),
               operator_shift=o.operator_shift, neigs=a.neigs, batch_size=a.batch_size,
               fourier_mapping_size=o.fourier_mapping_size,
               final_norms=[float(v) for v in np.asarray(norms[-1], dtype=np.float64)],
               nesting="sequential" if o.sequential else "joint", steps=o.steps,
               steps_per_second=round(o.steps / dt, 1), evaluations=len(eigs),
               wall_seconds_including_evaluations=round(dt, 1), eigvals=[float(v) for v in ev],
               ground_truth=[float(v) for v in gt], seed=o.seed, rel_err_mean=float(rel.mean()),
               rel_err_max=float(rel.max()), rel_err_mean_energies=float(energy.mean()),
               rel_err_max_energies=float(energy.max()))
    print(json.dumps(rec))
    if o.out:
        os.makedirs(os.path.dirname(o.out) or ".", exist_ok=True)
        json.dump(rec, open(o.out, "w"), indent=1)


if __name__ == "__main__":
    main()
