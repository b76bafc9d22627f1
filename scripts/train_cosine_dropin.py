"""The 2-D cosine Schroedinger problem (Han, Lu and Zhou 2020: V = sum_d cs[d] cos x_d on the periodic box [-pi, pi]^2)
through the REFERENCE API end to end: get_problem / get_wavefunctions / get_evd_method / get_dataloader /
train_operator -> FusedTrainer. Deterministic integer-harmonic Fourier features (--fourier_deterministic 1
--fourier_scale 1), uniform sampler with --sampling_scale pi, --lim pi, no boundary mask; --operator-shift 10 makes all
25 tabulated eigenvalues of -H + shift positive (with shift 0 the low-rank objective's optimum for the negative ones
is f = 0: README, infinite-well run). Evaluation by compute_spectrum_evd under the EMA weights inside train_operator;
mean and worst relative error of its last evaluation against the reference's table (problems.py:49-61).

    python scripts/train_cosine_dropin.py --steps 50000 --out profiles/cosine_train.json
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
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    dev = "cuda:0"
    pi = float(np.pi)
    a = argparse.Namespace(
        problem="sch", potential_type="cosine", charge=1.0, ndim=2, n_particles=1, neigs=o.neigs, laplacian_eps=0.01,
        operator_scale=1.0, operator_shift=o.operator_shift, sampling_mode="uniform", sampling_scale=pi,
        batch_size=o.batch_size, lim=pi, val_eps=pi / 100.0, use_fourier_feature=True,
        fourier_mapping_size=o.fourier_mapping_size, fourier_scale=1.0, fourier_deterministic=True,
        fourier_append_raw=False, mlp_hidden_dims="128,128,128", parallel=1, nonlinearity="softplus", apply_exp_mask=0,
        exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0, boundary_mode="dir_box_sqrt", sort=0,
        optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0, adam_eps=1e-7, num_iters=o.steps,
        ema_decay=0.995, use_lr_scheduler=True, print_freq=10 ** 9, eval_freq=o.eval_freq or o.steps, log_dir=None,
        fused_loop=not o.plain_loop)
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
    ev = np.asarray(eigs[-1], dtype=np.float64)
    gt = np.asarray(gt, dtype=np.float64)[:a.neigs]
    rel = np.abs(ev - gt) / np.abs(gt)
    energy = np.abs((ev - o.operator_shift) - (gt - o.operator_shift)) / np.abs(gt - o.operator_shift)
    rec = dict(api="drop_in.train_operator (fused loop body)" if a.fused_loop else "drop_in.train_operator (plain loop body)",
               problem="cosine", operator_shift=o.operator_shift, neigs=a.neigs, batch_size=a.batch_size,
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
