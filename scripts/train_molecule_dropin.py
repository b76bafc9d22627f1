"""A small molecule's electronic Schroedinger problem (the reference's --potential_type quantum_chemistry: n electrons
of --ndim coordinates each in the Coulomb field of the nuclei, kinetic scale 1/2, atomic units) through the REFERENCE
API end to end: get_problem(args.high_dim_stencil) / get_wavefunctions / get_evd_method / get_dataloader /
train_operator -> FusedTrainer. Gaussian sampler and importance over all n * ndim coordinates, exponential mask,
n * ndim <= 12 (H2 and He in 3-D: 6, LiH and Be in 3-D: 12): the step runs on the generic kernels with the
direction-loop epilogue. There is no validation grid: the evaluation is compute_spectrum_evd on --val-points points
drawn uniformly from [-lim, lim]^(n ndim). The reference tabulates no spectrum for these problems; the record holds the
measured Rayleigh quotients (energies in hartree, spin and antisymmetry not imposed: the lowest states of the spatial
Hamiltonian).

    python scripts/train_molecule_dropin.py --mol-name H2 --ndim 3 --steps 20000
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
from neural_svd_amd.operators import UniformBoxImportance, get_dataloader, get_problem
from neural_svd_amd.spectrum import compute_spectrum_evd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mol-name", default="H2", help="H, He, Li, Be, H2+, H2, LiH (neural_svd_amd.operators.Molecule)")
    ap.add_argument("--ndim", type=int, default=3, choices=(2, 3))
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--neigs", type=int, default=4)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--hidden", default="128,128,128")
    ap.add_argument("--fourier-mapping-size", type=int, default=64)
    ap.add_argument("--sampling-scale", type=float, default=2.0)
    ap.add_argument("--lim", type=float, default=6.0)
    ap.add_argument("--operator-shift", type=float, default=0.0)
    ap.add_argument("--val-points", type=int, default=65536)
    ap.add_argument("--sequential", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--exact", action="store_true",
                    help="laplacian_eps 0: the exact Laplacian on the generic kernels' forward-mode jets "
                         "(args.generic_exact_laplacian -> PATH_GENERIC_EXACT) instead of the eps = 0.01 stencil")
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    dev = "cuda:0"
    a = argparse.Namespace(
        problem="sch", potential_type="quantum_chemistry", mol_name=o.mol_name, charge=1.0, ndim=o.ndim, n_particles=1,
        neigs=o.neigs, laplacian_eps=0.0 if o.exact else 0.01, operator_scale=1.0, operator_shift=o.operator_shift,
        sampling_mode="gaussian", sampling_scale=o.sampling_scale, batch_size=o.batch_size, lim=o.lim, val_eps=0.5,
        use_fourier_feature=True, fourier_mapping_size=o.fourier_mapping_size, fourier_scale=0.1,
        fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims=o.hidden, parallel=1,
        nonlinearity="softplus", apply_exp_mask=1, exp_mask_init_scale=4.0, hard_mul_const=1.0, apply_boundary=0,
        boundary_mode="dir_box_sqrt", sort=0, optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0,
        adam_eps=1e-7, num_iters=o.steps, ema_decay=0.995, use_lr_scheduler=True, print_freq=10 ** 9,
        eval_freq=10 ** 9, log_dir=None, fused_loop=True, high_dim_stencil=True, generic_exact_laplacian=o.exact)
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=o.sequential))
    torch.manual_seed(o.seed)
    operator, _ = get_problem(a, dev)
    D = a.n_particles * a.ndim
    model = get_wavefunctions(a)
    make_batch, val_data, batch_ftn_val, imp_train, imp_val = get_dataloader(a, dev)
    method = get_evd_method(a, "neuralsvd", model).to(dev)
    t0 = time.perf_counter()
    train_operator(a, method, operator, make_batch, val_data, batch_ftn_val, None, None, dev, imp_train, imp_val)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pts = o.lim * (2 * torch.rand((o.val_points, D), device=dev, generator=torch.Generator(dev).manual_seed(1)) - 1)
    method.eval()
    out = compute_spectrum_evd(method, dataloader=((pts[i:i + 8192], 0.0) for i in range(0, len(pts), 8192)),
                               operator=operator, importance_train=imp_train,
                               importance_val=UniformBoxImportance(o.lim, D), normalize=True, device=dev)
    ev = np.asarray(out["eigvals"], dtype=np.float64)
    rec = dict(api="drop_in.train_operator (fused loop body)", problem="quantum_chemistry", mol_name=o.mol_name,
               ndim=o.ndim, n_particles=a.n_particles, input_dimensions=D, neigs=o.neigs, batch_size=o.batch_size,
               hidden=o.hidden, steps=o.steps, steps_per_second=round(o.steps / dt, 1),
               nesting="sequential" if o.sequential else "joint", operator_shift=o.operator_shift,
               energies_hartree=[float(-(v - o.operator_shift)) for v in ev],
               norms=[float(v) for v in np.asarray(out["norms"], dtype=np.float64)], seed=o.seed)
    print(json.dumps(rec))
    if o.out:
        os.makedirs(os.path.dirname(o.out) or ".", exist_ok=True)
        json.dump(rec, open(o.out, "w"), indent=1)


if __name__ == "__main__":
    main()
