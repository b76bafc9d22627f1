#!/usr/bin/env python3
"""Generate tests/golden/box.npz by IMPORTING the reference: bounded-domain problems - the Dirichlet box mask
(examples/operator/pde/boundary.py:16-36), the uniform sampler / density (main_pde.py:113-118), V = 0
(schrodinger/potentials.py:20-21) and InfiniteWell2D's spectrum (schrodinger/ground_truths.py:40-58).

Runs only where the reference checkout that make_golden.py imports is present; the test-suite never runs it, it only
reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_box.py

Per case, float64 (truth) and float32 (values only): NSTEPS training steps of the reference's own loop body
(compute_loss_operator, backward, RMSprop, cosine schedule) recording x, f, Tf, the loss, every parameter gradient and
the parameters after the last step; then compute_spectrum_evd(normalize=True) on a small grid and get_problem's ground
truth. Rows 0-5 of every x are PLANTED on and around the wall (finite-difference cases) or just inside / outside it
(exact cases: a row exactly on the wall is undefined there - autograd splits the tie of the clamp). No reference source
text is stored: fixtures are arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)

from methods.general import get_evd_method  # noqa: E402
from methods.spectrum import compute_spectrum_evd  # noqa: E402
from examples import OperatorWrapper  # noqa: E402
from examples.operator.pde.problems import get_problem  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402
from examples.operator.pde.main_pde import get_dataloader  # noqa: E402
from examples.operator.pde.schrodinger import NegativeHamiltonian  # noqa: E402
from examples.operator.pde.schrodinger.potentials import infinite_well_potential  # noqa: E402
from examples.utils import get_optimizer  # noqa: E402

NSTEPS = 3
BASE = dict(mlp_hidden_dims="16,16", fourier_mapping_size=8, batch_size=24, fourier_scale=0.1, lim=5.0, val_eps=0.5,
            apply_boundary=1, operator_scale=1.0, operator_shift=0.0)
WELL = dict(BASE, potential_type="infinite_well", sampling_mode="uniform", sampling_scale=5.0, apply_exp_mask=0)
CASES = dict(
    iw_sqrt=dict(WELL, neigs=4, boundary_mode="dir_box_sqrt", laplacian_eps=0.01),
    iw_exp=dict(WELL, neigs=5, boundary_mode="dir_box_exp", laplacian_eps=0.1),
    box_expmask=dict(BASE, neigs=4, boundary_mode="dir_box_exp", laplacian_eps=0.01,
                     potential_type="harmonic_oscillator", operator_shift=16.0, sampling_mode="gaussian",
                     sampling_scale=4.0, apply_exp_mask=1, exp_mask_init_scale=10.0),
    iw_exact_sqrt=dict(WELL, neigs=4, boundary_mode="dir_box_sqrt", laplacian_eps=0.0),
    iw_exact_exp=dict(WELL, neigs=5, boundary_mode="dir_box_exp", laplacian_eps=0.0),
    # get_problem asserts ndim == 2 for the well: these two are built from the classes
    iw_1d=dict(WELL, neigs=4, boundary_mode="dir_box_sqrt", laplacian_eps=0.01, ndim=1),
    iw_3d_exact=dict(WELL, neigs=4, boundary_mode="dir_box_exp", laplacian_eps=0.0, ndim=3),
)


def draw_x(args):
    """the sampler's batch (main_pde.py:92-93 / :114-115), float32, then the planted rows"""
    shape = (args.batch_size, args.n_particles, args.ndim)
    if args.sampling_mode == "uniform":
        x = args.sampling_scale * (2 * torch.rand(shape) - 1)
    else:
        x = args.sampling_scale * torch.randn(shape)
    x = x.reshape(args.batch_size, -1).clone()
    lim, eps, D = np.float32(args.lim), np.float32(args.laplacian_eps), args.ndim
    last = D - 1
    # (the coordinates a planted row keeps lie inside the box: the Gaussian sampler's need not)
    x[:5] = torch.clamp(x[:5], min=-0.8 * float(lim), max=0.8 * float(lim))
    if args.laplacian_eps > 0:
        x[0, 0] = float(lim - eps / 2)                 # the outer neighbour is beyond the right wall
        x[1, last] = float(-lim + eps / 2)             # ... beyond the left wall
        x[2, 0] = float(lim)                           # exactly on the wall
        x[3, last] = float(lim + eps / 2)              # outside: only the inner neighbour is inside
        x[4, :] = float(lim - eps / 2)                 # a corner, within eps of the wall in every coordinate
        x[4, last] = float(-lim + eps / 3)
        x[5, :] = float(2 * lim)                       # far outside
        x[5, 0] = float(-1.7 * lim)
    else:
        x[0, 0] = float(lim - np.float32(1e-3))        # just inside
        x[1, last] = float(1.5 * lim)                  # outside
    return x


def importance_for(args, dtype):
    if args.sampling_mode == "uniform":  # main_pde.py:116-118 (a float32 value there), rebuilt in `dtype`
        p = 1 / (2 * args.sampling_scale) ** args.ndim
        return lambda x: (p * torch.ones(x.shape[0], 1)).to(dtype)
    return G.importance_for(args, dtype)


def build(args):
    torch.manual_seed(args.seed)
    gt = None
    if args.ndim == 2:
        operator, gt = get_problem(args, torch.device("cpu"))
    else:
        args.n_particles = 1
        ham = NegativeHamiltonian(local_potential_ftn=infinite_well_potential, scale_kinetic=1.,
                                  laplacian_eps=args.laplacian_eps, n_particles=1)
        operator = OperatorWrapper(ham, scale=args.operator_scale, shift=args.operator_shift)
    model = get_wavefunctions(args)
    _, val_data, _, _, imp_val = get_dataloader(args, torch.device("cpu"))
    return operator, gt, get_evd_method(args, "neuralsvd", model), val_data, imp_val


def run_case(out, name, case):
    args0 = G.make_args(**case)
    torch.manual_seed(args0.seed + 1000)
    xs = [draw_x(args0) for _ in range(NSTEPS)]
    out[f"{name}_x"] = np.stack([x.numpy() for x in xs])
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        args = G.make_args(**case)
        operator, gt, method, val_data, imp_val = build(args)
        p = f"{name}_{tag}_"
        store = G.np64 if tag == "f64" else (lambda t: t.detach().cpu().float().numpy().copy())
        if tag == "f64":
            sd = method.state_dict()
            out[f"{name}_sd_keys"] = np.array(list(sd.keys()))
            out[f"{name}_sd_shapes"] = np.array([repr(tuple(v.shape)) for v in sd.values()])
            out[f"{name}_param_names"] = np.array([n for n, t in method.named_parameters() if t.requires_grad])
            for n, t in method.named_parameters():
                if t.requires_grad:
                    out[f"{name}_param0_{n}"] = t.detach().float().numpy()
                elif n.endswith("feature_map._B"):
                    out[f"{name}_fourier_B"] = t.detach().float().numpy()
            if gt is not None:
                out[f"{name}_gt"] = np.asarray(gt, dtype=np.float64)
            out[f"{name}_cfg"] = np.array(repr({k: v for k, v in vars(args).items() if k != "loss"}))
        method = method.to(dtype)
        imp_train = importance_for(args, dtype)
        optimizer = get_optimizer(args, method)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, args.num_iters)
        for it in range(NSTEPS):
            method.train()
            optimizer.zero_grad()
            x = xs[it].to(dtype)
            loss, aux = method.compute_loss_operator(operator, x, importance=imp_train)
            loss.backward()
            out[p + f"step{it}_loss"] = G.np64(loss)
            out[p + f"step{it}_f"] = store(aux["f"])
            out[p + f"step{it}_Tf"] = store(aux["Tf"])
            optimizer.step()
            scheduler.step()
            if tag == "f64":
                for n, t in method.named_parameters():
                    if t.requires_grad:
                        out[p + f"step{it}_grad_{n}"] = G.np64(t.grad)
                        if it == NSTEPS - 1:
                            out[p + f"step{it}_param_{n}"] = G.np64(t)
        if val_data is None:
            continue
        method.eval()
        # (exact mode differentiates through x: no torch.no_grad there, like examples/operator/__init__.py's evaluation)
        vd = val_data.to(dtype)
        bs = args.batch_size

        def loader():
            for i in range(int(np.ceil(len(vd) / float(bs)))):
                yield vd[i * bs:min((i + 1) * bs, len(vd))], 0.

        with torch.set_grad_enabled(args.laplacian_eps <= 0):
            res = compute_spectrum_evd(method, dataloader=loader(), operator=operator, importance_train=imp_train,
                                       importance_val=lambda z: imp_val(z).to(dtype), normalize=True,
                                       set_first_mode_const=False, device=torch.device("cpu"))
        out[p + "spec_eigvals"] = np.asarray(res["eigvals"], dtype=np.float64)
        out[p + "spec_norms"] = np.asarray(res["norms"], dtype=np.float64)
        if tag == "f64":
            out[f"{name}_val_data"] = val_data.numpy()


def main():
    out = {}
    for name, case in CASES.items():
        run_case(out, name, case)
    path = os.path.join(HERE, "box.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
