#!/usr/bin/env python3
"""Generate tests/golden/periodic.npz by IMPORTING the reference: the periodic benchmark pair - the cosine Schroedinger
problem (examples/operator/pde/schrodinger/potentials.py:30-31, problems.py:36-69) and the linear Fokker-Planck operator
(examples/operator/pde/others.py:6-34, problems.py:96-119) -, the hydrogen molecule ion (potentials.py:11-17) and 3-D
hydrogen (ground_truths.py, Hydrogen3D).

Runs only where the reference checkout that make_golden.py imports is present; the test-suite never runs it, it only
reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_periodic.py

Per case, float64 only: 3 (cos_2d, fp_2d) or 2 training steps of the reference's own loop body (compute_loss_operator,
backward, RMSprop, cosine schedule) recording x, f, Tf, the loss, every parameter gradient and (3-step cases) the parameters
after the last step; for cos_2d and fp_2d also compute_spectrum_evd(normalize=True) on a small grid; get_problem's ground truth where
it has one. The first rows of every x are PLANTED: for the periodic cases on x_d in {0, pi/2, pi, -pi} (float32
values), where sin or cos vanish; for H2+ 1e-3 and eps/2 away from each nucleus (never on one: V is infinite there).
get_problem's cosine and fp branches read args.use_gaussian_sampling and args.scale_operator, which main_pde.py's
parser does not define: the argument sets below carry them. No reference source text is stored: arrays and reprs only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)
import make_golden_box as GB  # noqa: E402

from methods.general import get_evd_method  # noqa: E402
from methods.spectrum import compute_spectrum_evd  # noqa: E402
from examples.operator.pde.problems import get_problem  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402
from examples.operator.pde.main_pde import get_dataloader  # noqa: E402
from examples.operator.pde.schrodinger.ground_truths import Hydrogen3D  # noqa: E402
from examples.utils import get_optimizer  # noqa: E402

NSTEPS = {"cos_2d": 3, "fp_2d": 3}  # (the optimiser trajectory is held on these two; the other cases record 2 steps)
BASE = dict(mlp_hidden_dims="16,16", batch_size=48, neigs=4, val_eps=0.5, apply_boundary=0, operator_scale=1.0,
            operator_shift=0.0, hydrogen_mol_ion_R=1.0)
PERIODIC = dict(BASE, lim=float(np.pi), use_fourier_feature=True, fourier_deterministic=True, fourier_scale=1.0,
                fourier_mapping_size=4, sampling_mode="uniform", sampling_scale=float(np.pi), apply_exp_mask=0,
                use_gaussian_sampling=False, scale_operator=1.0)
COS = dict(PERIODIC, problem="sch", potential_type="cosine", operator_shift=10.0)
FP = dict(PERIODIC, problem="fp", operator_shift=1.0, scale_operator=0.5)
COULOMB = dict(BASE, problem="sch", fourier_mapping_size=8, fourier_scale=0.1, lim=5.0, sampling_mode="gaussian",
               sampling_scale=2.0, apply_exp_mask=1, exp_mask_init_scale=4.0, charge=1.0)
CASES = dict(
    cos_2d=dict(COS, laplacian_eps=0.01),
    cos_1d=dict(COS, laplacian_eps=0.01, ndim=1),
    cos_2d_exact=dict(COS, laplacian_eps=0.0),
    fp_2d=dict(FP, laplacian_eps=0.01),
    fp_2d_eps01=dict(FP, laplacian_eps=0.1),
    fp_1d=dict(FP, laplacian_eps=0.01, ndim=1),
    fp_2d_expmask=dict(FP, laplacian_eps=0.01, apply_exp_mask=1, exp_mask_init_scale=4.0),
    h2p_2d=dict(COULOMB, potential_type="hydrogen_mol_ion", laplacian_eps=0.01),
    h2p_3d_exact=dict(COULOMB, potential_type="hydrogen_mol_ion", laplacian_eps=0.0, ndim=3),
    hyd_3d=dict(COULOMB, potential_type="hydrogen", laplacian_eps=0.01, ndim=3, neigs=6),
)
SPECTRUM = ("cos_2d", "fp_2d")


def draw_x(args):
    """the sampler's batch (main_pde.py:92-93 / :114-115), float32, then the planted rows"""
    shape = (args.batch_size, args.n_particles, args.ndim)
    if args.sampling_mode == "uniform":
        x = args.sampling_scale * (2 * torch.rand(shape) - 1)
    else:
        x = args.sampling_scale * torch.randn(shape)
    x = x.reshape(args.batch_size, -1).clone()
    last = args.ndim - 1
    if args.potential_type == "hydrogen_mol_ion":
        R = float(args.hydrogen_mol_ion_R)
        near = float(np.float32(args.laplacian_eps)) / 2 if args.laplacian_eps > 0 else 5e-3
        x[:4] = 0.0
        x[0, 0], x[0, last] = 1e-3, R           # 1e-3 beside the upper nucleus
        x[1, last] = -R + 1e-3                  # 1e-3 above the lower one, on the axis
        x[2, 0], x[2, last] = near, -R          # eps / 2 beside the lower one
        x[3, last] = R - near                   # eps / 2 below the upper one: the stencil straddles the nucleus
    elif args.potential_type == "cosine" or args.problem == "fp":
        vals = [0.0, float(np.float32(np.pi / 2)), float(np.float32(np.pi)), float(-np.float32(np.pi))]
        for j, v in enumerate(vals):
            x[2 * j, 0] = v
            x[2 * j + 1, last] = v
        x[8, :] = vals[2]                       # every coordinate on pi
        x[9, :] = vals[0]
        x[9, last] = vals[1]                    # (0, pi / 2)
    return x


def build(args):
    torch.manual_seed(args.seed)
    operator, gt = get_problem(args, torch.device("cpu"))
    model = get_wavefunctions(args)
    _, val_data, _, _, imp_val = get_dataloader(args, torch.device("cpu"))
    return operator, gt, get_evd_method(args, "neuralsvd", model), val_data, imp_val


def run_case(out, name, case):
    args0 = G.make_args(**case)
    torch.manual_seed(args0.seed + 2000)
    nsteps = NSTEPS.get(name, 2)
    xs = [draw_x(args0) for _ in range(nsteps)]
    out[f"{name}_x"] = np.stack([x.numpy() for x in xs])
    dtype = torch.float64
    args = G.make_args(**case)
    operator, gt, method, val_data, imp_val = build(args)
    p = f"{name}_f64_"
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
    imp_train = GB.importance_for(args, dtype)
    optimizer = get_optimizer(args, method)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, args.num_iters)
    for it in range(nsteps):
        method.train()
        optimizer.zero_grad()
        x = xs[it].to(dtype)
        loss, aux = method.compute_loss_operator(operator, x, importance=imp_train)
        loss.backward()
        out[p + f"step{it}_loss"] = G.np64(loss)
        out[p + f"step{it}_f"] = G.np64(aux["f"])
        out[p + f"step{it}_Tf"] = G.np64(aux["Tf"])
        optimizer.step()
        scheduler.step()
        for n, t in method.named_parameters():
            if t.requires_grad:
                out[p + f"step{it}_grad_{n}"] = G.np64(t.grad)
                if it == nsteps - 1 and name in NSTEPS:
                    out[p + f"step{it}_param_{n}"] = G.np64(t)
    if name not in SPECTRUM:
        return
    method.eval()
    vd = val_data.to(dtype)
    bs = args.batch_size

    def loader():
        for i in range(int(np.ceil(len(vd) / float(bs)))):
            yield vd[i * bs:min((i + 1) * bs, len(vd))], 0.

    with torch.no_grad():
        res = compute_spectrum_evd(method, dataloader=loader(), operator=operator, importance_train=imp_train,
                                   importance_val=lambda z: imp_val(z).to(dtype), normalize=True,
                                   set_first_mode_const=False, device=torch.device("cpu"))
    out[p + "spec_eigvals"] = np.asarray(res["eigvals"], dtype=np.float64)
    out[p + "spec_norms"] = np.asarray(res["norms"], dtype=np.float64)
    out[f"{name}_val_data"] = val_data.numpy()


def main():
    out = {}
    for name, case in CASES.items():
        run_case(out, name, case)
    # Hydrogen3D.get_eigvals: the list comes back short when its shells hold fewer than neigs states
    for n in (1, 5, 6, 14, 16, 30):
        out[f"hydrogen3d_eigvals_{n}"] = np.asarray(Hydrogen3D(charge=1.0).get_eigvals(n), dtype=np.float64)
    # the full ground-truth table of the 2-D cosine problem
    a = G.make_args(**dict(CASES["cos_2d"], neigs=25))
    out["cos_2d_gt25"] = np.asarray(get_problem(a, torch.device("cpu"))[1], dtype=np.float64)
    path = os.path.join(HERE, "periodic.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
