#!/usr/bin/env python3
"""Generate tests/golden/highdim.npz by IMPORTING the reference: the problems with more than four input dimensions -
the cosine Schroedinger problem at ndim 5 and the linear Fokker-Planck operator at ndim 10 (problems.py:62-69, 106-111)
- and the many-electron molecules of its quantum_chemistry branch (potentials.py:35-57, problems.py:79-90): H2 in 2-D
(D = 4) and in 3-D (D = 6), LiH in 3-D (D = 12).

Runs only where the reference checkout that make_golden.py imports is present; the test-suite never runs it, it only
reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_highdim.py

Per case, float64 only: 2 training steps of the reference's own loop body (compute_loss_operator, backward, RMSprop,
cosine schedule) recording x, f, Tf, the loss and every parameter gradient. All cases: neigs 4, batch 64, hidden
(16, 16), mapping size 8, laplacian_eps 0.01. The periodic cases use the uniform sampler on [-pi, pi]^D and the
integer-harmonic features, with rows 0-9 PLANTED on x_d in {0, pi/2, pi, -pi} as in make_golden_periodic.py. The
molecules use the Gaussian sampler and the exponential mask; the molecule handed to the reference's
local_potential_energy is a plain namespace of coords / charges tensors (its molecule.py reads a TOML table that the
stubbed `toml` of make_golden.py leaves empty), built the way its Molecule builds them: float32, angstrom to bohr by
1 / 0.52917721092. Their rows 0-3 have an electron 0.01 .. 0.04 from a nucleus, rows 4-7 two electrons 0.01 .. 0.04
apart; no distance of any row is below 1e-3. local_potential_energy itself is recorded on the 64 rows of step 0.
No reference source text is stored: arrays and reprs only.
"""
import os
import sys
import types
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)
import make_golden_box as GB  # noqa: E402

from methods.general import get_evd_method  # noqa: E402
from examples import OperatorWrapper  # noqa: E402
from examples.operator.pde.problems import get_problem  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402
from examples.operator.pde.schrodinger import NegativeHamiltonian  # noqa: E402
from examples.operator.pde.schrodinger.potentials import local_potential_energy, nuclear_energy  # noqa: E402
from examples.utils import get_optimizer  # noqa: E402

NSTEPS = 2
ANGSTROM = 1 / 0.52917721092
BASE = dict(mlp_hidden_dims="16,16", batch_size=64, neigs=4, val_eps=0.5, apply_boundary=0, operator_scale=1.0,
            operator_shift=0.0, laplacian_eps=0.01, fourier_mapping_size=8)
PERIODIC = dict(BASE, lim=float(np.pi), use_fourier_feature=True, fourier_deterministic=True, fourier_scale=1.0,
                sampling_mode="uniform", sampling_scale=float(np.pi), apply_exp_mask=0, use_gaussian_sampling=False,
                scale_operator=1.0)
MOLECULE = dict(BASE, problem="sch", potential_type="quantum_chemistry", fourier_scale=0.1, lim=5.0,
                sampling_mode="gaussian", sampling_scale=2.0, apply_exp_mask=1, exp_mask_init_scale=4.0)
# public data: bond lengths in angstrom
SYSTEMS = dict(H2=dict(coords=[[0.0, 0.0, 0.0], [0.742, 0.0, 0.0]], charges=[1, 1], charge=0),
               LiH=dict(coords=[[0.0, 0.0, 0.0], [1.595, 0.0, 0.0]], charges=[3, 1], charge=0))
CASES = dict(
    cos_5d=dict(PERIODIC, problem="sch", potential_type="cosine", operator_shift=10.0, ndim=5),
    fp_10d=dict(PERIODIC, problem="fp", operator_shift=1.0, scale_operator=0.5, ndim=10),
    h2_2d=dict(MOLECULE, mol_name="H2", ndim=2),
    h2_3d=dict(MOLECULE, mol_name="H2", ndim=3),
    lih_3d=dict(MOLECULE, mol_name="LiH", ndim=3),
)


def molecule_of(args):
    s = SYSTEMS[args.mol_name]
    mol = types.SimpleNamespace(coords=ANGSTROM * torch.as_tensor(s["coords"]),
                                charges=1.0 * torch.as_tensor(s["charges"]), charge=s["charge"])
    if args.ndim == 2:
        mol.coords = mol.coords[:, :2]
    return mol


def min_distances(x, mol, n_particles):
    """per row: the smallest electron-nucleus and the smallest electron-electron distance"""
    rs = x.double().reshape(x.shape[0], n_particles, -1)
    en = (rs[:, :, None] - mol.coords.double()).norm(dim=-1).reshape(x.shape[0], -1).min(dim=1).values
    i, j = np.triu_indices(n_particles, k=1)
    ee = (rs[:, :, None] - rs[:, None, :])[:, i, j].norm(dim=-1).min(dim=1).values
    return en, ee


def draw_x(args, mol):
    shape = (args.batch_size, args.n_particles, args.ndim)
    if args.sampling_mode == "uniform":
        x = args.sampling_scale * (2 * torch.rand(shape) - 1)
    else:
        x = args.sampling_scale * torch.randn(shape)
    if mol is None:
        x = x.reshape(args.batch_size, -1).clone()
        last = x.shape[1] - 1
        vals = [0.0, float(np.float32(np.pi / 2)), float(np.float32(np.pi)), float(-np.float32(np.pi))]
        for j, v in enumerate(vals):
            x[2 * j, 0] = v
            x[2 * j + 1, last] = v
        x[8, :] = vals[2]
        x[9, :] = vals[0]
        x[9, last] = vals[1]
        return x
    x = x.clone()
    nn_, npart = mol.coords.shape[0], args.n_particles
    for r in range(4):  # an electron 0.01 (r + 1) from a nucleus, off its axis
        x[r, r % npart] = mol.coords[r % nn_]
        x[r, r % npart, 1] += 0.01 * (r + 1)
    for r in range(4, 8):  # two electrons 0.01 (r - 3) apart
        i = r % npart
        j = (i + 1) % npart
        x[r, j] = x[r, i]
        x[r, j, 0] += 0.01 * (r - 3)
    x = x.reshape(args.batch_size, -1)
    en, ee = min_distances(x, mol, npart)
    assert float(en.min()) > 1e-3 and float(ee.min()) > 1e-3, (float(en.min()), float(ee.min()))
    assert int((en < 0.1).sum()) >= 4 and int((ee < 0.1).sum()) >= 4
    return x


def build(args):
    torch.manual_seed(args.seed)
    mol, gt = None, None
    if args.potential_type == "quantum_chemistry" and args.problem == "sch":
        mol = molecule_of(args)
        args.n_particles = int((mol.charges.sum() - mol.charge).type(torch.int).item())
        ham = NegativeHamiltonian(local_potential_ftn=partial(local_potential_energy, mol=mol), scale_kinetic=0.5,
                                  laplacian_eps=args.laplacian_eps, n_particles=args.n_particles)
        operator = OperatorWrapper(ham, scale=args.operator_scale, shift=args.operator_shift)
    else:
        operator, gt = get_problem(args, torch.device("cpu"))
    model = get_wavefunctions(args)
    return operator, gt, get_evd_method(args, "neuralsvd", model), mol


def run_case(out, name, case):
    dtype = torch.float64
    args = G.make_args(**case)
    operator, gt, method, mol = build(args)
    torch.manual_seed(args.seed + 3000)
    xs = [draw_x(args, mol) for _ in range(NSTEPS)]
    out[f"{name}_x"] = np.stack([x.numpy() for x in xs])
    assert out[f"{name}_x"].dtype == np.float32
    p = f"{name}_f64_"
    out[f"{name}_param_names"] = np.array([n for n, t in method.named_parameters() if t.requires_grad])
    for n, t in method.named_parameters():
        if t.requires_grad:
            out[f"{name}_param0_{n}"] = t.detach().float().numpy()
        elif n.endswith("feature_map._B"):
            out[f"{name}_fourier_B"] = t.detach().float().numpy()
    if gt is not None:
        out[f"{name}_gt"] = np.asarray(gt, dtype=np.float64)
    out[f"{name}_cfg"] = np.array(repr({k: v for k, v in vars(args).items() if k != "loss"}))
    if mol is not None:
        out[f"{name}_mol_coords"] = mol.coords.numpy()
        out[f"{name}_mol_charges"] = mol.charges.numpy()
        out[f"{name}_nuclear_energy"] = nuclear_energy(mol).numpy()
        rs = xs[0].to(dtype).reshape(args.batch_size, args.n_particles, -1)
        V = local_potential_energy(rs, mol)
        assert V.dtype == dtype and bool(torch.isfinite(V).all())
        out[f"{name}_V"] = G.np64(V)
    else:
        out[f"{name}_cs"] = np.asarray(operator.operator.local_potential_ftn.keywords["cs"], dtype=np.float64)
    method = method.to(dtype)
    imp_train = GB.importance_for(args, dtype)
    optimizer = get_optimizer(args, method)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, args.num_iters)
    for it in range(NSTEPS):
        method.train()
        optimizer.zero_grad()
        x = xs[it].to(dtype)
        loss, aux = method.compute_loss_operator(operator, x, importance=imp_train)
        loss.backward()
        assert bool(torch.isfinite(aux["f"]).all()) and bool(torch.isfinite(aux["Tf"]).all())
        out[p + f"step{it}_loss"] = G.np64(loss)
        out[p + f"step{it}_f"] = G.np64(aux["f"])
        out[p + f"step{it}_Tf"] = G.np64(aux["Tf"])
        optimizer.step()
        scheduler.step()
        for n, t in method.named_parameters():
            if t.requires_grad:
                out[p + f"step{it}_grad_{n}"] = G.np64(t.grad)


def main():
    out = {}
    for name, case in CASES.items():
        run_case(out, name, case)
    # get_problem's tables at the dimensions no case above runs
    for key, over in (("cos_10d", dict(CASES["cos_5d"], ndim=10)), ("fp_5d", dict(CASES["fp_10d"], ndim=5))):
        op, gt = get_problem(G.make_args(**over), torch.device("cpu"))
        out[f"{key}_gt"] = np.asarray(gt, dtype=np.float64)
        out[f"{key}_cs"] = np.asarray(op.operator.local_potential_ftn.keywords["cs"], dtype=np.float64)
    path = os.path.join(HERE, "highdim.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
