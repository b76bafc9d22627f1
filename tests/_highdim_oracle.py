"""Float64 restatement of the problems above four input dimensions and of the many-electron potential (reference
examples/operator/pde/schrodinger/potentials.py:35-57, problems.py:62-90, 106-111), composed around
tests/_periodic_oracle.py, tests/_box_oracle.py and oracle.nsvd_oracle by import. The tests hold it to the reference's
own float64 run (tests/golden/highdim.npz) on the CPU, and the HIP kernels to it on the GPU."""
from __future__ import annotations

import dataclasses
from typing import Tuple

import numpy as np
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _periodic_oracle as PO

POT_MOLECULE = 7
POT_COSINE, POT_SIN_OF_COS, POT_H2_ION = PO.POT_COSINE, PO.POT_SIN_OF_COS, PO.POT_H2_ION
OP_SCHROEDINGER, OP_FOKKER_PLANCK = PO.OP_SCHROEDINGER, PO.OP_FOKKER_PLANCK
IMP_NONE, IMP_GAUSSIAN, IMP_UNIFORM = PO.IMP_NONE, PO.IMP_GAUSSIAN, PO.IMP_UNIFORM
ANGSTROM = 1 / 0.52917721092

# public data (bond lengths in angstrom); coordinates become float32 bohr values as torch.as_tensor makes them
SYSTEMS = {
    "H2": ([[0.0, 0.0, 0.0], [0.742, 0.0, 0.0]], [1, 1], 0),
    "He": ([[0.0, 0.0, 0.0]], [2], 0),
    "LiH": ([[0.0, 0.0, 0.0], [1.595, 0.0, 0.0]], [3, 1], 0),
    "Be": ([[0.0, 0.0, 0.0]], [4], 0),
    "B": ([[0.0, 0.0, 0.0]], [5], 0),
}


@dataclasses.dataclass
class Problem(PO.Problem):
    """PO.Problem + the particles sharing the coordinates and the molecule: nuclei rows (R_0, .., R_{d-1}, Z) as float32
    values, pot_const the nuclear repulsion energy (a float32 value, as the reference's float32 tensors give it)"""
    n_particles: int = 1
    nuclei: Tuple[Tuple[float, ...], ...] = ()
    pot_const: float = 0.0


def molecule_tables(name, ndim):
    """-> (coords (n, ndim) float32, charges (n,) float32, total charge) the way the reference's Molecule builds them"""
    coords, charges, charge = SYSTEMS[name]
    c = (ANGSTROM * torch.as_tensor(coords))[:, :ndim].contiguous()
    return c, 1.0 * torch.as_tensor(charges), charge


def nuclear_energy(coords, charges):
    """sum_{a<b} Z_a Z_b / |R_a - R_b| in the dtype of the tables (float32 in the reference)"""
    coul = charges[:, None] * charges / (coords[:, None] - coords).norm(dim=-1)
    return coul.triu(1).sum()


def molecule_potential(x, prob: Problem):
    """V(x), (B, 1): pot_const - sum_i sum_a Z_a / |r_i - R_a| + sum_{i<j} 1 / |r_i - r_j|"""
    B = x.shape[0]
    rs = x.reshape(B, prob.n_particles, -1)
    tab = torch.tensor(prob.nuclei, dtype=x.dtype)
    R, Z = tab[:, :-1], tab[:, -1]
    V = torch.full((B,), float(prob.pot_const), dtype=x.dtype)
    V = V - (Z / (rs[:, :, None] - R).norm(dim=-1)).sum(dim=(-1, -2))
    for i in range(prob.n_particles):
        for j in range(i + 1, prob.n_particles):
            V = V + 1.0 / (rs[:, i] - rs[:, j]).norm(dim=-1)
    return V.view(-1, 1)


def potential(x, prob: Problem):
    if prob.potential == POT_MOLECULE:
        return molecule_potential(x, prob)
    return PO.potential(x, prob)


def operator_forward(x, p: O.Params, prob: Problem) -> O.OperatorCache:
    """PO.operator_forward; the molecule as BO.operator_forward with V = 0 plus the term -op_scale V f it leaves out.
    (Gaussian density: over all D coordinates; uniform: the cases here have one particle, D = ndim.)"""
    if prob.potential == POT_MOLECULE:
        assert prob.operator_kind == OP_SCHROEDINGER
        c = BO.operator_forward(x, p, dataclasses.replace(prob, potential=BO.POT_ZERO))
        return dataclasses.replace(c, Tf=c.Tf - prob.op_scale * molecule_potential(x, prob) * c.f)
    assert prob.n_particles == 1
    return PO.operator_forward(x, p, prob)


def loss_and_grads(x, p: O.Params, prob: Problem, v, M):
    c = operator_forward(x, p, prob)
    v, M = v.to(x.dtype), M.to(x.dtype)
    loss, lam1, lam2, _, _ = O.evd_loss_forward(c.f, c.Tf, v, M)
    df = O.evd_loss_backward(c.f, c.Tf, v, M, lam1, lam2)
    return dict(loss=loss, f=c.f, Tf=c.Tf, df=df, grads=O.operator_backward(c, p, prob, df), cache=c)


def distances(x, prob: Problem):
    """per row: the smallest electron-nucleus and electron-electron distance (inf without a second electron)"""
    B = x.shape[0]
    rs = x.double().reshape(B, prob.n_particles, -1)
    R = torch.tensor(prob.nuclei, dtype=torch.float64)[:, :-1]
    en = (rs[:, :, None] - R).norm(dim=-1).reshape(B, -1).min(dim=1).values
    ee = torch.full((B,), float("inf"), dtype=torch.float64)
    for i in range(prob.n_particles):
        for j in range(i + 1, prob.n_particles):
            ee = torch.minimum(ee, (rs[:, i] - rs[:, j]).norm(dim=-1))
    return en, ee


def row_groups(x, prob: Problem, within=0.1):
    """the groups check_rows-style comparisons measure separately: rows with an electron within `within` of a nucleus,
    rows with two electrons within `within` of each other, and the rest"""
    if prob.potential != POT_MOLECULE:
        return (("all", torch.ones(x.shape[0], dtype=torch.bool)),)
    en, ee = distances(x, prob)
    near, coal = en < within, (ee < within) & ~(en < within)
    return (("nucleus", near), ("coalescence", coal), ("other", ~(near | coal)))


COSINE_CS = dict(PO.COSINE_CS)
COSINE_CS[5] = (0.162944737278636, 0.181158387415124, 0.025397363258701, 0.182675171227804, 0.126471849245082)
COSINE_CS[10] = COSINE_CS[5] + (0.019508080999882, 0.055699643773410, 0.109376303840997, 0.191501367086860,
                                0.192977707039855)
FP_CS = dict(PO.FP_CS)
FP_CS[5] = (1.0, 0.8, 0.6, 0.4, 0.2)
FP_CS[10] = (0.1, 0.3, 0.2, 0.5, 0.2, 0.1, 0.3, 0.4, 0.2, 0.2)
COSINE_FIRST_EIGVAL = {5: 0.054018930536326, 10: 0.098087448866409}


def problem_of(cfg) -> Problem:
    """the fixture's recorded argument set -> Problem"""
    common = dict(eps=cfg["laplacian_eps"], op_scale=cfg["operator_scale"], op_shift=cfg["operator_shift"],
                  sigma=cfg["sampling_scale"], hard_mul_const=cfg["hard_mul_const"],
                  importance=IMP_UNIFORM if cfg["sampling_mode"] == "uniform" else IMP_GAUSSIAN)
    if cfg["problem"] == "fp":
        return Problem(potential=POT_SIN_OF_COS, operator_kind=OP_FOKKER_PLANCK, fp_scale=cfg["scale_operator"],
                       pot_coef=FP_CS[cfg["ndim"]], **common)
    if cfg["potential_type"] == "cosine":
        return Problem(potential=POT_COSINE, pot_coef=COSINE_CS[cfg["ndim"]], **common)
    assert cfg["potential_type"] == "quantum_chemistry"
    coords, charges, charge = molecule_tables(cfg["mol_name"], cfg["ndim"])
    nuclei = tuple(tuple(float(v) for v in row) + (float(z),) for row, z in zip(coords, charges))
    return Problem(potential=POT_MOLECULE, scale_kinetic=0.5, n_particles=int(charges.sum().item()) - charge,
                   nuclei=nuclei, pot_const=float(nuclear_energy(coords, charges)), **common)


def f32(a):
    return np.asarray(a, dtype=np.float32)
