"""Float64 restatement of the problems whose potential is a function of the coordinates, not of |x| - the cosine
potential (reference examples/operator/pde/schrodinger/potentials.py:30-31), the hydrogen molecule ion (:11-17) - and of
the linear Fokker-Planck operator (examples/operator/pde/others.py:6-34), composed around tests/_box_oracle.py and
oracle.nsvd_oracle. The tests hold it to the reference's own float64 run (tests/golden/periodic.npz) on the CPU, and the
HIP kernels to it on the GPU."""
from __future__ import annotations

import dataclasses
import math
from typing import Tuple

import numpy as np
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO

POT_COSINE, POT_H2_ION, POT_SIN_OF_COS = 3, 4, 5
OP_SCHROEDINGER, OP_FOKKER_PLANCK = 0, 1
IMP_NONE, IMP_GAUSSIAN, IMP_UNIFORM = BO.IMP_NONE, BO.IMP_GAUSSIAN, BO.IMP_UNIFORM


@dataclasses.dataclass
class Problem(BO.Problem):
    """BO.Problem + the operator kind, the Fokker-Planck scale and the potential's coefficients (cs, or (R,) for H2+)"""
    operator_kind: int = OP_SCHROEDINGER
    fp_scale: float = 1.0
    pot_coef: Tuple[float, ...] = ()


def coefs(prob: Problem, dtype):
    """torch.tensor(cs) is float32 in the reference even in a float64 run: the float32 roundings of the literals"""
    return torch.tensor([float(np.float32(c)) for c in prob.pot_coef], dtype=dtype).view(1, -1)


def potential(x, prob: Problem):
    """V(x), (B, 1)"""
    if prob.potential == POT_COSINE:
        return (torch.cos(x) * coefs(prob, x.dtype)).sum(-1, keepdim=True)
    if prob.potential == POT_SIN_OF_COS:
        return torch.sin((torch.cos(x) * coefs(prob, x.dtype)).sum(-1, keepdim=True))
    if prob.potential == POT_H2_ION:
        e = torch.zeros(x.shape[1], dtype=x.dtype)
        e[-1] = 1.0
        R, q = prob.pot_coef[0], prob.charge_or_k
        return (-q / torch.linalg.norm(x - R * e, dim=1) - q / torch.linalg.norm(x + R * e, dim=1)).view(-1, 1)
    return BO.potential(x, prob)


def operator_forward(x, p: O.Params, prob: Problem) -> O.OperatorCache:
    """Tf, f of OperatorWrapper(NegativeHamiltonian or NegativeLinearFokkerPlanck)(model, x, importance).
    Schroedinger kind: BO.operator_forward with V = 0, then the potential term -op_scale V f it leaves out (Tf is
    linear in V). Fokker-Planck kind (others.py:16-30): the stencil on g = sqrt(p) f gives Lap g, grad g and g, all
    divided by the UNCLAMPED sqrt p(x); V = sin(sum cs cos x) goes through the same stencil;
    Tf = op_scale fp_scale (Lap f + grad V . grad f + f Lap V) + op_shift f."""
    if prob.operator_kind == OP_SCHROEDINGER:
        c = BO.operator_forward(x, p, dataclasses.replace(prob, potential=BO.POT_ZERO))
        return dataclasses.replace(c, Tf=c.Tf - prob.op_scale * potential(x, prob) * c.f)
    assert prob.eps > 0 and prob.box_mode == BO.BOX_NONE
    D = x.shape[1]
    pts = O.stencil_points(x, prob.eps)
    gs, vs = [], []
    for j, xe in enumerate(pts):
        if j == 0:
            u, (phi0, zs, base0, mask0) = BO.wave(xe, p, prob, keep=True)
        else:
            u = BO.wave(xe, p, prob)
        gs.append(BO.sqrt_importance(xe, prob) * u)
        vs.append(potential(xe, prob))
    lap, lap_v = -2 * D * gs[0], -2 * D * vs[0]
    adv = torch.zeros_like(gs[0])
    for i in range(D):
        gp, gm, vp, vm = gs[1 + 2 * i], gs[2 + 2 * i], vs[1 + 2 * i], vs[2 + 2 * i]
        lap = lap + (gp + gm)
        lap_v = lap_v + (vp + vm)
        adv = adv + ((vp - vm) / (2 * prob.eps)) * ((gp - gm) / (2 * prob.eps))
    sp0 = BO.sqrt_importance(x, prob)
    lap_f, adv, fs = lap / prob.eps ** 2 / sp0, adv / sp0, gs[0] / sp0
    Tf = prob.fp_scale * (lap_f + adv + fs * (lap_v / prob.eps ** 2))
    Tf = prob.op_scale * Tf + prob.op_shift * fs
    return O.OperatorCache(x, phi0, zs, base0, mask0, sp0, sp0, fs, Tf)


def operator_backward(c: O.OperatorCache, p: O.Params, prob: Problem, df):
    return O.operator_backward(c, p, prob, df)


def loss_and_grads(x, p: O.Params, prob: Problem, v, M):
    """O.loss_and_grads on this module's operator"""
    c = operator_forward(x, p, prob)
    v, M = v.to(x.dtype), M.to(x.dtype)
    loss, lam1, lam2, _, _ = O.evd_loss_forward(c.f, c.Tf, v, M)
    df = O.evd_loss_backward(c.f, c.Tf, v, M, lam1, lam2)
    return dict(loss=loss, f=c.f, Tf=c.Tf, df=df, grads=operator_backward(c, p, prob, df), cache=c)


def spectrum_evd(grid, p: O.Params, prob: Problem, lim):
    """BO.spectrum_evd on this module's operator"""
    D = grid.shape[1]
    sqrt_val = math.sqrt(float(np.float32(1.0 / (2 * lim) ** D)))  # (a float32 value in the reference: main_pde.py:130)
    c = operator_forward(grid, p, prob)
    w = BO.sqrt_importance(grid, prob) / sqrt_val
    phi = torch.nan_to_num(w * c.f)
    Tphi = torch.nan_to_num(w * c.Tf)
    Tphi[torch.all(torch.isclose(grid, torch.zeros_like(grid[0])), dim=1)] = 0.0
    n = grid.shape[0]
    cov, quad = phi.T @ phi / n, phi.T @ Tphi / n
    return dict(eigvals=torch.diag(quad) / torch.diag(cov), norms=torch.diag(cov), cov=cov, quad=quad)


def nucleus_rows(x, prob: Problem, within=0.1):
    """rows within `within` of a nucleus of the H2+ potential"""
    e = torch.zeros(x.shape[1], dtype=x.dtype)
    e[-1] = 1.0
    R = prob.pot_coef[0]
    return torch.minimum(torch.linalg.norm(x - R * e, dim=1), torch.linalg.norm(x + R * e, dim=1)) < within


def hydrogen3d_eigvals(neigs, charge=1.0):
    """-Z^2 / (4 n^2) with degeneracy n^2 over n < ceil(neigs^(1/3)) + 1, cut to neigs - SHORT when those shells hold
    fewer states (ground_truths.py, Hydrogen3D.get_eigvals)"""
    nmax = int(math.ceil(neigs ** (1.0 / 3))) + 1
    q = [n for n in range(1, nmax) for _ in range(n * n)][:neigs]
    return np.array([-charge ** 2 / (4.0 * n * n) for n in q], dtype=np.float64)


COSINE_CS = {1: (1.0,), 2: (0.814723686393179, 0.905791937075619)}
FP_CS = {1: (1.0,), 2: (1.0, 1.0)}


def problem_of(cfg) -> Problem:
    """the fixture's recorded argument set -> Problem"""
    common = dict(eps=cfg["laplacian_eps"], op_scale=cfg["operator_scale"], op_shift=cfg["operator_shift"],
                  sigma=cfg["sampling_scale"], hard_mul_const=cfg["hard_mul_const"],
                  importance=IMP_UNIFORM if cfg["sampling_mode"] == "uniform" else IMP_GAUSSIAN)
    if cfg["problem"] == "fp":
        return Problem(potential=POT_SIN_OF_COS, operator_kind=OP_FOKKER_PLANCK, fp_scale=cfg["scale_operator"],
                       pot_coef=FP_CS[cfg["ndim"]], **common)
    pt = cfg["potential_type"]
    if pt == "cosine":
        return Problem(potential=POT_COSINE, pot_coef=COSINE_CS[cfg["ndim"]], **common)
    if pt == "hydrogen_mol_ion":
        return Problem(potential=POT_H2_ION, charge_or_k=2 * cfg["charge"], pot_coef=(cfg["hydrogen_mol_ion_R"],),
                       **common)
    return Problem(potential=O.POT_HYDROGEN, charge_or_k=cfg["charge"], **common)
