"""Float64 restatement of the bounded-domain problems - the Dirichlet box mask (reference examples/operator/pde/
boundary.py:16-36) alone or inside the exponential mask, the uniform sampling density (main_pde.py:113-118) and V = 0
(schrodinger/potentials.py:20-21) - composed around oracle.nsvd_oracle's pieces. The tests hold it to the reference's
own float64 run (tests/golden/box.npz) on the CPU, and the HIP kernels to it on the GPU."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from oracle import nsvd_oracle as O

POT_ZERO = 2
BOX_NONE, BOX_SQRT, BOX_EXP = 0, 1, 2
IMP_NONE, IMP_GAUSSIAN, IMP_UNIFORM = 0, 1, 2


@dataclasses.dataclass
class Problem(O.Problem):
    """O.Problem + which density `sigma` belongs to, and the model's box mask"""
    importance: int = IMP_GAUSSIAN
    box_mode: int = BOX_NONE
    box_lim: float = 0.0

    def __post_init__(self):
        self.use_importance = self.importance != IMP_NONE


def box_mask(x, prob: Problem):
    """M(x) = prod_d m(clamp(x_d, -lim, lim)), (B, 1); differentiable like the reference's (clamp, maximum)"""
    if prob.box_mode == BOX_NONE:
        return torch.ones(x.shape[0], 1, dtype=x.dtype)
    lim = prob.box_lim
    t = torch.clamp(x, min=-lim, max=lim)
    if prob.box_mode == BOX_SQRT:
        m = torch.clamp(((2 * lim ** 2 - t ** 2).sqrt() - lim) / lim, min=0.0)
    else:
        m = (1 - torch.exp(-(lim - t))) * (1 - torch.exp(-(t + lim)))
    return m.prod(dim=1, keepdim=True)


def sqrt_importance(x, prob: Problem):
    if prob.importance == IMP_GAUSSIAN:
        return O.sqrt_importance(x, prob.sigma)
    if prob.importance == IMP_UNIFORM:
        return torch.full((x.shape[0], 1), math.sqrt(1.0 / (2 * prob.sigma) ** x.shape[1]), dtype=x.dtype)
    return torch.ones(x.shape[0], 1, dtype=x.dtype)


def potential(x, prob: Problem):
    if prob.potential == POT_ZERO:
        return torch.zeros(x.shape[0], 1, dtype=x.dtype)
    return O.potential(x, prob)


def wave(xe, p: O.Params, prob: Problem, keep=False):
    """c * base(x) * exponential mask(x) * box mask(x); keep: also (phi, zs, base, exponential mask)"""
    phi = O.fourier_features(xe, p.fourier_B)
    base, zs = O.mlp_forward(phi, p, keep=True)
    m = O.boundary_mask(xe, p)
    u = prob.hard_mul_const * base * box_mask(xe, prob)
    if m is not None:
        u = u * m
    return (u, (phi, zs, base, m)) if keep else u


def operator_forward(x, p: O.Params, prob: Problem) -> O.OperatorCache:
    """Tf, f of OperatorWrapper(NegativeHamiltonian)(model, x, importance) as O.operator_forward states it, with the
    box mask in the model, the problem's density and potential. eps <= 0: the exact Laplacian by double autograd, the
    way the reference takes it (diff_ops.py:54-99). The cache is what O.operator_backward reads, with the box mask's
    centre value folded into sp0 (df reaches base and scales through sp0 / spc0 times the masks)."""
    B, D = x.shape
    if prob.eps <= 0:
        xr = x.detach().clone().requires_grad_(True)
        u, (phi0, zs, base0, mask0) = wave(xr, p, prob, keep=True)
        g = sqrt_importance(xr, prob) * u
        lap = torch.zeros_like(g)
        for l in range(g.shape[1]):
            (grad,) = torch.autograd.grad(g[:, l].sum(), xr, create_graph=True)
            for d in range(D):
                lap[:, l] += torch.autograd.grad(grad[:, d].sum(), xr, retain_graph=True)[0][:, d]
        g, phi0, zs, base0 = g.detach(), phi0.detach(), [z.detach() for z in zs], base0.detach()
        mask0 = None if mask0 is None else mask0.detach()
    else:
        pts = O.stencil_points(x, prob.eps)
        gs = []
        for j, xe in enumerate(pts):
            if j == 0:
                u, (phi0, zs, base0, mask0) = wave(xe, p, prob, keep=True)
            else:
                u = wave(xe, p, prob)
            gs.append(sqrt_importance(xe, prob) * u)
        lap = -2 * D * gs[0]
        for i in range(D):
            lap = lap + (gs[1 + 2 * i] + gs[2 + 2 * i])
        lap = lap / (prob.eps ** 2)
        g = gs[0]
    sp0 = sqrt_importance(x, prob)
    spc0 = torch.clamp(sp0, min=O.SQRT_P_CLAMP) if prob.importance != IMP_NONE else sp0
    lap = lap / spc0
    fs = g / spc0
    Tf = -(-prob.scale_kinetic * lap + potential(x, prob) * fs)
    Tf = prob.op_scale * Tf + prob.op_shift * fs
    return O.OperatorCache(x, phi0, zs, base0, mask0, sp0 * box_mask(x, prob), spc0, fs, Tf)


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
    """O.spectrum_evd (methods/spectrum.py:29-102, importance_val uniform on the validation box) on this operator;
    returns the eigenvalues diag(quad) / diag(cov) and the norms diag(cov)"""
    D = grid.shape[1]
    sqrt_val = math.sqrt(float(np.float32(1.0 / (2 * lim) ** D)))  # (a float32 value in the reference: main_pde.py:130)
    c = operator_forward(grid, p, prob)
    w = sqrt_importance(grid, prob) / sqrt_val
    phi = torch.nan_to_num(w * c.f)
    Tphi = torch.nan_to_num(w * c.Tf)
    Tphi[torch.all(torch.isclose(grid, torch.zeros_like(grid[0])), dim=1)] = 0.0
    n = grid.shape[0]
    cov, quad = phi.T @ phi / n, phi.T @ Tphi / n
    return dict(eigvals=torch.diag(quad) / torch.diag(cov), norms=torch.diag(cov), cov=cov, quad=quad)


def wall_rows(x, prob: Problem):
    """rows with a stencil point clamped or outside the box (|x_d| + eps >= lim for some d; exact mode: |x_d| >= lim)"""
    e = max(float(np.float32(prob.eps)), 0.0)
    return ((x.abs() + e) >= prob.box_lim).any(dim=1)


def infinite_well_2d_eigvals(neigs, L):
    """(n_x^2 + n_y^2) pi^2 / L^2 over n_x, n_y >= 1, ascending (ground_truths.py:52-57)"""
    vals = sorted(nx * nx + ny * ny for nx in range(1, neigs + 1) for ny in range(1, neigs + 1))[:neigs]
    return np.array(vals, dtype=np.float64) * np.pi ** 2 / L ** 2


def problem_of(cfg) -> Problem:
    """the fixture's recorded argument set -> Problem"""
    pot = {"infinite_well": POT_ZERO, "harmonic_oscillator": O.POT_HARMONIC, "hydrogen": O.POT_HYDROGEN}
    box = {"dir_box_sqrt": BOX_SQRT, "dir_box_exp": BOX_EXP}[cfg["boundary_mode"]] if cfg["apply_boundary"] else BOX_NONE
    return Problem(potential=pot[cfg["potential_type"]],
                   charge_or_k=cfg["charge"] if cfg["potential_type"] == "hydrogen" else 1.0,
                   eps=cfg["laplacian_eps"], op_scale=cfg["operator_scale"], op_shift=cfg["operator_shift"],
                   sigma=cfg["sampling_scale"], hard_mul_const=cfg["hard_mul_const"],
                   importance=IMP_UNIFORM if cfg["sampling_mode"] == "uniform" else IMP_GAUSSIAN,
                   box_mode=box, box_lim=float(cfg["lim"]))
