"""Float64 restatement of NeuralEF on the operator path (reference methods/neuralef.py, methods/utils.py:36-68,
examples/operator/pde/diff_ops.py:9-52) built from oracle.nsvd_oracle's pieces. The tests hold it to the reference's own
float64 run (tests/golden/neuralef.npz) on the CPU, and the HIP kernels to it on the GPU."""
from __future__ import annotations

import dataclasses
import math

import torch

from oracle import nsvd_oracle as O

MOMENTUM = 0.9


def wave_outputs(x, p: O.Params, prob: O.Problem):
    """u_e = c * base(x_e) * mask(x_e) at the 1 + 2D stencil points, in the reference's order"""
    out = []
    for xe in O.stencil_points(x, prob.eps):
        u = prob.hard_mul_const * O.mlp_forward(O.fourier_features(xe, p.fourier_B), p)
        m = O.boundary_mask(xe, p)
        out.append(u if m is None else u * m)
    return out


def update_running(running, norms, momentum=MOMENTUM):
    """running = [norm_biased, norm_unbiased, initialized]; one update per stencil point (utils.py:58-68)"""
    rb, ru, init = running
    for n in norms:
        if not init:
            rb, ru, init = n.clone(), n.clone(), True
        else:
            rb = momentum * rb + (1 - momentum) * n
            ru = torch.sqrt(momentum * ru ** 2 + (1 - momentum) * n ** 2)
    return [rb, ru, init]


def operator_forward(x, p: O.Params, prob: O.Problem, running=None, normalize=True, training=True, momentum=MOMENTUM):
    """Tphi, phi of operator(BatchL2NormalizedFunctions(model), x, importance) (normalize=False: batchnorm_mode 'none').
    Returns a dict with phi, Tphi, the batch norms, the updated running norms and what the backward needs."""
    B, D = x.shape
    pts = O.stencil_points(x, prob.eps)
    us = wave_outputs(x, p, prob)
    if normalize and training:
        norms = [u.norm(dim=0, keepdim=True) / math.sqrt(B) for u in us]
        running = update_running(running, norms, momentum)
    elif normalize:
        norms = [running[0]] * len(us)
    else:
        norms = [torch.ones(1, us[0].shape[1], dtype=x.dtype)] * len(us)
    sps = [O.sqrt_importance(xe, prob.sigma) if prob.use_importance else torch.ones(B, 1, dtype=x.dtype) for xe in pts]
    gs = [sp * u / n for sp, u, n in zip(sps, us, norms)]
    lap = -2 * D * gs[0]
    for i in range(D):
        lap = lap + (gs[1 + 2 * i] + gs[2 + 2 * i])
    lap = lap / (prob.eps ** 2)
    spc = torch.clamp(sps[0], min=O.SQRT_P_CLAMP) if prob.use_importance else sps[0]
    lap = lap / spc
    phi = gs[0] / spc
    Tphi = -(-prob.scale_kinetic * lap + O.potential(x, prob) * phi)
    Tphi = prob.op_scale * Tphi + prob.op_shift * phi
    return dict(phi=phi, Tphi=Tphi, norms=norms, running=running, u0=us[0], n0=norms[0], r=sps[0] / spc)


def loss_and_dphi(phi, Tphi, unbiased, diagonal=1, phi1=None, Tphi1=None, phi2=None, Tphi2=None):
    """NeuralEigenfunctionsLossFunction: loss and the pseudo-gradients (dphi, dphi1, dphi2) (neuralef.py:37-62).
    Without halves: the chunks of phi (compute_loss_operator), dphi1 / dphi2 then added into dphi's rows."""
    chunked = phi1 is None
    if chunked:
        phi1, phi2 = torch.chunk(phi, 2)
        Tphi1, Tphi2 = torch.chunk(Tphi, 2)
    B, B1, B2 = phi.shape[0], phi1.shape[0], phi2.shape[0]
    var = -Tphi / B
    if unbiased:
        c1 = (phi1.T @ phi1 / B1).triu(diagonal)
        c2 = (phi2.T @ phi2 / B2).triu(diagonal)
    else:
        q1 = phi1.T @ Tphi1 / B1
        q2 = phi2.T @ Tphi2 / B2
        c1 = q2.triu(diagonal) / (q2.diag() + 1e-5).view(-1, 1)
        c2 = q1.triu(diagonal) / (q1.diag() + 1e-5).view(-1, 1)
    a1 = Tphi1 @ c1 / B1
    a2 = Tphi2 @ c2 / B2
    loss = (phi * var).sum() + 0.5 * ((phi1 * a1).sum() + (phi2 * a2).sum())
    if chunked:
        return loss, 4 * var + 2 * torch.cat([a1, a2]), None, None
    return loss, 4 * var, 2 * a1, 2 * a2


def norm_backward(dphi, fwd):
    """d loss / d u0 through phi = r u0 / n0 with n0 the batch norm of u0: du0 = (dh - h mean_b(dh h)) / n0"""
    h = fwd["u0"] / fwd["n0"]
    dh = fwd["r"] * dphi
    return (dh - h * (dh * h).mean(0, keepdim=True)) / fwd["n0"]


def param_grads(x, p: O.Params, prob: O.Problem, du0):
    """gradients of sum(du0 * u0) in Params.trainable() order (the centre backward of nsvd_oracle with r = 1)"""
    c = O.operator_forward(x, p, prob)
    one = torch.ones_like(c.sp0)
    return O.operator_backward(dataclasses.replace(c, sp0=one, spc0=one), p, prob, du0)


def train_step(x, p: O.Params, prob: O.Problem, running, unbiased, normalize=True, diagonal=1, momentum=MOMENTUM):
    """one compute_loss_operator + backward; returns (fwd dict, loss, grads in Params.trainable() order)"""
    fwd = operator_forward(x, p, prob, running, normalize, momentum=momentum)
    loss, dphi, _, _ = loss_and_dphi(fwd["phi"], fwd["Tphi"], unbiased, diagonal)
    if normalize:
        grads = param_grads(x, p, prob, norm_backward(dphi, fwd))
    else:
        c = O.operator_forward(x, p, prob)
        grads = O.operator_backward(c, p, prob, dphi)
    return fwd, loss, grads
