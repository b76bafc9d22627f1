"""Float64 oracle of the exact-Laplacian mode (laplacian_eps <= 0: VectorizedLaplacian.exact_laplacian, reference
examples/operator/pde/diff_ops.py:54-61) for ANY input dimension, potential, mask and density the HIP kernels carry on
NSVD_PATH_GENERIC_EXACT - and of the two jet kernels that path adds.

The operator is not restated here: tests/_highdim_oracle.py (composed around _periodic_oracle, _box_oracle and
oracle.nsvd_oracle) already takes the Laplacian by double autograd of the float64 model whenever prob.eps <= 0, at any D
- this module pins that branch to the reference's own exact mode (tests/golden/exact_nd.npz, test_generic_exact_oracle)
and adds what the GPU tests of the jets need: the jets of the Fourier map and of softplus in the kernels' layout, and
the distance of a batch from every singular point (with a constructor of batches that keep it)."""
from __future__ import annotations

import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _highdim_oracle as HO

Problem = HO.Problem


def loss_and_grads(x, p: O.Params, prob: Problem, v, M):
    """f, Tf, df and the parameter gradients of one NestedLoRA step in exact mode, float64 (x, p float64)"""
    assert not prob.eps > 0, "the exact mode is laplacian_eps <= 0"
    return HO.loss_and_grads(x, p, prob, v, M)


def fourier_jets(x, fB):
    """phiT (2 m, (D + 2) B), float64: block 0 [sin | cos](x B), block 1 + d the derivative along d, block D + 1 the
    Laplacian"""
    t = (x @ fB).T  # (m, B)
    sn, cs = torch.sin(t), torch.cos(t)
    blocks = [torch.cat([sn, cs], 0)]
    for d in range(x.shape[1]):
        bd = fB[d].view(-1, 1)
        blocks.append(torch.cat([cs * bd, -sn * bd], 0))
    q = (fB * fB).sum(0).view(-1, 1)
    blocks.append(torch.cat([-q * sn, -q * cs], 0))
    return torch.cat(blocks, 1)


def softplus_jets(z, B, D):
    """z (rows, (D + 2) B), the jet of a pre-activation -> the jet of softplus(z), same layout (torch's threshold 20)"""
    z0, l = z[:, :B], z[:, (D + 1) * B:]
    s = O.softplus_grad(z0)
    s2 = torch.where(z0 > O.SOFTPLUS_THRESHOLD, torch.zeros_like(z0), s * (1 - s))
    ts = [z[:, (1 + d) * B:(2 + d) * B] for d in range(D)]
    sq = sum(t * t for t in ts)
    return torch.cat([O.softplus(z0)] + [s * t for t in ts] + [s * l + s2 * sq], 1)


def clearance(x, p_scales, prob: Problem):
    """per row: the distance to the nearest point where the operator is singular or has a kink - the origin (hydrogen
    potential, exponential mask: grad mask = -(x / r) / s mask), a nucleus, a coalescence point, a wall of the box"""
    x = x.double()
    out = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    if prob.potential == O.POT_HYDROGEN or p_scales is not None:
        out = torch.minimum(out, x.norm(dim=1))
    if prob.potential == HO.POT_H2_ION:
        e = torch.zeros(x.shape[1], dtype=torch.float64)
        e[-1] = prob.pot_coef[0]
        out = torch.minimum(out, torch.minimum((x - e).norm(dim=1), (x + e).norm(dim=1)))
    if prob.potential == HO.POT_MOLECULE:
        en, ee = HO.distances(x, prob)
        out = torch.minimum(out, torch.minimum(en, ee))
    if prob.box_mode != BO.BOX_NONE:
        out = torch.minimum(out, (prob.box_lim - x.abs()).min(dim=1).values)
    return out


def clear_batch(B, D, span, scales, prob: Problem, seed):
    """B float32-valued rows uniform in [-span, span]^D, more than 0.1 from every singular point BY CONSTRUCTION: rows
    that are closer are drawn again from the same generator (the tests assert the clearance of what they get)"""
    g = torch.Generator().manual_seed(seed)

    def draw(n):
        return (span * (2 * torch.rand(n, D, generator=g, dtype=torch.float64) - 1)).float().double()
    x = draw(B)
    for _ in range(200):
        bad = clearance(x, scales, prob) <= 0.1
        if not bool(bad.any()):
            return x
        x[bad] = draw(int(bad.sum()))
    raise AssertionError("no clear batch")
