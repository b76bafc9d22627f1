"""CPU checks of the float64 restatement of NeuralEF's kernel-operator step (tests/_nef_kernel_oracle.py) against the
fixture recorded from the reference's own NeuralEigenfunctions (tests/golden/nef_kernel.npz, written by
tests/golden/make_golden_nef_kernel.py), of its hand-written reverse mode against torch autograd, and of the order of
the running-norm updates. No GPU.

Tolerances: the oracle and the reference's float64 run compute the same step in float64 in another order (one model
evaluation against two or four, a hand-derived cotangent against autograd): 1e-9 relative, the bound the SpIN and SpINx
oracles are held to; the hand-written du against autograd through u / n(u) on well-scaled columns: 1e-12.
"""
import os

import numpy as np
import pytest
import torch

from tests import _nef_kernel_oracle as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nef_kernel.npz")
F64 = torch.float64


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _runs():
    return [(name, tag, split) for name in sorted(N.SHAPES) for tag, *_ in N.variants(name) for split in (False, True)]


def _variant(name, tag):
    return next(v for v in N.variants(name) if v[0] == tag)


def test_fixture_holds_arrays_only_and_every_case(golden):
    assert os.path.getsize(GOLDEN) < 1 << 20
    for k in golden.files:
        assert golden[k].dtype.kind in "fi", k
    # six shapes x two unbiased values x two split modes, plus three more variants of shape a in both split modes
    assert len(_runs()) == 6 * 2 * 2 + 3 * 2
    for name, tag, split in _runs():
        for it in range(N.NSTEPS):
            assert N.prefix(name, tag, split, it) + "vals" in golden.files
    halves = sorted(N.chunk_rows(cs["B"], True) for cs in N.SHAPES.values())
    assert (5, 5) in halves and (17, 16) in halves and (48, 48) in halves and max(cs["L"] for cs in N.SHAPES.values()) == 64


@pytest.mark.parametrize("name,tag,split", _runs())
def test_oracle_reproduces_the_reference(golden, name, tag, split):
    _, unbiased, mode, include_diag = _variant(name, tag)
    fB, ws, bs, xs = N.load_case(golden, name)
    orc = N.NefOracle(fB, ws, bs, N.gaussian_kernel(N.ELL), N.case_c(name), unbiased, mode, include_diag)
    B1, _ = N.chunk_rows(N.SHAPES[name]["B"], split)
    for it in range(N.NSTEPS):
        res = orc.step(xs[it], split)
        nr, dr = N.admission(res["phi"], res["Kphi"], res["stats"], B1, split, unbiased)
        assert nr >= N.NORM_RATIO_MIN and dr >= N.DIAG_RATIO_MIN, (nr, dr)
        for k, (ref, _) in N.unpack_step(golden, name, tag, split, it).items():
            e = N.rel_err(N.sample(N.flat(res)[k]), ref)
            assert e <= 1e-9, (it, k, e)
        orc.sgd(res["grad"], N.LR)


@pytest.mark.parametrize("B,B1,L", [(2, 2, 1), (2, 1, 1), (3, 2, 2), (65, 33, 33), (130, 130, 64)])
def test_hand_written_du_is_autograd_through_the_normalisation(B, B1, L):
    g = torch.Generator().manual_seed(B * 100 + L)
    u = (torch.randn(B, L, generator=g, dtype=F64) * (0.5 + torch.rand(L, generator=g, dtype=F64))).requires_grad_(True)
    cot = torch.randn(B, L, generator=g, dtype=F64)
    phi, stats = N.normalize(u, B1)
    (want,) = torch.autograd.grad((phi * cot).sum(), u)
    got = N.normalize_backward(phi.detach(), stats.detach(), B1, cot)
    if B - B1 == 1 or B1 == 1:
        # a one-row segment: phi = sign(u) whatever u is, the cotangent is zero up to rounding (absolute check)
        rows = slice(B1, None) if B - B1 == 1 else slice(0, 1)
        assert float(got[rows].abs().max()) <= 1e-12 * float((cot[rows].abs() / stats.detach()[1 if B - B1 == 1 else 0]).max())
    assert N.rel_err(got, want) <= 1e-12
    # without batch norms the cotangent passes through
    assert torch.equal(N.normalize_backward(None, None, B1, cot), cot)


def test_running_norm_updates_follow_the_operator_callable(golden):
    """segments 0, 1, 1, 0 per split step (0 once otherwise), the first update ever a copy: with 1, 0, 0, 1 the first
    step would leave norms that differ from the fixture's by far more than the bound"""
    name = "t3"
    fB, ws, bs, xs = N.load_case(golden, name)
    assert N.update_order(False) == (0,) and N.update_order(True) == (0, 1, 1, 0)
    orc = N.NefOracle(fB, ws, bs, N.gaussian_kernel(N.ELL), N.case_c(name))
    res = orc.step(xs[0], True)
    assert orc.updates == [0, 1, 1, 0]
    n1, n2 = res["stats"]
    m = N.MOMENTUM

    def replay(order):
        st = dict(biased=None, unbiased=None, initialized=False)
        for h in order:
            N.running_update(st, (n1, n2)[h])
        return st

    right, wrong = replay((0, 1, 1, 0)), replay((1, 0, 0, 1))
    # by hand: copy n1, then two updates with n2, then one with n1
    rb = m * (m * (m * n1 + (1 - m) * n2) + (1 - m) * n2) + (1 - m) * n1
    ru = torch.sqrt(m * (m * (m * n1 ** 2 + (1 - m) * n2 ** 2) + (1 - m) * n2 ** 2) + (1 - m) * n1 ** 2)
    assert N.rel_err(right["biased"], rb) <= 1e-14 and N.rel_err(right["unbiased"], ru) <= 1e-14
    want = N.unpack_step(golden, name, "b0", True, 0)
    for key, k in (("biased", "norm_biased"), ("unbiased", "norm_unbiased")):
        assert N.rel_err(right[key], want[k][0]) <= 1e-9
        assert N.rel_err(wrong[key], want[k][0]) > 1e-3  # the two orders are told apart
    # not split: one update per step, and the second step is no copy
    orc = N.NefOracle(fB, ws, bs, N.gaussian_kernel(N.ELL), N.case_c(name))
    s0 = orc.step(xs[0], False)
    assert torch.equal(s0["norm_biased"], s0["stats"][0]) and torch.equal(s0["norm_unbiased"], s0["stats"][0])
    s1 = orc.step(xs[1], False)
    assert orc.updates == [0, 0]
    assert N.rel_err(s1["norm_biased"], m * s0["stats"][0] + (1 - m) * s1["stats"][0]) <= 1e-14


def test_loss_forms_agree():
    """the chunked call (phi1, phi2 the chunks of phi) and the sum of the three returned gradients"""
    g = torch.Generator().manual_seed(5)
    B, B1, L = 11, 6, 4
    phi, K = torch.randn(B, L, generator=g, dtype=F64), torch.randn(B, L, generator=g, dtype=F64)
    for unbiased in (False, True):
        for diagonal in (0, 1):
            loss, d, d1, d2 = N.loss_and_grads(phi, K, phi[:B1], K[:B1], phi[B1:], K[B1:], unbiased, diagonal)
            var = -K / B
            c1, c2 = N.coefficients(phi[:B1], K[:B1], phi[B1:], K[B1:], unbiased, diagonal)
            assert torch.equal(d, 4 * var)
            assert N.rel_err(d1, 2 * K[:B1] @ c1 / B1) <= 1e-15 and N.rel_err(d2, 2 * K[B1:] @ c2 / (B - B1)) <= 1e-15
            if diagonal == 1:
                assert not bool(torch.tril(c1).count_nonzero()) and not bool(torch.tril(c2).count_nonzero())
            assert torch.isfinite(loss)


def test_exports_and_refusals_without_a_gpu():
    import neural_svd_amd
    from neural_svd_amd.neuralef import NefKernelTrainer
    assert neural_svd_amd.NefKernelTrainer is NefKernelTrainer and "NefKernelTrainer" in neural_svd_amd.__all__
    with pytest.raises(NotImplementedError, match="MatrixFreeKernelOperator"):
        NefKernelTrainer(object(), L=4, m=8)
    with pytest.raises(ValueError, match="batchnorm_mode"):
        NefKernelTrainer(object(), L=4, m=8, batchnorm_mode="batch")
    with pytest.raises(ValueError, match="at least 2 rows"):
        NefKernelTrainer(object(), L=4, m=8, batch_size=1, split_batch=True)
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    op = RadialKernelOperator(H.RBF_GAUSSIAN, 1.0, 2)  # (no GPU call before the shape checks)
    for L in (0, 65):
        with pytest.raises(ValueError, match=r"L must be in 1\.\.64"):
            NefKernelTrainer(op, L=L, m=8)
