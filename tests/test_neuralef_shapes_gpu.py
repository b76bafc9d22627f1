"""NeuralEF on the HIP kernels at the shapes tests/test_neuralef_gpu.py does not reach, against the float64 restatement
(tests/_neuralef_oracle.py, oracle/nsvd_oracle.py):

  1. the loss kernels (nef_gram / nef_gram_sum / nef_align / nef_loss) at L from 1 to 64, single partial 64-row blocks,
     halves of unequal row counts, B1 + B2 == B on separately allocated halves, every unbiased x diagonal combination on
     both forms, bit reproducibility, the refusals and the autograd wrapper's three-gradient return;
  2. the fused training step (nef_norms / nef_epilogue / nef_norm_bwd around the operator forward stopped at the raw head
     outputs) at input dimension 1, 3 and 4 on the generic and the MFMA kernels (the split form at D = 3), with and
     without the mask and the importance weight, hard_mul_const != 1, a momentum that is not 0.9, a row at the origin and
     a row on the sqrt p clamp;
  3. evaluation mode (the biased running norm in either mode) and nef_scale_heads to one ulp;
  4. NeuralEigenfunctions.compute_loss_kernel, both split_batch modes, against torch autograd in float64.

Bounds are test_neuralef_gpu's: the loss kernel's loss within 1e-5 of sum |phi Tphi| / B and its gradients 1e-5 relative;
of a step phi and the running norms 2e-5, Tphi, the loss and every parameter gradient 1e-4. Where Tphi of a step misses
1e-4 the bound is max(1e-4, 2 x the Tf error of the plain operator forward (batchnorm 'none', held to float64 by
test_hip_parity and test_highdim_gpu) on the same weights and rows): the nu terms enter at the size of the stencil
weights themselves. The special rows (origin, clamp) and the remaining rows are measured as two groups, each against
its own norm; no row is left out."""
import dataclasses
import functools
import math
from functools import partial
from types import SimpleNamespace as NS

import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _neuralef_oracle as NO
from tests.test_neuralef_gpu import build_model, gpu_step, neuralef

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def rel(a, b):
    """relative L2 error; against an exactly zero reference (triu(G, 1) of one head) only exact zeros pass"""
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    nb = float(b.norm())
    if nb == 0.0:
        return 0.0 if float(a.norm()) == 0.0 else math.inf
    return float((a - b).norm()) / nb


# =============================================================================================== 1. loss kernels
LOSS_SEED = 7
LOSS_L = (1, 2, 5, 17, 64)
LOSS_B = (2, 3, 63, 64, 65, 129, 1000)
HALVES = ((96, 96, 96), (130, 65, 65), (100, 37, 200), (64, 1, 129))
HALVES_L = (1, 5, 64)
FLAGS = tuple((u, d) for u in (0, 1) for d in (0, 1))


def _lam(L):
    return torch.linspace(1.0, 3.0, L, dtype=torch.float64)


def _draw(g, B, L, lam):
    """phi = randn, Tphi = phi lam + 0.3 randn, both exactly representable in float32"""
    phi = torch.randn(B, L, generator=g, dtype=torch.float64).float().double()
    Tphi = (phi * lam + 0.3 * torch.randn(B, L, generator=g, dtype=torch.float64)).float().double()
    return phi, Tphi


def divisor(p, t):
    """|diag(phi_h^T Tphi_h / B_h) + 1e-5|: what the biased form divides by"""
    return ((p * t).sum(0) / p.shape[0] + 1e-5).abs()


def divisor_ok(p, t):
    d = divisor(p, t)
    return d >= 0.1 * d.median()


def _settle(g, p, t, lam):
    """The divisor condition by rejection: the heads of this half that miss it are drawn again (the same recipe, the same
    generator) until none does. A seed for the whole tensor cannot do it: with one or two rows in a half the condition
    asks all L heads to avoid |phi| < ~0.2 at once, which 20000 draws of a single row at L = 64 never did."""
    for _ in range(1000):
        bad = ~divisor_ok(p, t)
        if not bool(bad.any()):
            return
        pn, tn = _draw(g, p.shape[0], int(bad.sum()), lam[bad])
        p[:, bad] = pn
        t[:, bad] = tn
    raise AssertionError("divisor condition not reached")


@functools.lru_cache(maxsize=None)
def chunked_inputs(B, L):
    g = torch.Generator().manual_seed(LOSS_SEED * 1000003 + 131 * B + L)
    lam = _lam(L)
    phi, Tphi = _draw(g, B, L, lam)
    for p, t in zip(torch.chunk(phi, 2), torch.chunk(Tphi, 2)):  # views: the redrawn heads land in phi / Tphi
        _settle(g, p, t, lam)
    return phi, Tphi


@functools.lru_cache(maxsize=None)
def halves_inputs(B, B1, B2, L):
    g = torch.Generator().manual_seed(LOSS_SEED * 1000003 + 131 * (B + 7 * B1 + 49 * B2) + L)
    lam = _lam(L)
    out = []
    for i, rows in enumerate((B, B1, B2)):
        p, t = _draw(g, rows, L, lam)
        if i:  # (phi / Tphi of the variance term divide nothing)
            _settle(g, p, t, lam)
        out += [p, t]
    return tuple(out)


def assert_divisors(*halves):
    """the condition on the inputs, on the float64 side, for every half"""
    for p, t in halves:
        d = divisor(p, t)
        assert float(d.min()) >= 0.1 * float(d.median()), (tuple(p.shape), float(d.min()), float(d.median()))


def loss_close(loss, want, scale):
    assert bool(torch.isfinite(loss).all())
    return abs(float(loss[0]) - float(want)) < 1e-5 * scale


@pytest.mark.parametrize("B", LOSS_B)
@pytest.mark.parametrize("L", LOSS_L)
def test_loss_kernel_chunked(L, B):
    """phi1, phi2 = torch.chunk(phi, 2) as views: one fused pass, one gradient. B = 2, 3, 63: a single partial block per
    half; 64, 65, 129: a full block, a full block and one row, nblk[0] != nblk[1] (65 / 64 rows).
    L = 1, biased, diagonal 0: coeff = Q / (Q + 1e-5), and 2 align cancels 4 variance down to the 1e-5 remainder (at
    even B all of it). nef_align_kernel used to round coeff itself to float32 there: dphi was off by 3.4e-4 (B = 2),
    3.0e-3 (B = 64) and 5.6e-3 (B = 1000) of its norm; it now forms the remainder directly."""
    from neural_svd_amd import hip_ops as H
    phi, Tphi = chunked_inputs(B, L)
    assert_divisors(*zip(torch.chunk(phi, 2), torch.chunk(Tphi, 2)))
    pd, Td = phi.float().to(DEV), Tphi.float().to(DEV)
    assert torch.equal(pd.double().cpu(), phi) and torch.equal(Td.double().cpu(), Tphi)
    p1, p2 = torch.chunk(pd, 2)
    t1, t2 = torch.chunk(Td, 2)
    scale = float((phi * Tphi).abs().sum()) / B
    for unbiased, diag in FLAGS:
        want, dwant, _, _ = NO.loss_and_dphi(phi, Tphi, unbiased, diag)
        loss, dphi, d1, d2 = H.nef_loss(pd, Td, p1, t1, p2, t2, unbiased, diag)
        assert d1 is None and d2 is None
        e = rel(dphi, dwant)
        print(f"chunked B={B} L={L} unbiased={unbiased} diagonal={diag}: loss {abs(float(loss[0]) - float(want)) / scale:.2e}"
              f" of scale, dphi {e:.2e}")
        assert loss_close(loss, want, scale), (unbiased, diag)
        assert e < 1e-5, (unbiased, diag, e)


@pytest.mark.parametrize("L", HALVES_L)
@pytest.mark.parametrize("B,B1,B2", HALVES)
def test_loss_kernel_independent_halves(B, B1, B2, L):
    """separately allocated halves take the general form: (130, 65, 65) has B1 + B2 == B and must NOT be read as the
    chunks of phi; (100, 37, 200) and (64, 1, 129) have nblk[0] != nblk[1] (1 and 4, 1 and 3 blocks)."""
    from neural_svd_amd import hip_ops as H
    cpu = halves_inputs(B, B1, B2, L)
    assert_divisors(cpu[2:4], cpu[4:6])
    dev = [t.float().to(DEV) for t in cpu]
    scale = float((cpu[0] * cpu[1]).abs().sum()) / B
    for unbiased, diag in FLAGS:
        want, dv, w1, w2 = NO.loss_and_dphi(cpu[0], cpu[1], unbiased, diag, *cpu[2:])
        loss, dphi, d1, d2 = H.nef_loss(*dev, unbiased, diag)
        assert d1 is not None and d2 is not None
        assert tuple(d1.shape) == (B1, L) and tuple(d2.shape) == (B2, L)
        e = (rel(dphi, dv), rel(d1, w1), rel(d2, w2))
        print(f"halves {(B, B1, B2)} L={L} unbiased={unbiased} diagonal={diag}: loss "
              f"{abs(float(loss[0]) - float(want)) / scale:.2e} of scale, dphi {e[0]:.2e} d1 {e[1]:.2e} d2 {e[2]:.2e}")
        assert loss_close(loss, want, scale), (unbiased, diag)
        assert max(e) < 1e-5, (unbiased, diag, e)


def test_loss_kernel_reproducible_bits():
    """fixed-order reductions (neuralef.hip's header): two calls on the same inputs give the same bits"""
    from neural_svd_amd import hip_ops as H
    pd, Td = (t.float().to(DEV) for t in chunked_inputs(129, 17))
    chunked = (pd, Td, *[c for pair in zip(torch.chunk(pd, 2), torch.chunk(Td, 2)) for c in pair])
    halves = tuple(t.float().to(DEV) for t in halves_inputs(100, 37, 200, 5))
    for args in (chunked, halves):
        for unbiased in (0, 1):
            a = H.nef_loss(*args, unbiased, 1)
            b = H.nef_loss(*args, unbiased, 1)
            for s, t in zip(a, b):
                assert (s is None) == (t is None)
                if s is not None:
                    assert bool(torch.isfinite(s).all()) and torch.equal(s, t)


def test_loss_kernel_refusals():
    from neural_svd_amd import hip_ops as H
    p = torch.zeros(4, 65, device=DEV)
    with pytest.raises(H.NsvdError, match="unsupported"):
        H.nef_loss(p, p, p, p, p, p, 1, 1)
    p = torch.zeros(65537, 1, device=DEV)
    p1, p2 = torch.chunk(p, 2)
    with pytest.raises(H.NsvdError, match="unsupported"):
        H.nef_loss(p, p, p1, p1, p2, p2, 1, 1)


def test_loss_function_backward():
    """NeuralEigenfunctionsLossFunction: the pseudo-gradients of the kernel reach phi, phi1, phi2 bit for bit whatever
    grad_output is (reference methods/neuralef.py:52-62), the Tphi's get none; chunked: phi alone gets one."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.neuralef import NeuralEigenfunctionsLossFunction as F
    dev = [t.float().to(DEV) for t in halves_inputs(100, 37, 200, 5)]
    loss0, dphi, d1, d2 = H.nef_loss(*dev, True, 1)
    leaves = [t.clone().requires_grad_(True) for t in dev]
    loss = F.apply(*leaves, 1, 1)
    assert torch.equal(loss.detach(), loss0[0])
    (3.0 * loss).backward()
    for leaf, want in zip(leaves[0::2], (dphi, d1, d2)):
        assert bool(torch.isfinite(leaf.grad).all()) and torch.equal(leaf.grad, want)
    for leaf in leaves[1::2]:
        assert leaf.grad is None
    # chunked
    pd, Td = (t.float().to(DEV) for t in chunked_inputs(129, 17))
    (c1, c2), (s1, s2) = torch.chunk(pd, 2), torch.chunk(Td, 2)
    loss0, dphi, none1, none2 = H.nef_loss(pd, Td, c1, s1, c2, s2, True, 1)
    assert none1 is None and none2 is None
    phi, Tphi = pd.clone().requires_grad_(True), Td.clone().requires_grad_(True)
    p1, p2 = torch.chunk(phi, 2)
    t1, t2 = torch.chunk(Tphi, 2)
    for t in (p1, p2, t1, t2):
        t.retain_grad()
    loss = F.apply(phi, Tphi, p1, t1, p2, t2, 1, 1)
    assert torch.equal(loss.detach(), loss0[0])
    (3.0 * loss).backward()
    assert bool(torch.isfinite(phi.grad).all()) and torch.equal(phi.grad, dphi)
    for t in (Tphi, p1, p2, t1, t2):
        assert t.grad is None


# =============================================================================================== 2. training step
@dataclasses.dataclass(frozen=True)
class StepCase:
    name: str
    D: int
    potential: str          # "harmonic" (row 0 at the origin) or "hydrogen"
    mask: object            # ExponentialMask init scale or None
    sigma: object           # Gaussian importance (row 1 at 8 sigma on the first axis) or None: x = 2 randn
    c: float                # hard_mul_const
    B: int
    L: int
    wide: bool              # m = 64, hidden (128, 128); else m = 8, hidden (16, 16)
    path: str
    expect: str
    momentum: float = 0.9


STEP_CASES = (
    StepCase("d1_generic", 1, "harmonic", 10.0, 4.0, 1.0, 70, 5, False, "generic", "generic"),
    StepCase("d1_mfma", 1, "harmonic", 10.0, 4.0, 1.0, 96, 3, True, "fused", "fused_mfma"),
    StepCase("d3_generic", 3, "hydrogen", 4.0, 4.0, 0.9, 70, 5, False, "generic", "generic"),
    StepCase("d3_mfma_split", 3, "hydrogen", 4.0, 4.0, 0.9, 96, 3, True, "fused", "fused_mfma"),
    StepCase("d3_mfma_plain", 3, "harmonic", None, None, 1.0, 64, 2, True, "auto", "fused_mfma"),
    StepCase("d3_wide_b70", 3, "hydrogen", 4.0, 4.0, 1.0, 70, 3, True, "auto", "generic"),
    StepCase("d4_generic_plain", 4, "harmonic", None, None, 1.0, 96, 18, False, "auto", "generic"),
    StepCase("d4_wide", 4, "harmonic", 4.0, 2.0, 0.9, 64, 2, True, "auto", "generic"),
    StepCase("d2_generic", 2, "harmonic", 10.0, 4.0, 0.9, 70, 5, False, "generic", "generic"),
    StepCase("d1_generic_momentum", 1, "harmonic", 10.0, 4.0, 1.0, 70, 5, False, "generic", "generic", 0.5),
)
STEP_BY_NAME = {c.name: c for c in STEP_CASES}


def step_params(case):
    m, hidden = (64, (128, 128)) if case.wide else (8, (16, 16))
    return O.init_params(case.L, case.D, m, hidden, 0.2, case.mask, seed=11), hidden


def oracle_problem(case):
    hyd = case.potential == "hydrogen"
    return O.Problem(potential=O.POT_HYDROGEN if hyd else O.POT_HARMONIC, charge_or_k=1.0, eps=0.01,
                     op_scale=100.0 if hyd else 1.0, op_shift=0.0 if hyd else 16.0,
                     sigma=case.sigma if case.sigma is not None else 1.0, hard_mul_const=case.c,
                     use_importance=case.sigma is not None)


def hip_problem(case):
    from neural_svd_amd.operators import (GaussianImportance, NegativeHamiltonian, OperatorWrapper,
                                          harmonic_oscillator_potential, hydrogen_potential)
    po = oracle_problem(case)
    pot = partial(hydrogen_potential, charge=1.0) if case.potential == "hydrogen" else \
        partial(harmonic_oscillator_potential, k=1.0)
    op = OperatorWrapper(NegativeHamiltonian(pot, 1.0, po.eps), po.op_scale, po.op_shift)
    return op, (GaussianImportance(case.sigma, case.D) if case.sigma is not None else None)


def special_rows(case):
    rows = torch.zeros(case.B, dtype=torch.bool)
    rows[0] = case.potential == "harmonic"
    rows[1] = case.sigma is not None
    return rows


BATCH_SEED = 61   # chosen on the CPU: no case's float64 loss is a cancellation of its terms (step_oracle asserts it)


def step_batches(case, steps=2):
    g = torch.Generator().manual_seed(BATCH_SEED)
    out = []
    for _ in range(steps):
        x = (case.sigma if case.sigma is not None else 2.0) * torch.randn(case.B, case.D, generator=g)
        if case.potential == "harmonic":
            x[0] = 0.0                       # the origin: r0 = 0 in the mask ratio (hydrogen: V is infinite there)
        if case.sigma is not None:
            x[1] = 0.0
            x[1, 0] = 8.0 * case.sigma       # sqrt p < 1e-5: the clamp, r = sqrt p / 1e-5 < 1 into dphi
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def step_oracle(name):
    """the float64 side of a case: two steps, `running` threaded through; every condition on it is asserted here"""
    case = STEP_BY_NAME[name]
    p, _ = step_params(case)
    p64, po = p.to(torch.float64), oracle_problem(case)
    running = [None, None, False]
    steps = []
    for x in step_batches(case):
        fwd, loss, grads = NO.train_step(x.double(), p64, po, running, 1, momentum=case.momentum)
        running = fwd["running"]
        for t in (fwd["phi"], fwd["Tphi"], loss, *running[:2], *grads):
            assert bool(torch.isfinite(t).all())
        # the loss is held to 1e-4 of ITSELF: a condition on the inputs that it is no small difference of its terms
        assert float((fwd["phi"] * fwd["Tphi"]).abs().sum()) / case.B <= 32.0 * abs(float(loss))
        if case.sigma is not None:
            assert float(O.sqrt_importance(x.double()[1:2], case.sigma)) < O.SQRT_P_CLAMP
            assert float(fwd["r"][1]) < 1.0
        steps.append((x, fwd, loss, grads))
    return steps


def tf_yardstick(model, case, x, rows, path):
    """Tf error of the plain operator forward (batchnorm 'none') on the same weights and rows"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.operators import fused_problem_of
    op, imp = hip_problem(case)
    p, _ = step_params(case)
    shape = model.shape
    xd = x.float().to(DEV).contiguous()
    f, Tf = H.operator_forward(shape, model.packed_params(), fused_problem_of(op, imp, model), xd,
                               H.new_workspace(shape, xd.shape[0], DEV), path=path)
    want = O.operator_forward(x.double(), p.to(torch.float64), oracle_problem(case))
    return rel(Tf.cpu()[rows], want.Tf[rows])


def check_rows(what, phi, Tphi, fwd, groups, yardstick):
    for group, rows in groups:
        if not bool(rows.any()):
            continue
        ef, eT = rel(phi.cpu()[rows], fwd["phi"][rows]), rel(Tphi.cpu()[rows], fwd["Tphi"][rows])
        bound = 1e-4
        if eT >= bound:
            plain = yardstick(rows)
            bound = max(1e-4, 2.0 * plain)
            print(f"{what} {group}: Tphi {eT:.2e} misses 1e-4; plain operator forward Tf {plain:.2e}, bound {bound:.2e}")
        print(f"{what} {group} rows ({int(rows.sum())}): phi {ef:.2e} Tphi {eT:.2e}")
        assert ef < 2e-5, (what, group, ef)
        assert eT < bound, (what, group, eT, bound)


def make_method(case, mode="unbiased"):
    from neural_svd_amd import hip_ops as H
    p, hidden = step_params(case)
    model = build_model(p, hidden, 0.2)
    model.hard_mul_const = case.c
    path = {"auto": H.PATH_AUTO, "generic": H.PATH_GENERIC, "fused": H.PATH_FUSED}[case.path]
    assert model.shape.D == case.D and model.shape.has_exp_mask == (case.mask is not None)
    assert H.path_name(model.shape, case.B, path) == case.expect
    method = neuralef(model, case.L, path, mode)
    method.model.momentum = case.momentum
    return method, model, path


@pytest.mark.parametrize("name", [c.name for c in STEP_CASES])
def test_step_against_float64(name):
    """compute_loss_operator + backward, twice (the first call initialises the running norms, the second takes their
    EMA), against NO.train_step. Measured on an MI355X, the worse of the two steps (phi and Tphi: special rows / other
    rows; gradients: the worst tensor); the plain-operator yardstick for Tphi was needed by no case:

        case                 phi              Tphi             norms    loss     gradients
        d1_generic           2.2e-7 / 1.8e-7  3.0e-7 / 2.0e-7  9.7e-8   5.2e-7   6.3e-7
        d1_mfma              1.4e-7 / 1.7e-7  8.0e-7 / 1.9e-7  3.9e-8   9.7e-7   6.3e-6
        d3_generic           2.9e-7 / 3.0e-7  4.8e-7 / 9.2e-7  7.7e-8   1.1e-6   1.4e-6
        d3_mfma_split        1.9e-7 / 2.2e-7  2.8e-7 / 8.4e-7  1.4e-7   8.6e-7   1.3e-6
        d3_mfma_plain        3.3e-7 / 4.7e-7  5.0e-7 / 5.3e-7  1.1e-7   4.5e-7   6.3e-7
        d3_wide_b70          5.9e-7 / 2.9e-7  7.3e-7 / 9.3e-7  9.2e-8   6.9e-7   7.2e-7
        d4_generic_plain     1.0e-7 / 1.6e-7  2.8e-7 / 2.8e-7  1.0e-7   2.0e-6   8.3e-7
        d4_wide              1.2e-7 / 2.2e-7  1.3e-7 / 2.6e-7  1.4e-7   7.7e-7   3.0e-6
        d2_generic           1.9e-7 / 1.6e-7  2.9e-7 / 2.5e-7  9.1e-8   2.4e-7   1.2e-6
        d1_generic_momentum  2.2e-7 / 1.8e-7  3.0e-7 / 2.0e-7  8.4e-8   5.2e-7   6.3e-7"""
    case = STEP_BY_NAME[name]
    oracle = step_oracle(name)
    method, model, path = make_method(case)
    op, imp = hip_problem(case)
    special = special_rows(case)
    for it, (x, fwd, lwant, gwant) in enumerate(oracle):
        loss, phi, Tphi, grads = gpu_step(method, op, imp, x.to(DEV))
        check_rows(f"{name} step {it}", phi, Tphi, fwd, (("special", special), ("other", ~special)),
                   lambda rows: tf_yardstick(model, case, x, rows, path))
        eb = rel(method.model._norm_biased, fwd["running"][0])
        eu = rel(method.model._norm_unbiased, fwd["running"][1])
        el = rel(loss, lwant)
        eg = [rel(got, want) for got, want in zip(grads, gwant)]
        print(f"{name} step {it}: norms {eb:.2e} {eu:.2e} loss {el:.2e} grads " + " ".join(f"{e:.2e}" for e in eg))
        assert len(grads) == len(gwant) == 2 * len(model.base.ws) + (case.mask is not None)
        assert eb < 2e-5 and eu < 2e-5, (eb, eu)
        assert el < 1e-4, el
        assert max(eg) < 1e-4, eg


# =============================================================================================== 3. evaluation mode
@pytest.mark.parametrize("mode", ["biased", "unbiased"])
@pytest.mark.parametrize("name", ["d3_generic", "d2_generic"])
def test_evaluation_mode(name, mode):
    """after two training steps: apply_operator in evaluation mode divides the operator's (Tf, f) by the BIASED running
    norm in either batchnorm_mode (utils.py:55 tests the mode string) and leaves both running norms alone"""
    case = STEP_BY_NAME[name]
    oracle = step_oracle(name)
    method, model, path = make_method(case, mode)
    op, imp = hip_problem(case)
    for x, _, _, _ in oracle:
        gpu_step(method, op, imp, x.to(DEV))
    running = oracle[-1][1]["running"]
    assert rel(method.model._norm_biased, running[0]) < 2e-5 and rel(method.model._norm_unbiased, running[1]) < 2e-5
    assert rel(running[0], running[1]) > 1e-4  # the two norms differ: taking the wrong one would show
    before = method.model._norm_biased.data.clone(), method.model._norm_unbiased.data.clone()
    x = case.sigma * torch.randn(70, case.D, generator=torch.Generator().manual_seed(9))  # 70 L: no multiple of 256
    method.eval()
    Tphi, phi = method.apply_operator(op, x.to(DEV), imp)
    assert torch.equal(method.model._norm_biased.data, before[0])
    assert torch.equal(method.model._norm_unbiased.data, before[1])
    p, _ = step_params(case)
    want = NO.operator_forward(x.double(), p.to(torch.float64), oracle_problem(case), running, normalize=True,
                               training=False)
    assert bool(torch.isfinite(want["phi"]).all()) and bool(torch.isfinite(want["Tphi"]).all())
    check_rows(f"{name} eval {mode}", phi, Tphi, want, (("all", torch.ones(70, dtype=torch.bool)),),
               lambda rows: tf_yardstick(model, case, x, rows, path))


@pytest.mark.parametrize("B,L", [(1, 1), (257, 3), (64, 64)])
def test_scale_heads_one_ulp(B, L):
    """one correctly rounded division per element (-fno-fast-math): within one float32 ulp of torch's f / norm"""
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(B + L)
    f, Tf = torch.randn(B, L, generator=g).to(DEV), (30.0 * torch.randn(B, L, generator=g)).to(DEV)
    norm = (0.5 + 1.5 * torch.rand(1, L, generator=g)).to(DEV)
    want = f / norm, Tf / norm
    got = f.clone(), Tf.clone()
    H.nef_scale_heads(got[0], got[1], norm)
    inf = torch.full_like(f, math.inf)
    for a, w in zip(got, want):
        assert bool(torch.isfinite(a).all())
        assert bool(((a >= torch.nextafter(w, -inf)) & (a <= torch.nextafter(w, inf))).all())


# =============================================================================================== 4. kernel loss
def kernel_loss_oracle(p64, x, split, mode, ell):
    """compute_loss_kernel in float64 with torch autograd; p64's ws / bs are leaves and receive the gradients.
    Returns loss, phi, Kphi and the running norms after the model's calls."""
    state = dict(running=[None, None, False])

    def model64(xe):
        u = O.mlp_forward(O.fourier_features(xe, p64.fourier_B), p64)
        if mode == "none":
            return u
        n = u.norm(dim=0, keepdim=True) / math.sqrt(xe.shape[0])
        state["running"] = NO.update_running(state["running"], [n.detach()])
        return u / n

    def op64(x_ref):
        def op(xe):
            f = model64(xe)
            with torch.no_grad():
                Kf = torch.exp(-torch.cdist(xe, x_ref) ** 2 / (2.0 * ell ** 2)) @ model64(x_ref) / x_ref.shape[0]
            return Kf, f
        return op

    if split:
        x1, x2 = torch.chunk(x, 2)
        K1, f1 = op64(x2)(x1)
        K2, f2 = op64(x1)(x2)
        f, Kf = torch.cat([f1, f2]), torch.cat([K1, K2])
        loss, dv, w1, w2 = NO.loss_and_dphi(f.detach(), Kf, 1, 1, f1.detach(), K1, f2.detach(), K2)
        ((f * dv).sum() + (f1 * w1).sum() + (f2 * w2).sum()).backward()
    else:
        Kf, f = op64(x)(x)
        loss, dv, w1, w2 = NO.loss_and_dphi(f.detach(), Kf, 1, 1, f.detach(), Kf, f.detach(), Kf)
        (f * (dv + w1 + w2)).sum().backward()
    return loss, f.detach(), Kf, state["running"]


@pytest.mark.parametrize("mode", ["unbiased", "none"])
@pytest.mark.parametrize("split", [False, True])
def test_compute_loss_kernel(split, mode):
    """NeuralEigenfunctions.compute_loss_kernel through BatchL2NormalizedFunctions.forward around the HIP model (16
    input dimensions, a toy Gaussian-kernel operator) against torch autograd in float64. Every call of the model in
    training mode divides by its own batch's norm and updates the running norms, in call order - the operator calls the
    model on x_ref too, so they move twice without split_batch and four times with it. B = 97: halves of 49 / 48 rows,
    B1 + B2 == B on a concatenated (not aliased) phi."""
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.neuralef import NeuralEigenfunctions
    Din, L, B, ell = 16, 6, 97, 4.0
    args = NS(ndim=Din, n_particles=1, use_fourier_feature=True, fourier_mapping_size=12, fourier_scale=0.05,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="24,16", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0)
    torch.manual_seed(4)
    net = get_wavefunctions(args)
    method = NeuralEigenfunctions(net, L, batchnorm_mode=mode, unbiased=True).to(DEV)
    method.train()
    x = torch.randn(B, Din, generator=torch.Generator().manual_seed(3))

    def get_approx_kernel_op(x_ref):
        def op(m, xe, importance=None):
            f = m(xe)
            with torch.no_grad():
                Kmat = torch.exp(-torch.cdist(xe.double(), x_ref.double()) ** 2 / (2.0 * ell ** 2))
                Kf = (Kmat @ m(x_ref).double() / x_ref.shape[0]).float()
            return Kf, f
        return op

    loss, aux = method.compute_loss_kernel(get_approx_kernel_op, x.to(DEV), None, split_batch=split)
    loss.backward()

    p64 = O.Params([w.detach().double().cpu().requires_grad_(True) for w in net.base.ws],
                   [b.detach().double().cpu().requires_grad_(True) for b in net.base.bs],
                   net.base.feature_map._B.detach().double().cpu())
    lwant, f, Kf, running = kernel_loss_oracle(p64, x.double(), split, mode, ell)
    for t in (lwant, f, Kf):
        assert bool(torch.isfinite(t).all())
    errs = dict(loss=rel(loss, lwant), f=rel(aux["f"], f), Tf=rel(aux["Tf"], Kf))
    for i, (t, t64) in enumerate(zip(list(net.base.ws) + list(net.base.bs), p64.trainable())):
        errs[f"grad{i}"] = rel(t.grad, t64.grad)
    if mode != "none":
        errs["norm_biased"] = rel(method.model._norm_biased, running[0])
        errs["norm_unbiased"] = rel(method.model._norm_unbiased, running[1])
    print(f"compute_loss_kernel split={split} {mode}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert tuple(aux["f"].shape) == tuple(aux["Tf"].shape) == (B, L)
    for k, v in errs.items():
        assert v < 1e-4, (k, v)
