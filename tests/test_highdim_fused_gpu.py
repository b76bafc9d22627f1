"""The MFMA forward in split form above the small stencil (5 <= D <= 12, 128-wide hidden layers, finite-difference mode,
on explicit request: path="fused"): D direction groups of the E = 3 split instance, then the direction-loop epilogue
kernel on the raw head outputs. f and Tf against the float64 restatement at the bounds of tests/test_highdim_gpu.py
(2e-5, 1e-4) and against the generic kernels on the same inputs (both are within those bounds of float64, so within
their sum of each other: 4e-5, 2e-4); the backward after a fused forward against the oracle's gradients (3e-5, and 3e-5
against the generic path's as test_hip_parity.test_backward_split_k_matches_oracle holds them)."""
import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _highdim_oracle as HO
from tests import test_highdim_gpu as TG

pytestmark = pytest.mark.gpu

PI32 = TG.PI32
rel = TG.rel


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import hip_ops
    TG.H = hip_ops
    TG.TB.H = hip_ops
    yield


def _problem(D):
    if D == 5:
        return None, HO.Problem(potential=HO.POT_COSINE, pot_coef=HO.COSINE_CS[5], op_scale=1.0, op_shift=10.0, eps=0.01,
                                sigma=PI32, importance=HO.IMP_UNIFORM, hard_mul_const=0.9)
    cfg = dict(problem="sch", potential_type="quantum_chemistry", mol_name="H2" if D == 6 else "LiH", ndim=3,
               laplacian_eps=0.01, operator_scale=1.0, operator_shift=0.0, sampling_scale=2.0, hard_mul_const=1.0,
               sampling_mode="gaussian")
    return 4.0, HO.problem_of(cfg)


# (D, L, B): three dimensions; B = 96: three sample tiles; L = 3 at D = 12: a grid that is no multiple of the XCD count
@pytest.mark.parametrize("D,L,B", [(5, 2, 64), (6, 2, 64), (12, 2, 64), (6, 2, 96), (12, 3, 64)])
def test_split_form_above_four_dimensions(D, L, B):
    H = TG.H
    mask_init, prob = _problem(D)
    p = O.init_params(L, D, 64, (128, 128), 0.2, exp_mask_init=mask_init, seed=44)
    g = torch.Generator().manual_seed(9)
    if prob.importance == HO.IMP_UNIFORM:
        x = (PI32 * (2 * torch.rand(B, D, generator=g) - 1)).float()
        x[0] = 0.0
        x[1] = PI32
    else:
        x = (2.0 * torch.randn(B, D, generator=g)).float()
    shape = TG.shape_of(p, prob)
    hp = TG.hip_problem(prob, D)
    assert H.path_name(shape, B, H.PATH_FUSED, hp) == "fused_mfma"
    assert H.path_name(shape, B, H.PATH_AUTO, hp) == "generic"          # auto stays generic: not measured yet
    assert H.path_name(shape, B, H.PATH_FUSED_BF16X3, hp) == "unsupported"
    v, M = O.sequential_nesting_masks(L)
    ref = HO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
    r = TG.run_hip(p, prob, x, v, M, H.PATH_FUSED, df_override=ref["df"])
    assert r["path"] == "fused_mfma"
    TG.check_rows(r, ref["f"], ref["Tf"], x, prob, f"fused D{D}/L{L}/B{B}")
    gen = TG.run_hip(p, prob, x, v, M, H.PATH_GENERIC, df_override=ref["df"])
    ef, eT = rel(r["f"], gen["f"]), rel(r["Tf"], gen["Tf"])
    print(f"fused against generic D{D}/L{L}/B{B}: f {ef:.2e} Tf {eT:.2e}")
    assert ef < 4e-5 and eT < 2e-4
    for i, (a, b, c) in enumerate(zip(r["grads"], ref["grads"], gen["grads"])):
        assert torch.isfinite(a).all(), i
        assert rel(a.view(-1), b.reshape(-1)) < 3e-5, (i, rel(a.view(-1), b.reshape(-1)))
        assert rel(a, c) < 3e-5, i
    # refused: the exact-Laplacian mode and the bf16x3 forward
    import dataclasses
    with pytest.raises(H.NsvdError, match="unsupported"):
        TG.run_hip(p, dataclasses.replace(prob, eps=0.0), x, v, M, H.PATH_FUSED)
    with pytest.raises(H.NsvdError, match="unsupported"):
        TG.run_hip(p, prob, x, v, M, H.PATH_FUSED_BF16X3)


def test_graphed_steps_on_the_split_form():
    """FusedTrainer on path="fused" at D = 5 (cosine, uniform device sampler above four dimensions, device-resident
    schedule): capture_graph against the same number of eager steps, equal bits; every batch inside [-pi, pi]^5"""
    from neural_svd_amd.trainer import FusedTrainer
    H = TG.H
    D = 5
    shape = H.ModelShape(L=2, D=D, m=64, hidden=(128, 128))
    table = torch.tensor(HO.COSINE_CS[5], dtype=torch.float32, device=TG.DEV)
    prob = H.make_problem(H.POT_COSINE, 0.0, 0.01, 1.0, 10.0, PI32, importance_kind=H.IMP_UNIFORM, pot_table=table)
    assert H.path_name(shape, 64, H.PATH_FUSED, prob) == "fused_mfma"

    def make(sched):
        return FusedTrainer(shape, prob, 64, sequential=True, lr=1e-3, num_iters=60, seed=4, device=TG.DEV,
                            sampling_scale=PI32, fourier_scale=0.1, device_schedule=sched, path=H.PATH_FUSED)
    a, g = make(False), make(True)
    assert not a.guest_features and not g.guest_features  # (the next-batch guest features stay D <= 3)
    gs = g.capture_graph(2)
    gs.replay(3)
    for _ in range(g.t):
        a.step()
        assert float(a.x.abs().max()) < PI32
    torch.cuda.synchronize()
    assert g.t == 6
    for name in ("flat", "sq", "ema"):
        assert torch.equal(getattr(a.P, name), getattr(g.P, name)), name
    assert torch.equal(a.x, g.x) and torch.equal(a.f, g.f) and torch.equal(a.Tf, g.Tf)
    assert bool(torch.isfinite(a.P.flat).all()) and float(a.f.abs().max()) > 0
