"""Cosine, H2+, 3-D hydrogen and Fokker-Planck problems on the CPU: the float64 restatement (tests/_periodic_oracle.py)
against the reference's own float64 run (tests/golden/periodic.npz, made by tests/golden/make_golden_periodic.py),
get_problem's four new branches, Hydrogen3D, and the refusals."""
import argparse
import ast
import os

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _periodic_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "periodic.npz")
CASES = ("cos_2d", "cos_1d", "cos_2d_exact", "fp_2d", "fp_2d_eps01", "fp_1d", "fp_2d_expmask", "h2p_2d", "h2p_3d_exact",
         "hyd_3d")
NSTEPS = {"cos_2d": 3, "fp_2d": 3}


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def case_setup(z, name, dtype=torch.float64):
    cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
    names = [str(n) for n in z[f"{name}_param_names"]]
    t = lambda n: torch.tensor(z[f"{name}_param0_{n}"], dtype=dtype)  # noqa: E731
    ws = [t(n) for n in names if ".ws." in n]
    bs = [t(n) for n in names if ".bs." in n]
    sc = [t(n) for n in names if n.endswith("scales")]
    p = O.Params(ws, bs, torch.tensor(z[f"{name}_fourier_B"], dtype=dtype), sc[0] if sc else None)
    return cfg, names, p, PO.problem_of(cfg)


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a), dtype=torch.float64), torch.as_tensor(np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_float64(z, name):
    """the float64 bounds of test_box_oracle.py"""
    cfg, names, p, prob = case_setup(z, name)
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    sq = [torch.zeros_like(t) for t in p.trainable()]
    nsteps = NSTEPS.get(name, 2)
    for it in range(nsteps):
        x = torch.tensor(z[f"{name}_x"][it], dtype=torch.float64)
        r = PO.loss_and_grads(x, p, prob, v, M)
        pre = f"{name}_f64_step{it}_"
        scale = float((r["f"] * r["Tf"]).abs().sum()) / x.shape[0]
        assert abs(float(r["loss"]) - float(z[pre + "loss"])) < 1e-9 * scale
        assert rel(r["f"], z[pre + "f"]) < 1e-9
        assert rel(r["Tf"], z[pre + "Tf"]) < 1e-9
        for n, g in zip(names, r["grads"]):
            assert rel(g, z[pre + f"grad_{n}"]) < 1e-9, n
        lr = O.cosine_lr(cfg["lr"], it, cfg["num_iters"])
        O.rmsprop_step(p.trainable(), r["grads"], sq, lr, cfg["rmsprop_decay"], 1e-10)  # (in place)
    if name in NSTEPS:
        for n, t in zip(names, p.trainable()):
            assert rel(t, z[f"{name}_f64_step{nsteps - 1}_param_{n}"]) < 1e-9, n
        grid = torch.tensor(z[f"{name}_val_data"], dtype=torch.float64)
        s = PO.spectrum_evd(grid, p, prob, cfg["lim"])
        # (the reference's validation density 1 / (2 lim)^D is a float32 value even in its float64 run: 1e-8)
        assert rel(s["norms"], z[f"{name}_f64_spec_norms"]) < 1e-7
        assert rel(s["eigvals"], z[f"{name}_f64_spec_eigvals"]) < 1e-9


def test_coefficients_are_float32_roundings(z):
    """torch.tensor(cs) is float32 in the reference: with the float64 literals instead the restatement misses the
    fixture (1.6e-8 on V), with their float32 roundings it meets it"""
    cfg, names, p, prob = case_setup(z, "cos_2d")
    x = torch.tensor(z["cos_2d_x"][0], dtype=torch.float64)
    cs64 = torch.tensor(prob.pot_coef, dtype=torch.float64).view(1, -1)
    d = ((torch.cos(x) * cs64).sum(-1, keepdim=True) - PO.potential(x, prob)).abs().max()
    assert 1e-9 < float(d) < 1e-7


@pytest.mark.parametrize("name", ("cos_2d", "fp_2d", "fp_2d_eps01", "fp_2d_expmask"))
def test_planted_rows_periodic(z, name):
    """rows 0-9 sit on x_d in {0, pi/2, pi, -pi} (float32 values): sin or cos of a coordinate vanishes there"""
    x = z[f"{name}_x"]
    vals = np.array([0.0, np.float32(np.pi / 2), np.float32(np.pi), -np.float32(np.pi)], dtype=np.float32)
    assert x.dtype == np.float32
    for it in range(x.shape[0]):
        for j, v in enumerate(vals):
            assert x[it, 2 * j, 0] == v and x[it, 2 * j + 1, -1] == v
        assert np.all(x[it, 8] == vals[2]) and x[it, 9, 0] == 0 and x[it, 9, -1] == vals[1]
        assert np.all(np.isfinite(z[f"{name}_f64_step{it}_Tf"]))


@pytest.mark.parametrize("name", ("h2p_2d", "h2p_3d_exact"))
def test_planted_rows_h2p(z, name):
    """rows 0-3 lie 1e-3 and eps / 2 (5e-3 in exact mode) from a nucleus, none on one"""
    cfg, names, p, prob = case_setup(z, name)
    near = float(np.float32(cfg["laplacian_eps"])) / 2 if cfg["laplacian_eps"] > 0 else 5e-3
    for it in range(z[f"{name}_x"].shape[0]):
        x = torch.tensor(z[f"{name}_x"][it], dtype=torch.float64)
        e = torch.zeros(x.shape[1], dtype=torch.float64)
        e[-1] = 1.0
        R = prob.pot_coef[0]
        dist = torch.minimum((x - R * e).norm(dim=1), (x + R * e).norm(dim=1))
        assert torch.allclose(dist[:4], torch.tensor([1e-3, 1e-3, near, near], dtype=torch.float64), rtol=1e-4)
        assert bool((dist > 0).all()) and bool(PO.nucleus_rows(x, prob)[:4].all())
        assert np.all(np.isfinite(z[f"{name}_f64_step{it}_Tf"]))


def _args(cfg, **over):
    a = argparse.Namespace(**dict(cfg, **over))
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    return a


@pytest.mark.parametrize("name", CASES)
def test_get_problem_branches(z, name):
    """every new branch of get_problem: operator class, potential kind and coefficients, ground truth == the fixture's"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.operators import NegativeHamiltonian, NegativeLinearFokkerPlanck, get_problem
    cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
    op, gt = get_problem(_args(cfg))
    prob = PO.problem_of(cfg)
    inner = op.operator
    assert inner.potential_kind == prob.potential
    assert tuple(inner.potential_coef) == tuple(prob.pot_coef)
    assert inner.laplacian_eps == cfg["laplacian_eps"] and op.scale == cfg["operator_scale"]
    assert op.shift == cfg["operator_shift"]
    if cfg["problem"] == "fp":
        assert isinstance(inner, NegativeLinearFokkerPlanck) and op.fokker_planck
        assert inner.scale == cfg["scale_operator"] == 0.5
    else:
        assert isinstance(inner, NegativeHamiltonian) and not op.fokker_planck
        assert inner.potential_param == prob.charge_or_k or prob.potential == H.POT_COSINE
    if f"{name}_gt" in z.files:
        np.testing.assert_allclose(gt, z[f"{name}_gt"], rtol=1e-14, atol=0)
    else:
        assert gt is None
    assert (f"{name}_gt" in z.files) == (name not in ("cos_1d", "h2p_2d", "h2p_3d_exact"))


def test_cosine_table_and_hydrogen3d_quirk(z):
    from neural_svd_amd.operators import Hydrogen3D, get_problem
    cfg = ast.literal_eval(str(z["cos_2d_cfg"]))
    _, gt = get_problem(_args(cfg, neigs=25))
    np.testing.assert_allclose(gt, z["cos_2d_gt25"], rtol=1e-14)
    assert len(gt) == 25 and bool((gt > 0).all())  # (shift 10: every tabulated eigenvalue of -H + shift is positive)
    for n in (1, 5, 6, 14, 16, 30):
        want = z[f"hydrogen3d_eigvals_{n}"]
        np.testing.assert_allclose(Hydrogen3D(charge=1.0).get_eigvals(n), want, rtol=1e-14)
        np.testing.assert_allclose(PO.hydrogen3d_eigvals(n), want, rtol=1e-14)
    assert len(Hydrogen3D().get_eigvals(16)) == 14 and len(Hydrogen3D().get_eigvals(6)) == 5  # the short lists
    np.testing.assert_allclose(Hydrogen3D(charge=2.0).get_eigvals(5), [-1.0, -0.25, -0.25, -0.25, -0.25])


def test_renamed_arguments(z):
    """args.use_gaussian_sampling is read as sampling_mode == 'gaussian', args.scale_operator with default 1.0: the
    argument set of main_pde.py's parser (neither name defined) is accepted"""
    from neural_svd_amd.operators import get_problem
    for name in ("cos_2d", "fp_2d"):
        cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
        del cfg["use_gaussian_sampling"], cfg["scale_operator"]
        op, _ = get_problem(_args(cfg))
        if name == "fp_2d":
            assert op.operator.scale == 1.0
        with pytest.raises(AssertionError, match="Gaussian sampler"):
            get_problem(_args(cfg, sampling_mode="gaussian"))


def test_refusals(z):
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.operators import (GaussianImportance, NegativeHamiltonian, NegativeLinearFokkerPlanck,
                                          OperatorWrapper, UniformImportance, get_problem, sin_of_cos_potential)
    from functools import partial
    for name in ("cos_2d", "fp_2d"):
        cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
        for over in (dict(lim=5.0), dict(apply_boundary=1), dict(use_fourier_feature=False),
                     dict(fourier_deterministic=False), dict(ndim=3)):
            with pytest.raises(AssertionError):  # the reference's asserts
                get_problem(_args(cfg, **over))
        for nd in (5, 10):  # valid in the reference, beyond the stencil here: said so
            with pytest.raises(NotImplementedError, match="at most 4 input dimensions"):
                get_problem(_args(cfg, ndim=nd))
    cfg = ast.literal_eval(str(z["cos_2d_cfg"]))
    with pytest.raises(AssertionError, match="25"):
        get_problem(_args(cfg, neigs=26))
    with pytest.raises(NotImplementedError):
        get_problem(_args(cfg, potential_type="quantum_chemistry"))
    with pytest.raises(NotImplementedError):
        get_problem(_args(cfg, problem="heat"))
    with pytest.raises(NotImplementedError, match="laplacian_eps > 0"):  # no exact-Laplacian Fokker-Planck
        get_problem(_args(ast.literal_eval(str(z["fp_2d_cfg"])), laplacian_eps=0.0))
    with pytest.raises(NsvdError):
        NegativeHamiltonian(partial(sin_of_cos_potential, cs=[1.0, 1.0]))
    fp = OperatorWrapper(NegativeLinearFokkerPlanck(partial(sin_of_cos_potential, cs=[1.0, 1.0]), 1.0, 0.01))
    assert fp.fused(UniformImportance(np.pi, 2)) and fp.fused(None) and not fp.fused(GaussianImportance(1.0, 2))


def test_path_name_for_new_problems():
    """host-side query, no GPU: 'invalid' for unknown values, 'unsupported' for the Fokker-Planck kind outside what the
    epilogue implements"""
    from neural_svd_amd import hip_ops as H
    gen = H.ModelShape(L=4, D=2, m=8, hidden=(16, 16))
    mfma = H.ModelShape(L=4, D=2, m=64, hidden=(128, 128, 128))
    box = H.ModelShape(L=4, D=2, m=8, hidden=(16, 16), box_mask=H.BOX_EXP, box_lim=float(np.pi))
    fp = dict(operator_kind=H.OP_FOKKER_PLANCK, fp_scale=1.0, pot_coef=(1.0, 1.0))

    def name(shape, pot, eps=0.01, imp=H.IMP_UNIFORM, sigma=float(np.pi), B=64, **kw):
        prob = H.make_problem(pot, 1.0, eps, 1.0, 0.0, sigma, importance_kind=imp, **kw)
        return H.path_name(shape, B, H.PATH_AUTO, prob)

    assert name(gen, H.POT_SIN_OF_COS, **fp) == "generic" and name(mfma, H.POT_SIN_OF_COS, **fp) == "fused_mfma"
    assert name(gen, H.POT_SIN_OF_COS, imp=H.IMP_NONE, **fp) == "generic"
    assert name(mfma, H.POT_COSINE, pot_coef=(0.8, 0.9)) == "fused_mfma"
    assert name(mfma, H.POT_COSINE, eps=0.0, pot_coef=(0.8, 0.9)) == "fused_mfma"
    assert name(mfma, H.POT_H2_ION, imp=H.IMP_GAUSSIAN, pot_coef=(1.0,)) == "fused_mfma"
    assert name(gen, H.POT_SIN_OF_COS, pot_coef=(1.0, 1.0)) == "invalid"        # sin-of-cos outside Fokker-Planck
    assert name(gen, 6) == "invalid" and name(gen, H.POT_COSINE, operator_kind=2) == "invalid"
    assert name(mfma, H.POT_SIN_OF_COS, eps=0.0, **fp) == "unsupported"         # no exact-Laplacian mode
    assert name(mfma, H.POT_SIN_OF_COS, imp=H.IMP_GAUSSIAN, **fp) == "unsupported"
    assert name(box, H.POT_SIN_OF_COS, **fp) == "unsupported"                    # box mask
    assert name(gen, H.POT_SIN_OF_COS, sigma=1e6, **fp) == "unsupported"        # sqrt p = 1 / (2e6) < 1e-5
    assert name(gen, H.POT_COSINE, **dict(fp, pot_coef=(0.8, 0.9))) == "unsupported"  # another potential
    # all-zero appended fields: the problems of ABI 3, unchanged
    old = H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, 16.0)
    assert old.operator_kind == 0 and old.fp_scale == 0.0 and list(old.pot_coef) == [0.0] * 4
    with pytest.raises(Exception, match="at most 4"):
        H.make_problem(H.POT_COSINE, 0.0, 0.01, 1.0, 0.0, 1.0, pot_coef=(1.0,) * 5)
    p = H.make_problem(H.POT_COSINE, 0.0, 0.01, 1.0, 0.0, 1.0, pot_coef=(0.814723686393179,))
    assert p.pot_coef[0] == float(np.float32(0.814723686393179))  # the float32 rounding, as torch.tensor(cs)


def test_torch_potentials_match_restatement(z):
    """the torch forms serving apply_stencil and foreign callers are the reference's expressions"""
    from neural_svd_amd.operators import cosine_potential, hydrogen_mol_ion_potential, sin_of_cos_potential
    x = torch.tensor(z["cos_2d_x"][0], dtype=torch.float64)
    cs = PO.COSINE_CS[2]
    assert torch.equal(cosine_potential(x.view(-1, 1, 2), list(cs)),
                       PO.potential(x, PO.Problem(potential=PO.POT_COSINE, pot_coef=cs)).view(-1))
    assert torch.equal(sin_of_cos_potential(x, [1.0, 1.0]),
                       PO.potential(x, PO.Problem(potential=PO.POT_SIN_OF_COS, pot_coef=(1.0, 1.0))).view(-1))
    xh = torch.tensor(z["h2p_2d_x"][0], dtype=torch.float64)
    want = PO.potential(xh, PO.Problem(potential=PO.POT_H2_ION, charge_or_k=2.0, pot_coef=(1.0,)))
    assert torch.allclose(hydrogen_mol_ion_potential(xh, R=1.0, charge=2.0), want, rtol=1e-15, atol=0)


def test_apply_stencil_fokker_planck_matches_restatement(z):
    """OperatorWrapper.apply_stencil's Fokker-Planck op sequence (the path for densities the kernel does not carry),
    run on the CPU in float64 around the restatement's model"""
    from functools import partial
    from neural_svd_amd.operators import NegativeLinearFokkerPlanck, OperatorWrapper, sin_of_cos_potential
    cfg, names, p, prob = case_setup(z, "fp_2d")
    x = torch.tensor(z["fp_2d_x"][0], dtype=torch.float64)
    from tests import _box_oracle as BO
    op = OperatorWrapper(NegativeLinearFokkerPlanck(partial(sin_of_cos_potential, cs=[1.0, 1.0]), cfg["scale_operator"],
                                                    float(np.float32(cfg["laplacian_eps"]))),
                         scale=cfg["operator_scale"], shift=cfg["operator_shift"])

    class Imp:
        def __call__(self, t):
            return BO.sqrt_importance(t.double(), prob) ** 2

    # (apply_stencil casts x to float32 - the rows are float32 values - and shifts by a float32 eps: the model below
    # lifts every stencil point back to float64, so its run differs from the restatement by rounding alone)
    Tf, f = op.apply_stencil(lambda t: BO.wave(t.double(), p, prob), x, Imp())
    c = PO.operator_forward(x, p, prob)
    assert rel(f, c.f) < 1e-12
    assert rel(Tf, c.Tf) < 1e-3  # float32 stencil points: x + eps rounds to float32 (1e-7 / eps^2 on the Laplacian)
