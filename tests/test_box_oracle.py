"""Bounded-domain problems on the CPU: the float64 restatement (tests/_box_oracle.py) against the reference's own
float64 run (tests/golden/box.npz, made by tests/golden/make_golden_box.py), InfiniteWell2D, the drop-in factories'
state_dict layout, and the refusals."""
import argparse
import ast
import os

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box.npz")
CASES = ("iw_sqrt", "iw_exp", "box_expmask", "iw_exact_sqrt", "iw_exact_exp", "iw_1d", "iw_3d_exact")
NSTEPS = 3


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
    return cfg, names, p, BO.problem_of(cfg)


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a), dtype=torch.float64), torch.as_tensor(np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_float64(z, name):
    cfg, names, p, prob = case_setup(z, name)
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    sq = [torch.zeros_like(t) for t in p.trainable()]
    for it in range(NSTEPS):
        x = torch.tensor(z[f"{name}_x"][it], dtype=torch.float64)
        r = BO.loss_and_grads(x, p, prob, v, M)
        pre = f"{name}_f64_step{it}_"
        # (loss: relative to the size of its terms - the loss itself is a difference of them)
        scale = float((r["f"] * r["Tf"]).abs().sum()) / x.shape[0]
        assert abs(float(r["loss"]) - float(z[pre + "loss"])) < 1e-9 * scale
        assert rel(r["f"], z[pre + "f"]) < 1e-9
        assert rel(r["Tf"], z[pre + "Tf"]) < 1e-9
        for n, g in zip(names, r["grads"]):
            assert rel(g, z[pre + f"grad_{n}"]) < 1e-9, n
        lr = O.cosine_lr(cfg["lr"], it, cfg["num_iters"])
        O.rmsprop_step(p.trainable(), r["grads"], sq, lr, cfg["rmsprop_decay"], 1e-10)  # (in place)
    for n, t in zip(names, p.trainable()):
        assert rel(t, z[f"{name}_f64_step{NSTEPS - 1}_param_{n}"]) < 1e-9, n
    if f"{name}_val_data" in z.files:
        grid = torch.tensor(z[f"{name}_val_data"], dtype=torch.float64)
        s = BO.spectrum_evd(grid, p, prob, cfg["lim"])
        # (the reference's validation density 1 / (2 lim)^D is a float32 value even in its float64 run: 1e-8)
        assert rel(s["norms"], z[f"{name}_f64_spec_norms"]) < 1e-7
        assert rel(s["eigvals"], z[f"{name}_f64_spec_eigvals"]) < 1e-9


@pytest.mark.parametrize("name", ("iw_sqrt", "iw_exp", "box_expmask", "iw_1d"))
def test_planted_rows(z, name):
    """the fixture's planted rows: 0-4 are wall rows, row 5 lies far outside and gives f = Tf = 0 exactly"""
    cfg, names, p, prob = case_setup(z, name)
    for it in range(NSTEPS):
        x = torch.tensor(z[f"{name}_x"][it], dtype=torch.float64)
        assert bool(BO.wall_rows(x, prob)[:6].all())
        assert np.all(z[f"{name}_f64_step{it}_f"][5] == 0) and np.all(z[f"{name}_f64_step{it}_Tf"][5] == 0)
        assert np.all(z[f"{name}_f64_step{it}_f"][2] == 0)  # on the wall: f = 0, Tf from the inner neighbour
        assert np.any(z[f"{name}_f64_step{it}_Tf"][2] != 0)
        assert np.all(z[f"{name}_f64_step{it}_f"][3] == 0) and np.any(z[f"{name}_f64_step{it}_Tf"][3] != 0)


def test_infinite_well_ground_truth(z):
    from neural_svd_amd.operators import InfiniteWell2D
    for name in ("iw_sqrt", "iw_exp", "iw_exact_sqrt", "iw_exact_exp"):
        cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
        gt = -InfiniteWell2D(L=2 * cfg["lim"]).get_eigvals(cfg["neigs"])
        np.testing.assert_allclose(cfg["operator_scale"] * gt + cfg["operator_shift"], z[f"{name}_gt"], rtol=1e-14)
        np.testing.assert_allclose(gt, -BO.infinite_well_2d_eigvals(cfg["neigs"], 2 * cfg["lim"]), rtol=1e-14)
    vals = InfiniteWell2D(L=2.0).get_eigvals(7) / (np.pi ** 2 / 4)
    np.testing.assert_allclose(vals, [2, 5, 5, 8, 10, 10, 13], rtol=1e-14)


def _args(cfg):
    a = argparse.Namespace(**cfg)
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    return a


@pytest.mark.parametrize("name", ("iw_sqrt", "iw_exp", "box_expmask", "iw_1d", "iw_3d_exact"))
def test_get_wavefunctions_state_dict_and_shape(z, name):
    """get_wavefunctions honours apply_boundary / boundary_mode; the masks add no state_dict key"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.models import DirichletBoundaryMaskBox, ExponentialMask, get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
    model = get_wavefunctions(_args(cfg))
    assert isinstance(model.box, DirichletBoundaryMaskBox)
    assert isinstance(model.boundary_mask, ExponentialMask) == bool(cfg["apply_exp_mask"])
    sh = model.shape
    assert sh.box_mask == {"dir_box_sqrt": H.BOX_SQRT, "dir_box_exp": H.BOX_EXP}[cfg["boundary_mode"]]
    assert sh.box_lim == cfg["lim"] and sh.has_exp_mask == bool(cfg["apply_exp_mask"]) and sh.D == cfg["ndim"]
    d = sh.desc()
    assert d.box_mask == sh.box_mask and d.box_lim == np.float32(cfg["lim"])
    sd = get_evd_method(_args(cfg), "neuralsvd", model).state_dict()
    assert list(sd.keys()) == [str(k) for k in z[f"{name}_sd_keys"]]
    assert [repr(tuple(v.shape)) for v in sd.values()] == [str(s) for s in z[f"{name}_sd_shapes"]]


def test_torch_mask_forward_matches_oracle():
    """DirichletBoundaryMaskBox.forward (for foreign callers) is the reference's expression"""
    from neural_svd_amd.models import DirichletBoundaryMaskBox, ExponentialMask
    x = torch.tensor([[0.3, -4.99], [5.0, 0.0], [-7.0, 1.0], [4.995, -4.995], [0.0, 0.0]], dtype=torch.float64)
    for mode, kind in (("dir_box_sqrt", BO.BOX_SQRT), ("dir_box_exp", BO.BOX_EXP)):
        box = DirichletBoundaryMaskBox(5.0, mode)
        want = BO.box_mask(x, BO.Problem(box_mode=kind, box_lim=5.0))
        assert torch.equal(box(x), want)
        assert list(box.state_dict().keys()) == []
        em = ExponentialMask(3, init_scale=10.0, boundary_mask=box).double()
        r = x.norm(dim=1, keepdim=True)
        assert torch.allclose(em(x), torch.exp(-r / 10.0) * want, rtol=1e-15, atol=0)
        assert list(em.state_dict().keys()) == ["scales"]


def test_get_problem_and_descriptors(z):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.operators import (OperatorWrapper, UniformImportance, fused_problem_of, get_dataloader,
                                          get_problem, infinite_well_potential)
    cfg = ast.literal_eval(str(z["iw_sqrt_cfg"]))
    a = _args(cfg)
    op, gt = get_problem(a)
    np.testing.assert_allclose(gt, z["iw_sqrt_gt"], rtol=1e-14)
    assert op.operator.potential_kind == H.POT_ZERO
    assert torch.equal(infinite_well_potential(torch.ones(3, 1, 2)), torch.zeros(3))
    _, _, _, imp, _ = get_dataloader(a, "cpu")
    assert isinstance(imp, UniformImportance) and op.fused(imp)
    prob = fused_problem_of(op, imp, get_wavefunctions(a))
    assert prob.use_importance == H.IMP_UNIFORM and prob.sigma == cfg["sampling_scale"] and prob.potential == H.POT_ZERO
    assert H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 1.0, 0.0, 16.0).use_importance == H.IMP_GAUSSIAN
    assert H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 1.0, 0.0, 16.0, use_importance=False).use_importance == H.IMP_NONE
    a.ndim = 3
    with pytest.raises(AssertionError):
        get_problem(a)
    assert isinstance(op, OperatorWrapper)


def test_refusals_name_their_reason(z):
    from neural_svd_amd.drop_in import _refuse_neuralef
    from neural_svd_amd.models import ExponentialMask, WaveFunctions, get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    from neural_svd_amd.operators import get_problem
    cfg = ast.literal_eval(str(z["iw_sqrt_cfg"]))
    a = _args(cfg)
    a.loss = argparse.Namespace(name="neuralef", neuralef=argparse.Namespace(batchnorm_mode="unbiased", unbiased=1),
                                neuralsvd=argparse.Namespace(step=1, sequential=1))
    op, _ = get_problem(a)
    for mode in ("unbiased", "none"):
        a.loss.neuralef.batchnorm_mode = mode
        method = get_evd_method(a, "neuralef", get_wavefunctions(a))
        with pytest.raises(NotImplementedError, match="box mask"):
            _refuse_neuralef(a, method, op)
    a.apply_boundary = 0
    _refuse_neuralef(a, get_evd_method(a, "neuralef", get_wavefunctions(a)), op)  # V = 0 alone is no reason
    with pytest.raises(NotImplementedError, match="DirichletBoundaryMaskBox"):
        ExponentialMask(4, boundary_mask=lambda x: 0.5)
    with pytest.raises(NotImplementedError, match="DirichletBoundaryMaskBox"):
        WaveFunctions(get_wavefunctions(a).base, boundary_mask=lambda x: 0.5)
    a.apply_boundary, a.boundary_mode = 1, "sqrt"  # (the reference's argparse default fails its assert too)
    with pytest.raises(AssertionError):
        get_wavefunctions(a)
    a.boundary_mode, a.potential_type = "dir_box_sqrt", "cosine"
    with pytest.raises(NotImplementedError, match="cosine"):
        get_problem(a)
