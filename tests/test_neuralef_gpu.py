"""NeuralEF on the HIP kernels against the float64 restatement (tests/_neuralef_oracle.py) and the reference's own
float64 run (tests/golden/neuralef.npz): the loss kernel alone, the whole training step at the scripts' shapes on the
MFMA and the generic path, bit-for-bit reproducibility, and the drop-in loop (graph-replayed steps, evaluation,
checkpoints)."""
import argparse
import os
from functools import partial

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _neuralef_oracle as NO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neuralef.npz")


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------ loss kernel
@pytest.mark.parametrize("L", [16, 36, 55, 64])
@pytest.mark.parametrize("B", [512, 513, 8192])
def test_loss_kernel(L, B):
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(L * 7 + B)
    phi = torch.randn(B, L, generator=g, dtype=torch.float64)
    Tphi = torch.randn(B, L, generator=g, dtype=torch.float64) * 3.0 + phi
    pd, Td = phi.float().to(DEV), Tphi.float().to(DEV)
    # the loss is a difference of its terms (with diagonal 0 the biased form cancels to a few per mille of them): its
    # error is measured against their size
    scale = float((pd.double() * Td.double()).abs().sum()) / B

    def close(loss, want):
        return abs(float(loss) - float(want)) < 1e-5 * scale
    p1, p2 = torch.chunk(pd, 2)
    t1, t2 = torch.chunk(Td, 2)
    for unbiased in (0, 1):
        for diag in (0, 1):
            want, dwant, _, _ = NO.loss_and_dphi(pd.double().cpu(), Td.double().cpu(), unbiased, diag)
            loss, dphi, d1, d2 = H.nef_loss(pd, Td, p1, t1, p2, t2, unbiased, diag)
            assert d1 is None and d2 is None
            assert close(loss[0], want), (unbiased, diag)
            assert rel(dphi, dwant) < 1e-5, (unbiased, diag)
    # independent halves (compute_loss_kernel(split_batch=False) passes phi three times)
    for unbiased in (0, 1):
        want, dv, w1, w2 = NO.loss_and_dphi(pd.double().cpu(), Td.double().cpu(), unbiased, 1, pd.double().cpu(),
                                            Td.double().cpu(), pd.double().cpu(), Td.double().cpu())
        loss, dphi, d1, d2 = H.nef_loss(pd, Td, pd, Td, pd, Td, unbiased, 1)
        assert close(loss[0], want)
        assert rel(dphi, dv) < 1e-5 and rel(d1, w1) < 1e-5 and rel(d2, w2) < 1e-5


# ------------------------------------------------------------------------------------------------ full shapes
def build_model(p: O.Params, hidden, fourier_scale=1.0):
    from neural_svd_amd.models import ExponentialMask, GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    L, (D, m) = p.ws[0].shape[0], p.fourier_B.shape
    fm = GaussianFourierFeatureTransform(D, mapping_size=m, scale=fourier_scale)
    fm._B.data = p.fourier_B.float().clone()
    base = ParallelMLP(D, list(hidden), 1, L, "softplus", bias=True, feature_map=fm)
    for w, w0 in zip(base.ws, p.ws):
        w.data = w0.float().clone()
    for b, b0 in zip(base.bs, p.bs):
        b.data = b0.float().clone()
    if p.scales is not None:
        mask = ExponentialMask(L, init_scale=1.0)
        mask.scales.data = p.scales.float().clone()
    else:
        mask = lambda x: 1.0  # noqa: E731
    return WaveFunctions(base, mask).to(DEV)


def problem(kind):
    from neural_svd_amd.operators import (GaussianImportance, NegativeHamiltonian, OperatorWrapper,
                                          harmonic_oscillator_potential, hydrogen_potential)
    if kind == "hydrogen":
        po = O.Problem(potential=O.POT_HYDROGEN, charge_or_k=1.0, eps=0.01, op_scale=100.0, op_shift=0.0, sigma=16.0)
        ham = NegativeHamiltonian(partial(hydrogen_potential, charge=1.0), 1.0, 0.01)
        return po, OperatorWrapper(ham, 100.0, 0.0), GaussianImportance(16.0, 2)
    po = O.Problem(potential=O.POT_HARMONIC, charge_or_k=1.0, eps=0.01, op_scale=1.0, op_shift=16.0, sigma=4.0)
    ham = NegativeHamiltonian(partial(harmonic_oscillator_potential, k=1.0), 1.0, 0.01)
    return po, OperatorWrapper(ham, 1.0, 16.0), GaussianImportance(4.0, 2)


SHAPES = dict(
    hydrogen=dict(L=16, B=512, m=1024, hidden=(128, 128, 128), fs=0.1, mask=None),
    oscillator=dict(L=55, B=512, m=256, hidden=(128, 128, 128), fs=1.0, mask=10.0),
)


def neuralef(model, L, path, mode="unbiased", unbiased=1):
    from neural_svd_amd.neuralef import NeuralEigenfunctions
    return NeuralEigenfunctions(model, L, batchnorm_mode=mode, unbiased=unbiased, path=path).to(DEV)


def gpu_step(method, op, imp, x):
    method.train()
    for t in method.parameters():
        t.grad = None
    loss, aux = method.compute_loss_operator(op, x, importance=imp)
    loss.backward()
    return loss.detach(), aux["f"].detach(), aux["Tf"].detach(), [t.grad for t in method.model.base_model.trainable_tensors()]


@pytest.mark.parametrize("kind", ["hydrogen", "oscillator"])
@pytest.mark.parametrize("pathname", ["auto", "generic"])
def test_full_step_against_float64(kind, pathname):
    from neural_svd_amd import hip_ops as H
    s = SHAPES[kind]
    path = {"auto": H.PATH_AUTO, "generic": H.PATH_GENERIC}[pathname]
    p = O.init_params(s["L"], 2, s["m"], s["hidden"], s["fs"], s["mask"], seed=11)
    po, op, imp = problem(kind)
    model = build_model(p, s["hidden"], s["fs"])
    shape = model.shape
    assert H.path_name(shape, s["B"], path) == ("generic" if pathname == "generic" else "fused_mfma")
    method = neuralef(model, s["L"], path)
    p64 = p.to(torch.float64)
    running = [None, None, False]
    g = torch.Generator().manual_seed(5)
    for it in range(2):  # the second call exercises the running norms' EMA branch
        x = po.sigma * torch.randn(s["B"], 2, generator=g)
        loss, phi, Tphi, grads = gpu_step(method, op, imp, x.to(DEV))
        fwd, lwant, gwant = NO.train_step(x.double(), p64, po, running, 1)
        running = fwd["running"]
        assert rel(phi, fwd["phi"]) < 2e-5
        assert rel(Tphi, fwd["Tphi"]) < 1e-4
        assert rel(method.model._norm_biased, running[0]) < 2e-5
        assert rel(method.model._norm_unbiased, running[1]) < 2e-5
        assert rel(loss, lwant) < 1e-4
        for got, want in zip(grads, gwant):
            assert rel(got, want) < 1e-4


def test_reference_fixture():
    """float32 on the GPU against the reference's float64 run, first step of every case (both forms, both modes and
    'none', the mask, an odd batch)"""
    from tests.test_neuralef_oracle import CASES, case_setup
    from neural_svd_amd.operators import GaussianImportance, NegativeHamiltonian, OperatorWrapper
    from neural_svd_amd.operators import harmonic_oscillator_potential, hydrogen_potential
    z = np.load(GOLDEN)
    for name in CASES:
        cfg, unbiased, mode, names, p, po = case_setup(z, name)
        hidden = [int(h) for h in cfg["mlp_hidden_dims"].split(",")]
        model = build_model(p, hidden)
        model.hard_mul_const = cfg["hard_mul_const"]
        method = neuralef(model, len(p.ws[0]), 0, {0: "none", 1: "biased", 2: "unbiased"}[mode], unbiased)
        pot = partial(harmonic_oscillator_potential, k=1.0) if po.potential == O.POT_HARMONIC else \
            partial(hydrogen_potential, charge=cfg["charge"])
        op = OperatorWrapper(NegativeHamiltonian(pot, 1.0, cfg["laplacian_eps"]), cfg["operator_scale"],
                             cfg["operator_shift"])
        x = torch.tensor(z[f"{name}_x"][0], dtype=torch.float32, device=DEV)
        method.train()
        loss, aux = method.compute_loss_operator(op, x, importance=GaussianImportance(cfg["sampling_scale"], 2))
        loss.backward()
        pre = f"{name}_f64_step0_"
        assert rel(aux["f"], z[pre + "phi"]) < 1e-4, name
        assert rel(aux["Tf"], z[pre + "Tphi"]) < 1e-4, name
        assert rel(loss, z[pre + "loss"]) < 1e-4, name
        for n, t in zip(names, model.trainable_tensors()):
            assert rel(t.grad, z[pre + f"grad_{n}"]) < 1e-4, (name, n)
        if mode:
            assert rel(method.model._norm_biased, z[pre + "norm_biased"]) < 1e-4, name
            assert rel(method.model._norm_unbiased, z[pre + "norm_unbiased"]) < 1e-4, name


def test_reproducible_bits():
    s = SHAPES["hydrogen"]
    p = O.init_params(s["L"], 2, s["m"], s["hidden"], s["fs"], None, seed=3)
    po, op, imp = problem("hydrogen")
    x = (16.0 * torch.randn(s["B"], 2, generator=torch.Generator().manual_seed(1))).to(DEV)
    outs = []
    for _ in range(2):
        method = neuralef(build_model(p, s["hidden"], s["fs"]), s["L"], 0)
        loss, phi, Tphi, grads = gpu_step(method, op, imp, x)
        outs.append([loss, phi, Tphi, method.model._norm_biased.data.clone(), *grads])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ drop-in loop
def dropin_args(steps, log_dir=None):
    a = argparse.Namespace(
        problem="sch", potential_type="hydrogen", charge=1.0, ndim=2, n_particles=1, neigs=16, laplacian_eps=0.01,
        operator_scale=100.0, operator_shift=0.0, sampling_mode="gaussian", sampling_scale=16.0, batch_size=512,
        lim=50.0, val_eps=2.0, use_fourier_feature=True, fourier_mapping_size=1024, fourier_scale=0.1,
        fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="128,128,128", parallel=1,
        nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
        sort=0, optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0, adam_eps=1e-7, num_iters=steps,
        ema_decay=0.995, use_lr_scheduler=True, print_freq=10 ** 9, eval_freq=steps, log_dir=log_dir)
    a.loss = argparse.Namespace(name="neuralef", neuralef=argparse.Namespace(unbiased=1, batchnorm_mode="unbiased"),
                                neuralsvd=argparse.Namespace(step=1, sequential=0))
    return a


def run_dropin(steps, monkeypatch, warmup=None, log_dir=None):
    from neural_svd_amd import drop_in
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    from neural_svd_amd.operators import get_dataloader, get_problem
    if warmup is not None:
        monkeypatch.setattr(drop_in.CapturedPlainStep, "WARMUP", warmup)
    seen = {}
    real = drop_in.compute_spectrum_evd

    def spy(*a, **k):
        seen["normalize"] = k.get("normalize")
        return real(*a, **k)
    monkeypatch.setattr(drop_in, "compute_spectrum_evd", spy)
    a = dropin_args(steps, log_dir)
    torch.manual_seed(0)
    operator, gt = get_problem(a, DEV)
    model = get_wavefunctions(a)
    make_batch, val_data, batch_ftn_val, imp_train, imp_val = get_dataloader(a, DEV)
    method = get_evd_method(a, "neuralef", model).to(DEV)
    eigs, norms = drop_in.train_operator(a, method, operator, make_batch, val_data, batch_ftn_val, None, None, DEV,
                                         imp_train, imp_val, ground_truth_spectrum=gt)
    torch.cuda.synchronize()
    return method, eigs, seen


def test_dropin_graph_replay_matches_eager(monkeypatch, tmp_path):
    steps = 6  # 3 eager warm-up steps (the first initialises the running norms), then 3 graph replays
    m_graph, eigs, seen = run_dropin(steps, monkeypatch, log_dir=str(tmp_path))
    m_eager, _, _ = run_dropin(steps, monkeypatch, warmup=100)
    sd_g, sd_e = m_graph.state_dict(), m_eager.state_dict()
    for k in sd_g:
        assert torch.equal(sd_g[k], sd_e[k]), k
    assert seen["normalize"] is False  # reference examples/operator/__init__.py:110
    assert len(eigs) == 1 and np.all(np.isfinite(eigs[0]))
    ck = torch.load(os.path.join(str(tmp_path), f"{steps}.pth"), weights_only=False)
    keys = list(ck["method"].keys())
    assert keys[:2] == ["model._norm_biased", "model._norm_unbiased"]
    assert keys[2:] == ["model.base_model.base.feature_map._B"] + [f"model.base_model.base.ws.{i}" for i in range(4)] + \
        [f"model.base_model.base.bs.{i}" for i in range(4)]
