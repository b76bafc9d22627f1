"""GPU tests of RadialKernelOperator (neural_svd_amd/kernel_ops.py) behind the kernel-operator interface: the
reference's golden compute_loss_kernel, NeuralEF's compute_loss_kernel, the fused trainer against the module loop,
kernel_spectrum against float64, and the interface's refusals."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _rbf_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().numpy()
    b = np.asarray(torch.as_tensor(b).detach().double().cpu().numpy())
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("case", ["ka", "kb", "kc"])
@pytest.mark.parametrize("split", [False, True])
def test_compute_loss_kernel_matches_reference_golden(case, split):
    """tests/test_kernel_apply_gpu.py's test of the same name with the toy float64 cdist operator replaced by
    RadialKernelOperator(GAUSSIAN, ell) - Kf from nsvd_rbf_apply in float32: loss, f, Kf and every gradient against
    the REFERENCE's float64 values (tests/golden/kernel_loss.npz), same assertions and tolerances."""
    from tests import _golden as G
    from tests.test_dropin_gpu import make_args
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    z = G.load("kernel_loss")
    cfg = G.cfg_of(z, case)
    args = make_args(cfg)
    torch.manual_seed(cfg["seed"])
    method = get_evd_method(args, "neuralsvd", get_wavefunctions(args)).to(DEV)
    ell = float(z[f"{case}_ell"])
    x = torch.tensor(z[f"{case}_x"]).to(DEV)
    op = RadialKernelOperator(H.RBF_GAUSSIAN, ell, x.shape[1], 1.0, DEV)
    loss, aux = method.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
    loss.backward()
    q64, q32 = f"{case}_f64_split{int(split)}_", f"{case}_f32_split{int(split)}_"

    def tol(key, floor):  # a few times the float32 reference's own distance from its float64 self
        return max(4.0 * G.rel(z[q32 + key], z[q64 + key]), floor)
    el = abs(float(loss.detach()) - float(z[q64 + "loss"]))
    print(f"{case} split={split}: loss {el:.2e} f {rel(aux['f'].detach(), torch.tensor(z[q64 + 'f'])):.2e} "
          f"Kf {rel(aux['Tf'].detach(), torch.tensor(z[q64 + 'Kf'])):.2e} (tol {tol('Kf', 2e-6):.2e})")
    assert el < max(4 * abs(float(z[q32 + "loss"]) - float(z[q64 + "loss"])), 2e-6 * abs(float(z[q64 + "loss"])))
    assert rel(aux["f"].detach(), torch.tensor(z[q64 + "f"])) < tol("f", 2e-6)
    assert rel(aux["Tf"].detach(), torch.tensor(z[q64 + "Kf"])) < tol("Kf", 2e-6)
    checked = 0
    for n, t in method.named_parameters():
        if t.grad is None:
            continue
        checked += 1
        if q64 + f"grad_{n}" in z.files:
            assert rel(t.grad.reshape(z[q64 + f"grad_{n}"].shape), torch.tensor(z[q64 + f"grad_{n}"])) < \
                tol(f"grad_{n}", 5e-6), n
        else:
            want = float(z[q64 + f"gradnorm_{n}"])
            assert abs(float(t.grad.double().norm()) - want) < 1e-5 * want, n
            assert rel(t.grad.reshape(-1)[::61], torch.tensor(z[q64 + f"gradsample_{n}"])) < \
                tol(f"gradsample_{n}", 5e-6), n
    assert checked > 0


@pytest.mark.parametrize("split", [False, True])
def test_neuralef_compute_loss_kernel(split):
    """tests/test_neuralef_shapes_gpu.py:test_compute_loss_kernel (mode "unbiased", its shape and bounds) with the
    radial operator in place of the toy float64 one, against that test's float64 autograd oracle."""
    from tests.test_neuralef_shapes_gpu import kernel_loss_oracle
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.neuralef import NeuralEigenfunctions
    Din, L, B, ell, mode = 16, 6, 97, 4.0, "unbiased"
    args = NS(ndim=Din, n_particles=1, use_fourier_feature=True, fourier_mapping_size=12, fourier_scale=0.05,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="24,16", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0)
    torch.manual_seed(4)
    net = get_wavefunctions(args)
    method = NeuralEigenfunctions(net, L, batchnorm_mode=mode, unbiased=True).to(DEV)
    method.train()
    x = torch.randn(B, Din, generator=torch.Generator().manual_seed(3))
    op = RadialKernelOperator(H.RBF_GAUSSIAN, ell, Din, 1.0, DEV)
    loss, aux = method.compute_loss_kernel(op.get_approx_kernel_op, x.to(DEV), None, split_batch=split)
    loss.backward()
    p64 = O.Params([w.detach().double().cpu().requires_grad_(True) for w in net.base.ws],
                   [b.detach().double().cpu().requires_grad_(True) for b in net.base.bs],
                   net.base.feature_map._B.detach().double().cpu())
    lwant, f, Kf, running = kernel_loss_oracle(p64, x.double(), split, mode, ell)
    errs = dict(loss=rel(loss, lwant), f=rel(aux["f"], f), Tf=rel(aux["Tf"], Kf))
    for i, (t, t64) in enumerate(zip(list(net.base.ws) + list(net.base.bs), p64.trainable())):
        errs[f"grad{i}"] = rel(t.grad, t64.grad)
    # (without split_batch the operator reuses the model's evaluation of x for x_ref: the running norms then take one
    # update with the batch's norm instead of two with the same norm - the same values)
    errs["norm_biased"] = rel(method.model._norm_biased, running[0])
    errs["norm_unbiased"] = rel(method.model._norm_unbiased, running[1])
    print(f"radial compute_loss_kernel split={split}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert tuple(aux["f"].shape) == tuple(aux["Tf"].shape) == (B, L)
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


def test_fused_kernel_trainer_matches_the_module_loop():
    """FusedKernelTrainer on a RadialKernelOperator (model evaluation, nsvd_rbf_apply, loss, backward and RMSprop
    inside the C calls) against the reference-style loop on the same coordinate batches: NestedLoRA.compute_loss_kernel
    on the same operator, loss.backward(), torch.optim.RMSprop - three steps, losses and parameters, with the bounds of
    the dense operator's test of the same name."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import FusedKernelTrainer, RadialKernelOperator
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    D, L, B, m = 16, 8, 256, 64
    op = RadialKernelOperator(H.RBF_GAUSSIAN, 4.0, D, 1.0, DEV)
    fk = FusedKernelTrainer(op, L=L, m=m, hidden=(128, 128), batch_size=B, sequential=False, lr=1e-3, rmsprop_decay=0.99,
                            rmsprop_eps=1e-8, fourier_scale=0.05, seed=11)
    args = NS(ndim=D, n_particles=1, use_fourier_feature=True, fourier_mapping_size=m, fourier_scale=0.05,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="128,128", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
              sort=0, loss=NS(neuralsvd=NS(step=1, sequential=False)))
    net = get_wavefunctions(args).to(DEV)
    method = get_evd_method(args, "neuralsvd", net).to(DEV)
    sd = fk.P.state_dict()
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(sd["model." + n].reshape(p.shape))
        net.base.feature_map._B.copy_(sd["model.base.feature_map._B"])
    opt = torch.optim.RMSprop(method.parameters(), lr=1e-3, alpha=0.99, eps=1e-8)
    g = torch.Generator(device=DEV).manual_seed(5)
    for t in range(3):
        x = op.sample(B, g)
        la = fk.step(x).clone()
        opt.zero_grad()
        lb, _ = method.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=False)
        lb.backward()
        opt.step()
        print(f"radial trainer step {t}: fused {float(la[0]):.7f} module {float(lb.detach()):.7f}")
        lb = lb.detach()
        assert abs(float(la[0]) - float(lb)) < 2e-5 * max(1.0, abs(float(lb))), (t, float(la[0]), float(lb))
    sd = fk.P.state_dict()
    for n, p in net.named_parameters():
        got = sd["model." + n].reshape(p.shape)
        d = float((got - p).double().norm() / p.double().norm().clamp_min(1e-30))
        assert d < (2e-4 if ".bs." in n else 2e-5), (n, d)
    # a fresh draw of its own works too, and moves the parameters
    p0 = fk.P.flat.clone()
    assert bool(torch.isfinite(fk.step()).all()) and not torch.equal(fk.P.flat, p0)


def test_kernel_spectrum_against_float64():
    """The analytic eigenfunctions k < 4 (D = 1, sigma 1, ell 1.5) on 4096 fixed-seed samples, four chunks of rows:
    Rayleigh quotients and norms against the float64 evaluation of the same Monte-Carlo quotient on the same samples
    (not against lambda_k: that gap is sampling error)."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import (RadialKernelOperator, gaussian_kernel_eigenfunctions,
                                           gaussian_kernel_eigvals, kernel_spectrum)
    n, sigma, ell, L = 4096, 1.0, 1.5, 4
    x = sigma * torch.randn(n, 1, generator=torch.Generator().manual_seed(7))
    op = RadialKernelOperator(H.RBF_GAUSSIAN, ell, 1, sigma, DEV)
    out = kernel_spectrum(op, lambda xe: gaussian_kernel_eigenfunctions(xe, sigma, ell, L), x.to(DEV), chunk=1024)
    phi = gaussian_kernel_eigenfunctions(x.double(), sigma, ell, L)
    Kphi = R.radial_kernel_apply(x, x, phi, R.GAUSSIAN, ell, 1.0 / n)
    cov, quad = (phi.T @ phi / n).numpy(), (phi.T @ Kphi / n).numpy()
    want = np.diag(quad) / np.diag(cov)
    ev = np.abs(out["eigvals"] - want) / np.abs(want)
    en = np.abs(out["norms"] - np.diag(cov)) / np.diag(cov)
    lam = gaussian_kernel_eigvals(sigma, ell, 1, L)
    print("kernel_spectrum: eigvals " + " ".join(f"{v:.6f}" for v in out["eigvals"]) + " | vs float64 " +
          " ".join(f"{v:.1e}" for v in ev) + " | norms " + " ".join(f"{v:.1e}" for v in en) +
          " | sampling gap to lambda_k " + " ".join(f"{abs(a - b) / b:.1e}" for a, b in zip(want, lam)))
    assert out["eigvals"].dtype == np.float64 and out["eigvals"].shape == (L,)
    assert ev.max() < 1e-5 and en.max() < 1e-5
    assert float(np.abs(out["quad"] - quad).max() / np.abs(quad).max()) < 1e-5


def test_interface_refusals():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import FusedKernelTrainer, RadialKernelOperator, kernel_spectrum
    op = RadialKernelOperator(H.RBF_EXPONENTIAL, 2.0, 3, 1.0, DEV)
    x = op.sample(8, torch.Generator(device=DEV).manual_seed(0))
    assert tuple(x.shape) == (8, 3) and x.is_cuda

    def model(xe):
        return xe[:, :2] * 2.0
    Kf, f = op.get_approx_kernel_op(x)(model, x)
    want = R.radial_kernel_apply(x.cpu(), x.cpu(), model(x).cpu(), R.EXPONENTIAL, 2.0, 1.0 / 8)
    assert rel(Kf, want) < 1e-5 and torch.equal(f, model(x))
    with pytest.raises(NotImplementedError, match="importance"):
        op.get_approx_kernel_op(x)(model, x, importance=torch.ones(8, device=DEV))
    with pytest.raises(NsvdError, match="GPU"):
        op.get_approx_kernel_op(x.cpu())
    with pytest.raises(NsvdError, match="GPU"):
        op.get_approx_kernel_op(x)(model, x.cpu())
    with pytest.raises(NsvdError, match="GPU"):
        kernel_spectrum(op, model, x.cpu())
    with pytest.raises(NsvdError, match="GPU"):
        RadialKernelOperator(H.RBF_GAUSSIAN, 1.0, 3, 1.0, "cpu")
    with pytest.raises(NsvdError, match="unsupported"):
        RadialKernelOperator(H.RBF_GAUSSIAN, 1.0, 65, 1.0, DEV)
    with pytest.raises(NotImplementedError, match="comm"):
        FusedKernelTrainer(op, L=4, m=64, batch_size=64, comm=NS(multi=True, world=2, rank=0))
    fk = FusedKernelTrainer(op, L=4, m=64, batch_size=64)
    with pytest.raises(NsvdError, match="GPU"):
        fk.step(torch.zeros(64, 3))
