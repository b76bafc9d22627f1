"""GPU tests of the kernel SVD path (neural_svd_amd/kernel_svd.py, kernel_ops.apply_pair_raw /
get_approx_kernel_svd_op / kernel_singular_values): NestedLoRA.compute_loss_kernel_svd against the reference's golden
(tests/golden/kernel_svd.npz) on a RadialKernelOperator and against the float64 restatement (tests/_pair_oracle.py) on a
DotKernelOperator, KernelSvdTrainer against the class path with the same optimiser, kernel_singular_values against
float64, a short training run, and the refusals."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import _dot_oracle as DO
from tests import _pair_oracle as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().numpy()
    b = np.asarray(torch.as_tensor(b).detach().double().cpu().numpy())
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _pair_method(args, seed):
    """NestedLoRA on PairedFunctions(f, g): f seeded with `seed`, g with `seed + 1` (the golden's recipe)"""
    from neural_svd_amd.kernel_svd import PairedFunctions
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    torch.manual_seed(seed)
    net_f = get_wavefunctions(args)
    torch.manual_seed(seed + 1)
    net_g = get_wavefunctions(args)
    return get_evd_method(args, "neuralsvd", PairedFunctions(net_f, net_g)).to(DEV)


@pytest.mark.parametrize("case", ["sa", "sb", "sc"])
def test_compute_loss_kernel_svd_matches_reference_golden(case):
    """loss, f, g, Tg, Tadjf and every gradient of both models against the REFERENCE's float64 values: its
    NestedLoRALossFunctionSVD on two of its models and a float64 kernel matrix (tests/golden/make_golden_kernel_svd.py).
    Tolerance per quantity max(floor, 4 x the float32 reference's own error), the floors of
    tests/test_rbf_operator_gpu.py:test_compute_loss_kernel_matches_reference_golden."""
    from tests import _golden as G
    from tests.test_dropin_gpu import make_args
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    z = G.load("kernel_svd")
    cfg = G.cfg_of(z, case)
    method = _pair_method(make_args(cfg), cfg["seed"])
    x, y = torch.tensor(z[f"{case}_x"]).to(DEV), torch.tensor(z[f"{case}_y"]).to(DEV)
    op = RadialKernelOperator(H.RBF_GAUSSIAN, float(z[f"{case}_ell"]), x.shape[1], 1.0, DEV)
    loss, aux = method.compute_loss_kernel_svd(op.get_approx_kernel_svd_op(), x, y)
    loss.backward()
    q64, q32 = f"{case}_f64_", f"{case}_f32err_"

    def tol(key, floor):
        return max(4.0 * float(z[q32 + key]), floor)
    el = abs(float(loss.detach()) - float(z[q64 + "loss"]))
    errs = {k: rel(aux[k].detach(), torch.tensor(z[q64 + k])) for k in ("f", "g", "Tg", "Tadjf")}
    print(f"{case}: loss {el:.2e} (f32 ref {float(z[q32 + 'loss']):.2e}) " +
          " ".join(f"{k} {v:.2e} (tol {tol(k, 2e-6):.2e})" for k, v in errs.items()))
    assert aux["eigvals"] is None
    assert el < max(4.0 * float(z[q32 + "loss"]), 2e-6 * abs(float(z[q64 + "loss"])))
    for k, v in errs.items():
        assert v < tol(k, 2e-6), (k, v)
    checked = 0
    for side, net in (("f", method.model.f), ("g", method.model.g)):
        for n, t in net.named_parameters():
            if t.grad is None:
                continue
            checked += 1
            key = f"{side}.{n}"
            if q64 + f"grad_{key}" in z.files:
                want = z[q64 + f"grad_{key}"]
                assert rel(t.grad.reshape(want.shape), torch.tensor(want)) < tol(f"grad_{key}", 5e-6), key
            else:
                want = float(z[q64 + f"gradnorm_{key}"])
                assert abs(float(t.grad.double().norm()) - want) < 1e-5 * want, key
                assert rel(t.grad.reshape(-1)[::61], torch.tensor(z[q64 + f"gradsample_{key}"])) < \
                    tol(f"grad_{key}", 5e-6), key
    assert checked == 12  # three weight and three bias tensors a side


@pytest.mark.parametrize("kind", ["polynomial", "arccos1"])
def test_compute_loss_kernel_svd_on_the_two_call_base_path(kind):
    """a DotKernelOperator has no two-sided kernel: MatrixFreeKernelOperator.apply_pair_raw's two apply_raw calls.
    Tg and Tadjf against float64 (bound max(2e-6, 4 x the float32 library composition's error)); the loss and
    d loss / d f, d loss / d g against the float64 restatement of the Function's docstring on the GPU's own
    (f, Tg, g, Tadjf) (3e-5, tests/test_svd_loss_gpu.py's bound for the Function)."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator
    D, L, B = 5, 6, 96
    args = NS(ndim=D, n_particles=1, use_fourier_feature=True, fourier_mapping_size=12, fourier_scale=0.3,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="24,16", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
              sort=0, loss=NS(neuralsvd=NS(step=1, sequential=True)))
    method = _pair_method(args, 7)
    gen = torch.Generator().manual_seed(8)
    x, y = torch.randn(B, D, generator=gen), 0.5 * torch.randn(B, D, generator=gen)
    hk, ok = (H.DOT_POLYNOMIAL, DO.POLYNOMIAL) if kind == "polynomial" else (H.DOT_ARCCOS1, DO.ARCCOS1)
    op = DotKernelOperator(hk, D, gamma=0.5, coef0=1.0, degree=2, device=DEV)
    loss, aux = method.compute_loss_kernel_svd(op.get_approx_kernel_svd_op(), x.to(DEV), y.to(DEV))
    aux["f"].retain_grad()
    aux["g"].retain_grad()
    loss.backward()
    K = DO.dot_kernel_matrix(x, y, ok, 0.5, 1.0, 2)
    f64, g64 = aux["f"].detach().double().cpu(), aux["g"].detach().double().cpu()
    K32 = K.float().to(DEV)
    for name, want, yard in (("Tg", K @ g64 / B, K32 @ aux["g"].detach() / B),
                             ("Tadjf", K.T @ f64 / B, K32.T @ aux["f"].detach() / B)):
        e, ey = rel(aux[name], want), rel(yard, want)
        print(f"{kind} {name}: rel {e:.2e} yardstick {ey:.2e}")
        assert e < max(2e-6, 4.0 * ey), (name, e, ey)
    lw, dfw, dgw = P.svd_step(f64, aux["Tg"].double().cpu(), g64, aux["Tadjf"].double().cpu(),
                              method.vector_mask, method.matrix_mask)
    el = abs(float(loss.detach()) - float(lw))
    ef, eg = rel(aux["f"].grad, dfw), rel(aux["g"].grad, dgw)
    print(f"{kind}: loss {el:.2e} d/df {ef:.2e} d/dg {eg:.2e}")
    assert el <= 3e-5 * max(1.0, abs(float(lw))) and ef <= 3e-5 and eg <= 3e-5
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all())
               for n, t in method.named_parameters() if ".ws." in n or ".bs." in n)


@pytest.mark.parametrize("lr,rule", [pytest.param(1e-3, "rmsprop", id="0.001"),
                                     pytest.param(1e-4, "rmsprop", id="0.0001"),
                                     pytest.param(1e-3, "sgd", id="sgd-momentum-cosine")])
def test_kernel_svd_trainer_matches_the_class_path(lr, rule):
    """KernelSvdTrainer (two model evaluations, nsvd_rbf_apply_pair, moments, loss gradient, two backward passes and two
    RMSprop steps inside C calls) against NestedLoRA.compute_loss_kernel_svd on the same operator, loss.backward(),
    torch.optim.RMSprop over both models - three steps on the same batches, losses and parameters, with the bounds of
    tests/test_rbf_operator_gpu.py:test_fused_kernel_trainer_matches_the_module_loop.
    lr = 1e-3 is that test's: three RMSprop steps from a zero square average move every weight by about 1e-2, and the
    loss of the product f g^T of two freshly initialised models climbs - measured on an MI355X 2.7967746, 9542.3535,
    680595.00 over the three steps on the flat route against 2.7967749, 9542.3535, 680595.00 on the class path: the
    routes agree to seven digits while the step overshoots, which is what this test is about. lr = 1e-4 is the same
    comparison on a step that does not overshoot. The third case is the optimiser side of trainer.FlatModel that
    RMSprop leaves out: SGD with momentum 0.9 (no square average, a momentum buffer) under the cosine schedule of
    num_iters = 3, against torch.optim.SGD + CosineAnnealingLR(T_max=3), same bounds."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.kernel_svd import KernelSvdTrainer
    D, L, B, m = 16, 8, 256, 64
    op = RadialKernelOperator(H.RBF_GAUSSIAN, 4.0, D, 1.0, DEV)
    kt = KernelSvdTrainer(op, L=L, m=m, hidden=(128, 128), batch_size=B, sigma_x=1.0, sigma_y=0.5, sequential=False,
                          lr=lr, rmsprop_decay=0.99, rmsprop_eps=1e-8, fourier_scale=0.05, seed=11,
                          **(dict(optimizer="sgd", momentum=0.9, num_iters=3) if rule == "sgd" else {}))
    args = NS(ndim=D, n_particles=1, use_fourier_feature=True, fourier_mapping_size=m, fourier_scale=0.05,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="128,128", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
              sort=0, loss=NS(neuralsvd=NS(step=1, sequential=False)))
    method = _pair_method(args, 0)
    pairs = ((kt.Pf, method.model.f), (kt.Pg, method.model.g))
    with torch.no_grad():
        for P_, net in pairs:
            sd = P_.state_dict()
            for n, p in net.named_parameters():
                p.copy_(sd["model." + n].reshape(p.shape))
            net.base.feature_map._B.copy_(sd["model.base.feature_map._B"])
    assert not torch.equal(kt.Pf.flat, kt.Pg.flat)  # two models, seeded apart
    if rule == "sgd":
        opt = torch.optim.SGD(method.parameters(), lr=lr, momentum=0.9)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=3)
    else:
        opt, sched = torch.optim.RMSprop(method.parameters(), lr=lr, alpha=0.99, eps=1e-8), None
    svd_op = op.get_approx_kernel_svd_op()
    for t in range(3):
        x, y = kt.sample()
        la = kt.step(x, y).clone()
        opt.zero_grad()
        lb, _ = method.compute_loss_kernel_svd(svd_op, x, y)
        lb.backward()
        opt.step()
        if sched is not None:
            sched.step()
        lb = lb.detach()
        print(f"kernel svd trainer {rule} lr {lr:g} step {t}: flat {float(la[0]):.7f} class {float(lb):.7f}")
        assert abs(float(la[0]) - float(lb)) < 2e-5 * max(1.0, abs(float(lb))), (t, float(la[0]), float(lb))
    for P_, net in pairs:
        sd = P_.state_dict()
        for n, p in net.named_parameters():
            got = sd["model." + n].reshape(p.shape)
            d = float((got - p.detach()).double().norm() / p.detach().double().norm().clamp_min(1e-30))
            print(f"kernel svd trainer {rule} lr {lr:g} {n}: relative difference {d:.2e}")
            assert d < (2e-4 if ".bs." in n else 2e-5), (n, d)
    # a fresh draw of its own works too, and moves both models (but for the scheduled case: this is step t = 3 =
    # num_iters, where the cosine rate is zero)
    pf, pg = kt.Pf.flat.clone(), kt.Pg.flat.clone()
    assert bool(torch.isfinite(kt.step()).all())
    assert (torch.equal(kt.Pf.flat, pf) and torch.equal(kt.Pg.flat, pg)) if sched is not None else \
        (not torch.equal(kt.Pf.flat, pf) and not torch.equal(kt.Pg.flat, pg))
    assert tuple(kt.f(x).shape) == tuple(kt.g(y).shape) == (B, L)


def test_kernel_singular_values_against_float64():
    """The analytic eigenfunctions of the two one-measure problems as F and G (D = 1, sigma_x 1, sigma_y 0.5, ell 1.5) on
    n = 1030 fixed-seed samples a side, three chunks of rows (the last of 6): quotients, norms and the cross matrix
    against the float64 evaluation of the same Monte-Carlo quantities on the same samples (bound 1e-5,
    tests/test_rbf_operator_gpu.py:test_kernel_spectrum_against_float64's)."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator, gaussian_kernel_eigenfunctions, kernel_singular_values
    n, sx, sy, ell, L = 1030, 1.0, 0.5, 1.5, 4
    gen = torch.Generator().manual_seed(7)
    x, y = sx * torch.randn(n, 1, generator=gen), sy * torch.randn(n, 1, generator=gen)
    op = RadialKernelOperator(H.RBF_GAUSSIAN, ell, 1, sx, DEV)
    out = kernel_singular_values(op, lambda xe: gaussian_kernel_eigenfunctions(xe, sx, ell, L),
                                 lambda ye: gaussian_kernel_eigenfunctions(ye, sy, ell, L), x.to(DEV), y.to(DEV),
                                 chunk=512)
    F, G = gaussian_kernel_eigenfunctions(x.double(), sx, ell, L), gaussian_kernel_eigenfunctions(y.double(), sy, ell, L)
    KG = P.R.radial_kernel_apply(x, y, G, P.GAUSSIAN, ell, 1.0 / n)
    cf, cg, cr = (F.T @ F / n).numpy(), (G.T @ G / n).numpy(), (F.T @ KG / n).numpy()
    want = np.diag(cr) / np.sqrt(np.diag(cf) * np.diag(cg))
    es = np.abs(out["svals"] - want) / np.abs(want)
    print("kernel_singular_values: " + " ".join(f"{v:.6f}" for v in out["svals"]) + " | vs float64 " +
          " ".join(f"{v:.1e}" for v in es))
    assert out["svals"].dtype == np.float64 and out["svals"].shape == (L,)
    assert es.max() < 1e-5
    assert (np.abs(out["norms_f"] - np.diag(cf)) / np.diag(cf)).max() < 1e-5
    assert (np.abs(out["norms_g"] - np.diag(cg)) / np.diag(cg)).max() < 1e-5
    for k, w in (("cross", cr), ("cov_f", cf), ("cov_g", cg)):
        assert float(np.abs(out[k] - w).max() / np.abs(w).max()) < 1e-5, k


def test_short_training_run_moves_towards_the_closed_form():
    """200 steps at D = 1, L = 4, B = 512 (sigma_x 1, sigma_y 0.5, ell 1.5; s_0 = 0.8203): the loss of the first batch,
    evaluated again after the run, is finite and lower, and |f_0| |g_0| (root mean squares on 2048 held-out samples) has
    moved towards s_0. How close it gets is a property of the schedule, reported and not asserted."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator, gaussian_cross_singular_values, kernel_singular_values
    from neural_svd_amd.kernel_svd import KernelSvdTrainer
    sx, sy, ell, L, B = 1.0, 0.5, 1.5, 4, 512
    op = RadialKernelOperator(H.RBF_GAUSSIAN, ell, 1, sx, DEV)
    kt = KernelSvdTrainer(op, L=L, m=64, batch_size=B, sigma_x=sx, sigma_y=sy, sequential=True, lr=1e-3, seed=3)
    s = gaussian_cross_singular_values(sx, sy, ell, 1, L)
    gen = torch.Generator(device=DEV).manual_seed(99)
    xe, ye = sx * torch.randn(2048, 1, device=DEV, generator=gen), sy * torch.randn(2048, 1, device=DEV, generator=gen)

    def product():
        return float(kt.f(xe)[:, 0].double().pow(2).mean().sqrt() * kt.g(ye)[:, 0].double().pow(2).mean().sqrt())
    x0, y0 = kt.sample()
    p0 = product()
    l0 = float(kt.step(x0, y0)[0])
    for _ in range(198):
        kt.step()
    l1 = float(kt.step(x0, y0)[0])
    p1 = product()
    sv = kernel_singular_values(op, kt.f, kt.g, xe, ye)["svals"]
    print(f"kernel svd run: loss {l0:.5f} -> {l1:.5f}; |f_0||g_0| {p0:.4f} -> {p1:.4f} (s_0 {s[0]:.4f}); quotients " +
          " ".join(f"{v:.4f}" for v in sv) + " | closed form " + " ".join(f"{v:.4f}" for v in s))
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0
    assert abs(p1 - s[0]) < abs(p0 - s[0])


def test_refusals():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator, kernel_singular_values
    from neural_svd_amd.kernel_svd import KernelSvdTrainer
    from neural_svd_amd.nested_lowrank import NestedLoRA
    D, L, B = 3, 4, 64
    args = NS(ndim=D, n_particles=1, use_fourier_feature=True, fourier_mapping_size=12, fourier_scale=0.3,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="24,16", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
              sort=0, loss=NS(neuralsvd=NS(step=1, sequential=True)))
    method = _pair_method(args, 1)
    op = RadialKernelOperator(H.RBF_EXPONENTIAL, 2.0, D, 1.0, DEV)
    svd_op = op.get_approx_kernel_svd_op()
    x, y = torch.randn(B, D, device=DEV), torch.randn(B, D, device=DEV)
    with pytest.raises(NotImplementedError, match="importance"):
        method.compute_loss_kernel_svd(svd_op, x, y, importance=torch.ones(B, device=DEV))
    with pytest.raises(NsvdError, match="B1 == B2"):
        method.compute_loss_kernel_svd(svd_op, x, y[:32])
    with pytest.raises(NsvdError, match="PairedFunctions"):
        NestedLoRA(method.model.f, L).to(DEV).compute_loss_kernel_svd(svd_op, x, y)
    with pytest.raises(NsvdError, match="GPU"):
        method.compute_loss_kernel_svd(svd_op, x.cpu(), y)
    with pytest.raises(NsvdError, match="GPU"):
        kernel_singular_values(op, method.model.f, method.model.g, x.cpu(), y)
    with pytest.raises(NotImplementedError):  # the EVD-form wrappers still refuse evd=False
        method.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=False, evd=False)
    with pytest.raises(NsvdError, match="128"):
        KernelSvdTrainer(op, L=L, m=64, hidden=(64, 64), batch_size=B)
    with pytest.raises(NotImplementedError):
        KernelSvdTrainer(object(), L=L, m=64, batch_size=B)
    kt = KernelSvdTrainer(op, L=L, m=64, batch_size=B)
    with pytest.raises(NsvdError, match="GPU"):
        kt.step(x.cpu(), y)
    with pytest.raises(NsvdError, match="both"):
        kt.step(x)
    loss, aux = method.compute_loss_kernel_svd(svd_op, x, y)  # and the same arguments without the faults are accepted
    assert bool(torch.isfinite(loss)) and tuple(aux["Tg"].shape) == tuple(aux["Tadjf"].shape) == (B, L)
