"""GPU tests of the kernel SVD path on a DotKernelOperator: apply_pair_raw is the fused nsvd_dot_apply_pair call,
KernelSvdTrainer against the class path with the same optimiser on a polynomial operator, and a short training run
against the closed form (kernel_ops.polynomial_cross_singular_values)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import _dot_pair_oracle as P
from tests.test_dot_apply_pair_gpu import kernel32, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("kind", ["polynomial", "arccos1"])
def test_apply_pair_raw_is_the_fused_call(kind):
    """equal bits with hip_ops.dot_apply_pair; within max(2e-6, 4 x yardstick) of the base-class route (two
    nsvd_dot_apply calls), where the yardstick is the float32 library composition against float64"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator, MatrixFreeKernelOperator
    B1, B2, D, L = 130, 257, 5, 6
    gen = torch.Generator().manual_seed(5)
    x, y = torch.randn(B1, D, generator=gen), 0.5 * torch.randn(B2, D, generator=gen)
    g, f = torch.randn(B2, L, generator=gen), torch.randn(B1, L, generator=gen)
    hk, ok = (H.DOT_POLYNOMIAL, P.POLYNOMIAL) if kind == "polynomial" else (H.DOT_ARCCOS1, P.ARCCOS1)
    op = DotKernelOperator(hk, D, gamma=0.5, coef0=1.0, degree=3, device=DEV)
    assert type(op).apply_pair_raw is not MatrixFreeKernelOperator.apply_pair_raw
    assert type(op).workspace_pair is not MatrixFreeKernelOperator.workspace_pair
    xd, yd, gd, fd = x.to(DEV), y.to(DEV), g.to(DEV), f.to(DEV)
    ws = op.workspace_pair(B1, B2, L)
    assert ws.numel() == P.pair_workspace_bytes(B1, B2, D, L) and ws.device.type == "cuda"
    got = op.apply_pair_raw(xd, yd, gd, fd, 1.0 / B2, 1.0 / B1, ws=ws)
    direct = H.dot_apply_pair(xd, yd, gd, fd, hk, op.gamma, op.coef0, op.degree, 1.0 / B2, 1.0 / B1)
    assert torch.equal(got[0], direct[0]) and torch.equal(got[1], direct[1])
    base = MatrixFreeKernelOperator.apply_pair_raw(op, xd, yd, gd, fd, 1.0 / B2, 1.0 / B1)
    want = P.dot_kernel_apply_pair(x, y, g, f, ok, op.gamma, op.coef0, op.degree, 1.0 / B2, 1.0 / B1)
    k32 = kernel32(xd, yd, ok, op.gamma, op.coef0, op.degree)
    yard = (k32 @ gd / B2, k32.T @ fd / B1)
    for i, name in enumerate(("out_x", "out_y")):
        e, eb, ey = rel(got[i], want[i]), rel(got[i], base[i]), rel(yard[i], want[i])
        bound = max(2e-6, 4.0 * ey)
        print(f"{kind} {name}: vs float64 {e:.2e} vs the two-call route {eb:.2e} yardstick {ey:.2e} bound {bound:.2e}")
        assert e < bound and eb < bound, (name, e, eb, bound)
    # the consumer contract picks the fused call up with no change of its own
    Tg, ff, Tadjf, gg = op.get_approx_kernel_svd_op()(lambda t: fd, lambda t: gd, xd, yd)
    assert torch.equal(Tg, got[0]) and torch.equal(Tadjf, got[1]) and ff is fd and gg is gd


@pytest.mark.parametrize("lr", [1e-3, 1e-4])
def test_kernel_svd_trainer_matches_the_class_path_on_a_polynomial_operator(lr):
    """tests/test_kernel_svd_gpu.py:test_kernel_svd_trainer_matches_the_class_path on a polynomial DotKernelOperator:
    KernelSvdTrainer (nsvd_dot_apply_pair inside the step) against NestedLoRA.compute_loss_kernel_svd, loss.backward()
    and torch.optim.RMSprop over both models, three steps on the same batches, with that test's bounds."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator
    from neural_svd_amd.kernel_svd import KernelSvdTrainer
    from tests.test_kernel_svd_gpu import _pair_method
    D, L, B, m = 16, 8, 256, 64
    op = DotKernelOperator(H.DOT_POLYNOMIAL, D, gamma=1.0 / D, coef0=1.0, degree=2, device=DEV)
    kt = KernelSvdTrainer(op, L=L, m=m, hidden=(128, 128), batch_size=B, sigma_x=1.0, sigma_y=0.5, sequential=False,
                          lr=lr, rmsprop_decay=0.99, rmsprop_eps=1e-8, fourier_scale=0.05, seed=11)
    assert kt.pair_ws.numel() == P.pair_workspace_bytes(B, B, D, L)
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
    opt = torch.optim.RMSprop(method.parameters(), lr=lr, alpha=0.99, eps=1e-8)
    svd_op = op.get_approx_kernel_svd_op()
    for t in range(3):
        x, y = kt.sample()
        la = kt.step(x, y).clone()
        opt.zero_grad()
        lb, _ = method.compute_loss_kernel_svd(svd_op, x, y)
        lb.backward()
        opt.step()
        lb = lb.detach()
        print(f"polynomial kernel svd trainer lr {lr:g} step {t}: flat {float(la[0]):.7f} class {float(lb):.7f}")
        assert abs(float(la[0]) - float(lb)) < 2e-5 * max(1.0, abs(float(lb))), (t, float(la[0]), float(lb))
    for P_, net in pairs:
        sd = P_.state_dict()
        for n, p in net.named_parameters():
            got = sd["model." + n].reshape(p.shape)
            d = float((got - p.detach()).double().norm() / p.detach().double().norm().clamp_min(1e-30))
            assert d < (2e-4 if ".bs." in n else 2e-5), (n, d)


def test_short_training_run_moves_towards_the_closed_form():
    """200 steps, polynomial degree 2, D = 1, L = 3 (the kernel's rank), B = 512, sigma_x 1, sigma_y 0.5, gamma 0.5,
    coef0 1 (s = 1.0708, 0.5, 0.1167): the loss of the first batch, evaluated again after the run, is finite and lower,
    and |f_0| |g_0| (root mean squares on 2048 held-out samples) has moved towards s_0. How close it gets is a property
    of the schedule, reported and not asserted."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator, kernel_singular_values, polynomial_cross_singular_values
    from neural_svd_amd.kernel_svd import KernelSvdTrainer
    sx, sy, gamma, coef0, degree, L, B = 1.0, 0.5, 0.5, 1.0, 2, 3, 512
    op = DotKernelOperator(H.DOT_POLYNOMIAL, 1, gamma=gamma, coef0=coef0, degree=degree, sigma=sx, device=DEV)
    kt = KernelSvdTrainer(op, L=L, m=64, batch_size=B, sigma_x=sx, sigma_y=sy, sequential=True, lr=1e-3, seed=3)
    s = polynomial_cross_singular_values(sx, sy, gamma, coef0, degree, 1, L)
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
    print(f"polynomial kernel svd run: loss {l0:.5f} -> {l1:.5f}; |f_0||g_0| {p0:.4f} -> {p1:.4f} (s_0 {s[0]:.4f}); "
          "quotients " + " ".join(f"{v:.4f}" for v in sv) + " | closed form " + " ".join(f"{v:.4f}" for v in s))
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0
    assert abs(p1 - s[0]) < abs(p0 - s[0])
