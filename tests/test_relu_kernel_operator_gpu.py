"""GPU tests of DotKernelOperator with the deep ReLU kinds (H.DOT_RELU_NNGP, H.DOT_RELU_NTK) behind the interfaces that
inherit them through apply_raw / apply_pair_raw: get_approx_kernel_op in both split_batch modes, kernel_spectrum, Nystrom
and NystromSVD against float64 numpy, one step of FusedKernelTrainer and of KernelSvdTrainer against the class path with
Kf from the float64 oracle, and the stream contract of the two entry points (tests/_stream_contract.py). Tolerances are
those tests/test_dot_operator_gpu.py and tests/test_ksvd_baseline_gpu.py use for the arc-cosine kind."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import _relu_kernel_oracle as R
from tests import _stream_contract as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"nngp": R.RELU_NNGP, "ntk": R.RELU_NTK}
DEPTH, GAMMA, COEF0 = 3, 2.0, float(np.float32(0.1))
TOL = 1e-5


def make_op(kind, D, sigma=1.0, gamma=GAMMA, coef0=COEF0, depth=DEPTH):
    from neural_svd_amd.kernel_ops import DotKernelOperator
    op = DotKernelOperator(KINDS[kind], D, gamma=gamma, coef0=coef0, depth=depth, sigma=sigma, device=DEV)
    assert (op.kind, op.depth) == (KINDS[kind], depth)
    return op


def oracle_kf(op, x, y, f, scale):
    return R.relu_kernel_apply(x.detach().cpu(), y.detach().cpu(), f.detach().cpu(), op.kind, op.gamma, op.coef0, op.depth,
                               scale).float().to(x.device)


def oracle_operator(op):
    """get_approx_kernel_op of the same contract with Kf from the float64 oracle on the model's float32 outputs"""
    def get(x_ref):
        def run(model, x, importance=None):
            assert importance is None
            f = model(x)
            same = x is x_ref or (x.data_ptr() == x_ref.data_ptr() and x.shape == x_ref.shape)
            with torch.no_grad():
                f_ref = f.detach() if same else model(x_ref).detach()
                Kf = oracle_kf(op, x, x_ref, f_ref, 1.0 / x_ref.shape[0])
            return Kf, f
        return run
    return get


def _nestedlora_args(D, L, m, hidden="128,128"):
    return NS(ndim=D, n_particles=1, use_fourier_feature=True, fourier_mapping_size=m, fourier_scale=0.05,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims=hidden, neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
              sort=0, loss=NS(neuralsvd=NS(step=1, sequential=False)))


def _bound(got, yard, want, floor=2e-6):
    """the project's bound: (max |got - want| / max |want|, max(floor, 4 x the same figure of the float32 composition))"""
    want = torch.as_tensor(want).double().cpu()
    scale = float(want.abs().max())
    e = float((torch.as_tensor(got).double().cpu() - want).abs().max()) / scale
    ey = float((torch.as_tensor(yard).double().cpu() - want).abs().max()) / scale
    return e, max(floor, 4.0 * ey)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B", [8, 63, 64])
@pytest.mark.parametrize("split", [False, True])
def test_get_approx_kernel_op(split, B, kind):
    """the consumer contract at D = 3, L = 4 on 8, 63 and 64 rows, as NestedLoRA.compute_loss_kernel calls it: the whole
    batch against itself (split_batch = False: x is x_ref, f reused, the Gram's diagonal included) and one half against
    the other (True; odd halves at 63). Kf against the oracle on the model's own float32 outputs under
    max(2e-6, 4 x the float32 composition), f untouched."""
    D, L = 3, 4
    op = make_op(kind, D)
    xb = torch.randn(B, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    W = torch.randn(D, L, generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = []

    def model(xe):
        calls.append(xe)
        return torch.tanh(xe @ W) + 0.5
    x, x_ref = (xb[:B // 2], xb[B // 2:]) if split else (xb, xb)
    Kf, f = op.get_approx_kernel_op(x_ref)(model, x)
    assert len(calls) == (2 if split else 1) and torch.equal(f, torch.tanh(x @ W) + 0.5)
    f_ref = torch.tanh(x_ref @ W) + 0.5
    want = R.relu_kernel_apply(x.cpu(), x_ref.cpu(), f_ref.cpu(), op.kind, op.gamma, op.coef0, op.depth, 1.0 / x_ref.shape[0])
    yard = R.relu_kernel_matrix32(x, x_ref, op.kind, op.gamma, op.coef0, op.depth) @ f_ref / x_ref.shape[0]
    e, bound = _bound(Kf, yard, want)
    print(f"get_approx_kernel_op {kind} B={B} split={split}: Kf {e:.2e} bound {bound:.2e}")
    assert tuple(Kf.shape) == tuple(f.shape) and not Kf.requires_grad
    assert e < bound


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_spectrum_against_float64(kind):
    """four fixed functions of 3-D coordinates on 300 fixed-seed samples, three chunks of rows: Rayleigh quotients and
    norms against the float64 evaluation of the same quotient on the same samples, to 1e-5"""
    from neural_svd_amd.kernel_ops import kernel_spectrum
    n, D, L = 300, 3, 4
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(7))

    def fn(xe):
        return torch.stack([torch.ones_like(xe[:, 0]), xe[:, 0], xe[:, 1] * xe[:, 2], (xe * xe).sum(1) - 3.0], dim=1)
    op = make_op(kind, D)
    out = kernel_spectrum(op, fn, x.to(DEV), chunk=128)
    phi = fn(x).float().double()
    Kphi = R.relu_kernel_apply(x, x, phi, op.kind, op.gamma, op.coef0, op.depth, 1.0 / n)
    cov, quad = (phi.T @ phi / n).numpy(), (phi.T @ Kphi / n).numpy()
    want = np.diag(quad) / np.diag(cov)
    ev = np.abs(out["eigvals"] - want) / np.abs(want)
    en = np.abs(out["norms"] - np.diag(cov)) / np.diag(cov)
    print(f"kernel_spectrum {kind}: eigvals " + " ".join(f"{v:.6f}" for v in out["eigvals"]) + " | vs float64 " +
          " ".join(f"{v:.1e}" for v in ev))
    assert out["eigvals"].dtype == np.float64 and out["eigvals"].shape == (L,)
    # the bound: the arc-cosine kind's 1e-5, or 4 x what the float32 composition leaves in the same quotients (x against
    # itself: the Gram's diagonal is in every sum, and the NTK kind's diagonal carries A0's edge error)
    xd = x.to(DEV)
    K32phi = (R.relu_kernel_matrix32(xd, xd, op.kind, op.gamma, op.coef0, op.depth) @ fn(xd) / n).double().cpu()
    quad32 = (phi.T @ K32phi / n).numpy()
    bound = max(1e-5, 4.0 * float((np.abs(np.diag(quad32) / np.diag(cov) - want) / np.abs(want)).max()))
    print(f"    bound {bound:.1e}")
    assert ev.max() < bound and en.max() < 1e-5
    assert float(np.abs(out["quad"] - quad).max() / np.abs(quad).max()) < max(1e-5, 4.0 * float(
        np.abs(quad32 - quad).max() / np.abs(quad).max()))


@pytest.mark.parametrize("kind", list(KINDS))
def test_nystrom_against_eigh(kind):
    """Nystrom on n = 200 points in 3-D, 6 pairs, tol 1e-5: converged, eigenvalues and true residuals (recomputed in
    float64 from the exact Gram) within 2 tol lambda_0 of numpy.linalg.eigh, orthonormal columns"""
    from neural_svd_amd import Nystrom
    n, D, L = 200, 3, 6
    xs = torch.randn(n, D, generator=torch.Generator().manual_seed(17)).float()
    op = make_op(kind, D)
    G = R.relu_kernel_matrix(xs, xs, op.kind, op.gamma, op.coef0, op.depth).numpy() / n
    w = np.linalg.eigvalsh(G)[::-1]
    ny = Nystrom(op, xs.to(DEV), L, tol=TOL, check_every=1)
    theta, U = ny.eigvals.double().cpu().numpy(), ny.eigvecs.double().cpu().numpy()
    r = np.linalg.norm(G @ U - U * theta, axis=0)
    e = np.abs(np.sort(theta)[::-1] - w[:L]).max() / w[0]
    print(f"nystrom {kind}: iterations {ny.iterations}, worst r / lambda_0 {r.max() / w[0]:.1e}, eigenvalues {e:.1e}")
    assert ny.converged and tuple(ny.eigvecs.shape) == (n, L)
    assert r.max() <= 2 * TOL * w[0] and e <= 2 * TOL
    assert np.abs(U.T @ U - np.eye(L)).max() <= 2e-6


@pytest.mark.parametrize("kind", list(KINDS))
def test_nystrom_svd_against_svd(kind):
    """NystromSVD on 200 x 130 points in 3-D (y half as wide), 6 triplets, tol 1e-5: converged, singular values and true
    residuals within 2 tol sigma_0 of numpy.linalg.svd of the float64 cross Gram"""
    from neural_svd_amd import NystromSVD
    nx, ny_, D, L = 200, 130, 3, 6
    g = torch.Generator().manual_seed(23)
    xs, ys = torch.randn(nx, D, generator=g).float(), (0.5 * torch.randn(ny_, D, generator=g)).float()
    op = make_op(kind, D)
    C = R.relu_kernel_matrix(xs, ys, op.kind, op.gamma, op.coef0, op.depth).numpy() / math.sqrt(nx * ny_)
    sv = np.linalg.svd(C, compute_uv=False)
    sol = NystromSVD(op, xs.to(DEV), ys.to(DEV), L, tol=TOL, check_every=1)
    sg = sol.svals.double().cpu().numpy()
    U, V = sol.left.double().cpu().numpy(), sol.right.double().cpu().numpy()
    r = np.maximum(np.linalg.norm(C @ V - U * sg, axis=0), np.linalg.norm(C.T @ U - V * sg, axis=0))
    e = np.abs(sg - sv[:L]).max() / sv[0]
    print(f"nystrom_svd {kind}: iterations {sol.iterations}, worst r / sigma_0 {r.max() / sv[0]:.1e}, singular values {e:.1e}")
    assert sol.converged
    assert r.max() <= 2 * TOL * sv[0] and e <= 2 * TOL


@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_kernel_trainer_step(kind):
    """one FusedKernelTrainer step (model evaluation, nsvd_dot_apply, loss, backward and RMSprop inside the C calls)
    against the autograd route on the same weights and batch with Kf from the float64 oracle: loss and parameters, with
    the bounds of test_dot_operator_gpu.py's trainer test. sigma = 1 / 4 keeps the kernel values O(1) at D = 16."""
    from neural_svd_amd.kernel_ops import FusedKernelTrainer
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    D, L, B, m = 16, 8, 256, 64
    op = make_op(kind, D, sigma=0.25)
    fk = FusedKernelTrainer(op, L=L, m=m, hidden=(128, 128), batch_size=B, sequential=False, lr=1e-3, rmsprop_decay=0.99,
                            rmsprop_eps=1e-8, fourier_scale=0.05, seed=11)
    args = _nestedlora_args(D, L, m)
    net = get_wavefunctions(args).to(DEV)
    method = get_evd_method(args, "neuralsvd", net).to(DEV)
    sd = fk.P.state_dict()
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(sd["model." + n].reshape(p.shape))
        net.base.feature_map._B.copy_(sd["model.base.feature_map._B"])
    opt = torch.optim.RMSprop(method.parameters(), lr=1e-3, alpha=0.99, eps=1e-8)
    x = op.sample(B, torch.Generator(device=DEV).manual_seed(5))
    la = fk.step(x).clone()
    opt.zero_grad()
    lb, _ = method.compute_loss_kernel(oracle_operator(op), x, None, split_batch=False)
    lb.backward()
    opt.step()
    lb = lb.detach()
    print(f"{kind} trainer step: fused {float(la[0]):.7f} class path on the oracle's Kf {float(lb):.7f}")
    assert abs(float(la[0]) - float(lb)) < 2e-5 * max(1.0, abs(float(lb)))
    sd = fk.P.state_dict()
    for n, p in net.named_parameters():
        got = sd["model." + n].reshape(p.shape)
        d = float((got - p.detach()).double().norm() / p.detach().double().norm().clamp_min(1e-30))
        assert d < (2e-4 if ".bs." in n else 2e-5), (n, d)


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_svd_trainer_step(kind):
    """one KernelSvdTrainer step (nsvd_dot_apply_pair inside) against NestedLoRA.compute_loss_kernel_svd with Tg and
    Tadjf from the float64 oracle, loss.backward() and torch.optim.RMSprop over both models: loss and parameters, with
    the bounds of test_dot_kernel_svd_gpu.py's trainer test"""
    from neural_svd_amd.kernel_svd import KernelSvdTrainer
    from tests.test_kernel_svd_gpu import _pair_method
    D, L, B, m = 16, 8, 256, 64
    op = make_op(kind, D, sigma=0.25)
    kt = KernelSvdTrainer(op, L=L, m=m, hidden=(128, 128), batch_size=B, sigma_x=0.25, sigma_y=0.125, sequential=False,
                          lr=1e-3, rmsprop_decay=0.99, rmsprop_eps=1e-8, fourier_scale=0.05, seed=11)
    method = _pair_method(_nestedlora_args(D, L, m), 0)
    pairs = ((kt.Pf, method.model.f), (kt.Pg, method.model.g))
    with torch.no_grad():
        for P_, net in pairs:
            sd = P_.state_dict()
            for n, p in net.named_parameters():
                p.copy_(sd["model." + n].reshape(p.shape))
            net.base.feature_map._B.copy_(sd["model.base.feature_map._B"])
    opt = torch.optim.RMSprop(method.parameters(), lr=1e-3, alpha=0.99, eps=1e-8)

    def svd_op(model_f, model_g, x, y, importance=None):
        f, g = model_f(x), model_g(y)
        with torch.no_grad():
            Tg = oracle_kf(op, x, y, g, 1.0 / y.shape[0])
            Tadjf = oracle_kf(op, y, x, f, 1.0 / x.shape[0])
        return Tg, f, Tadjf, g
    x, y = kt.sample()
    la = kt.step(x, y).clone()
    opt.zero_grad()
    lb, _ = method.compute_loss_kernel_svd(svd_op, x, y)
    lb.backward()
    opt.step()
    lb = lb.detach()
    print(f"{kind} kernel svd trainer step: flat {float(la[0]):.7f} class path on the oracle's products {float(lb):.7f}")
    assert abs(float(la[0]) - float(lb)) < 2e-5 * max(1.0, abs(float(lb)))
    for P_, net in pairs:
        sd = P_.state_dict()
        for n, p in net.named_parameters():
            got = sd["model." + n].reshape(p.shape)
            d = float((got - p.detach()).double().norm() / p.detach().double().norm().clamp_min(1e-30))
            assert d < (2e-4 if ".bs." in n else 2e-5), (n, d)


# ---- the stream contract of the two entry points with the new kinds ----------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    return SC.DelayChain()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def _two(make):
    return make(torch.Generator().manual_seed(101)), make(torch.Generator().manual_seed(202))


def _apply_call(kind):
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, 1030, 3, 5  # two slices of the reference rows
    A, B = _two(lambda g: dict(x=_randn(g, B1, D), y=_randn(g, B2, D), f=_randn(g, B2, L)))

    def run(i, w, o, s):
        H.dot_apply(i["x"], i["y"], i["f"], KINDS[kind], GAMMA, COEF0, DEPTH, 1.0 / B2, ws=w[0], out=o["out"])
    return SC.Call(run, A, B, lambda: ([H.dot_apply_workspace(B1, B2, D, L, DEV)],
                                       dict(out=torch.empty(B1, L, device=DEV)), {}))


def _apply_pair_call(kind):
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 65, 257, 3, 5
    assert H.dot_apply_pair_partition(B1, B2, D, L) == (2, 2)
    A, B = _two(lambda g: dict(x=_randn(g, B1, D), y=_randn(g, B2, D), g=_randn(g, B2, L), f=_randn(g, B1, L)))

    def run(i, w, o, s):
        H.dot_apply_pair(i["x"], i["y"], i["g"], i["f"], KINDS[kind], GAMMA, COEF0, DEPTH, 1.0 / B2, 1.0 / B1, ws=w[0],
                         out_x=o["out_x"], out_y=o["out_y"])
    return SC.Call(run, A, B, lambda: ([H.dot_apply_pair_workspace(B1, B2, D, L, DEV)],
                                       dict(out_x=torch.empty(B1, L, device=DEV), out_y=torch.empty(B2, L, device=DEV)), {}))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("entry", ["dot_apply", "dot_apply_pair"])
def test_call_on_a_side_stream_behind_a_pending_producer(entry, kind, chain):
    call = (_apply_call if entry == "dot_apply" else _apply_pair_call)(kind)
    SC.check_side_stream(call, SC.eager(call, [call.A])[0], chain)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("entry", ["dot_apply", "dot_apply_pair"])
def test_captured_call_replays_on_other_inputs_over_poisoned_workspaces(entry, kind):
    call = (_apply_call if entry == "dot_apply" else _apply_pair_call)(kind)
    want = SC.eager(call, [call.A, call.B, call.B])
    assert all(torch.equal(SC.bits(want[1][k]), SC.bits(want[2][k])) for k in want[1])
    SC.check_capture(call, want)
