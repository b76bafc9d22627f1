"""GPU tests of DotKernelOperator (neural_svd_amd/kernel_ops.py) behind the kernel-operator interface, test for test
as tests/test_rbf_operator_gpu.py: NestedLoRA's and NeuralEF's compute_loss_kernel in both split_batch modes, the fused
trainer against the autograd route, kernel_spectrum against float64, Nystrom against float64 eigh, and the refusals.

There is no reference golden for these kernels. The consumer contract is checked by running the SAME method twice from
the same seed: once on DotKernelOperator, once on an operator that obeys the same contract with Kf from the float64
oracle (tests/_dot_oracle.py) applied to the model's own float32 outputs. Everything but Kf is then identical, so
Kf is held to the bound of tests/test_dot_apply_gpu.py's floor (2e-6) and what is linear in Kf - the loss and every
gradient - to 2e-5 / 1e-4, the bounds the radial operator's trainer and NeuralEF tests use."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import _dot_oracle as R
from tests import _nystrom_oracle as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA3 = float(np.float32(1.0 / 3.0))
# name -> (kind, gamma as a function of D, coef0, degree)
KINDS = {"arccos1": (R.ARCCOS1, 1.0, 1.0, 2), "poly3": (R.POLYNOMIAL, None, 1.0, 3)}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().numpy()
    b = np.asarray(torch.as_tensor(b).detach().double().cpu().numpy())
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def make_op(name, D, sigma=1.0):
    from neural_svd_amd.kernel_ops import DotKernelOperator
    kind, gamma, coef0, degree = KINDS[name]
    gamma = float(np.float32(1.0 / D)) if gamma is None else gamma
    return DotKernelOperator(kind, D, gamma=gamma, coef0=coef0, degree=degree, sigma=sigma, device=DEV)


def oracle_operator(op):
    """get_approx_kernel_op of the same contract with Kf from the float64 oracle on the model's float32 outputs"""
    def get(x_ref):
        def run(model, x, importance=None):
            assert importance is None
            f = model(x)
            same = x is x_ref or (x.data_ptr() == x_ref.data_ptr() and x.shape == x_ref.shape)
            with torch.no_grad():
                f_ref = f.detach() if same else model(x_ref).detach()
                Kf = R.dot_kernel_apply(x.detach().cpu(), x_ref.detach().cpu(), f_ref.cpu(), op.kind, op.gamma, op.coef0,
                                        op.degree, 1.0 / x_ref.shape[0]).float().to(x.device)
            return Kf, f
        return run
    return get


def _compare(build, op, x, split, what):
    """build() -> (method, parameters to compare); run compute_loss_kernel on the operator and on its oracle twin"""
    res = []
    for get in (op.get_approx_kernel_op, oracle_operator(op)):
        method, params = build()
        loss, aux = method.compute_loss_kernel(get, x, None, split_batch=split)
        loss.backward()
        res.append((loss.detach(), aux["f"].detach(), aux["Tf"].detach(),
                    [p.grad.clone() for p in params if p.grad is not None]))
    (l, f, Kf, g), (lw, fw, Kfw, gw) = res
    errs = dict(loss=abs(float(l) - float(lw)) / max(1.0, abs(float(lw))), Kf=rel(Kf, Kfw))
    errs["grad"] = max(rel(a, b) for a, b in zip(g, gw))
    print(f"{what} split={split}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert torch.equal(f, fw) and tuple(f.shape) == tuple(Kf.shape)
    assert len(g) == len(gw) > 0 and all(float(b.abs().max()) > 0 for b in gw)
    assert errs["Kf"] < 2e-6 and errs["loss"] < 2e-5 and errs["grad"] < 1e-4, errs


def _nestedlora_args(D, L, m):
    return NS(ndim=D, n_particles=1, use_fourier_feature=True, fourier_mapping_size=m, fourier_scale=0.05,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="128,128", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
              sort=0, loss=NS(neuralsvd=NS(step=1, sequential=False)))


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("split", [False, True])
def test_nestedlora_compute_loss_kernel(split, name):
    """NestedLoRA.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch) at D = 16, L = 8, B = 130 (odd
    halves of 65): loss, Kf and every gradient against the oracle twin. Measured on an MI355X:

        arccos1 split=False: loss 0 Kf 8.2e-8 grad 4.9e-8      poly3 split=False: loss 0 Kf 6.6e-8 grad 2.8e-8
        arccos1 split=True:  loss 0 Kf 7.9e-8 grad 3.9e-8      poly3 split=True:  loss 0 Kf 6.0e-8 grad 1.9e-8"""
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    D, L, B = 16, 8, 130
    args = _nestedlora_args(D, L, 64)

    def build():
        torch.manual_seed(3)
        method = get_evd_method(args, "neuralsvd", get_wavefunctions(args)).to(DEV)
        return method, [p for p in method.parameters() if p.requires_grad]
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    _compare(build, make_op(name, D), x, split, f"NestedLoRA {name}")


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("split", [False, True])
def test_neuralef_compute_loss_kernel(split, name):
    """tests/test_rbf_operator_gpu.py's test of the same name (mode "unbiased", its shape) with the dot-product
    operator, against the oracle twin. Measured on an MI355X:

        arccos1 split=False: loss 0 Kf 9.1e-8 grad 3.3e-7      poly3 split=False: loss 8.5e-8 Kf 7.3e-8 grad 1.8e-7
        arccos1 split=True:  loss 0 Kf 7.4e-8 grad 1.8e-7      poly3 split=True:  loss 0 Kf 6.5e-8 grad 5.3e-7"""
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.neuralef import NeuralEigenfunctions
    Din, L, B = 16, 6, 97
    args = NS(ndim=Din, n_particles=1, use_fourier_feature=True, fourier_mapping_size=12, fourier_scale=0.05,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims="24,16", neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0)

    def build():
        torch.manual_seed(4)
        net = get_wavefunctions(args)
        method = NeuralEigenfunctions(net, L, batchnorm_mode="unbiased", unbiased=True).to(DEV)
        method.train()
        return method, list(net.base.ws) + list(net.base.bs)
    x = torch.randn(B, Din, generator=torch.Generator().manual_seed(3)).to(DEV)
    _compare(build, make_op(name, Din), x, split, f"NeuralEF {name}")


@pytest.mark.parametrize("name", list(KINDS))
def test_fused_kernel_trainer_matches_the_module_loop(name):
    """FusedKernelTrainer on a DotKernelOperator (model evaluation, nsvd_dot_apply, loss, backward and RMSprop inside the
    C calls) against the autograd route on the same weights and the same coordinate batch: NestedLoRA's
    compute_loss_kernel on the same operator, loss.backward(), torch.optim.RMSprop - one step on a given batch, loss and
    parameters, with the bounds of the radial operator's test of the same name. sigma = 1 / 4 keeps |x|^2 ~ 1 and the
    kernel values O(1) at D = 16, as the radial kernel's are: with sigma = 1 the arc-cosine kernel is ~16, the first
    RMSprop step (+-10 lr per element whatever the gradient's size) throws the loss from 17 to 1.3e5, and what is
    compared after it is the sensitivity of a diverged run."""
    from neural_svd_amd.kernel_ops import FusedKernelTrainer
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    D, L, B, m = 16, 8, 256, 64
    op = make_op(name, D, sigma=0.25)
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
    g = torch.Generator(device=DEV).manual_seed(5)
    for t in range(1):
        x = op.sample(B, g)
        la = fk.step(x).clone()
        opt.zero_grad()
        lb, _ = method.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=False)
        lb.backward()
        opt.step()
        print(f"{name} trainer step {t}: fused {float(la[0]):.7f} module {float(lb.detach()):.7f}")
        lb = lb.detach()
        assert abs(float(la[0]) - float(lb)) < 2e-5 * max(1.0, abs(float(lb))), (t, float(la[0]), float(lb))
    sd = fk.P.state_dict()
    for n, p in net.named_parameters():
        got = sd["model." + n].reshape(p.shape)
        d = float((got - p.detach()).double().norm() / p.detach().double().norm().clamp_min(1e-30))
        print(f"{name} trainer parameters {n}: {d:.2e}")
        assert d < (2e-4 if ".bs." in n else 2e-5), (n, d)
    # a fresh draw of its own works too, and moves the parameters
    p0 = fk.P.flat.clone()
    assert bool(torch.isfinite(fk.step()).all()) and not torch.equal(fk.P.flat, p0)


@pytest.mark.parametrize("name", list(KINDS))
def test_kernel_spectrum_against_float64(name):
    """Four fixed functions of 3-D coordinates on 2048 fixed-seed samples, four chunks of rows: Rayleigh quotients and
    norms against the float64 evaluation of the same Monte-Carlo quotient on the same samples, to the radial test's 1e-5."""
    from neural_svd_amd.kernel_ops import kernel_spectrum
    n, D, L = 2048, 3, 4
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(7))

    def fn(xe):
        return torch.stack([torch.ones_like(xe[:, 0]), xe[:, 0], xe[:, 1] * xe[:, 2], (xe * xe).sum(1) - 3.0], dim=1)
    op = make_op(name, D)
    out = kernel_spectrum(op, fn, x.to(DEV), chunk=512)
    phi = fn(x).float().double()
    Kphi = R.dot_kernel_apply(x, x, phi, op.kind, op.gamma, op.coef0, op.degree, 1.0 / n)
    cov, quad = (phi.T @ phi / n).numpy(), (phi.T @ Kphi / n).numpy()
    want = np.diag(quad) / np.diag(cov)
    ev = np.abs(out["eigvals"] - want) / np.abs(want)
    en = np.abs(out["norms"] - np.diag(cov)) / np.diag(cov)
    print(f"kernel_spectrum {name}: eigvals " + " ".join(f"{v:.6f}" for v in out["eigvals"]) + " | vs float64 " +
          " ".join(f"{v:.1e}" for v in ev) + " | norms " + " ".join(f"{v:.1e}" for v in en))
    assert out["eigvals"].dtype == np.float64 and out["eigvals"].shape == (L,)
    assert ev.max() < 1e-5 and en.max() < 1e-5
    assert float(np.abs(out["quad"] - quad).max() / np.abs(quad).max()) < 1e-5


def _align(U, Uref):
    return U * np.sign(np.sum(U * Uref, axis=0))


_NYSTROM = {}


def _nystrom_truth(name):
    """points, float64 Gram / eigh and recurrence (b) of tests/_nystrom_oracle.py, once per process"""
    if name not in _NYSTROM:
        n, D, L = 1030, 3, 5
        g = torch.Generator().manual_seed(7 + 1000 * n + 10 * D + L)
        xs, xnew = torch.randn(n, D, generator=g).float(), torch.randn(40, D, generator=g).float()
        kind, gamma, coef0, degree = KINDS[name]
        gamma = GAMMA3 if gamma is None else gamma
        G = R.dot_kernel_matrix(xs, xs, kind, gamma, coef0, degree).numpy() / n
        w, U = np.linalg.eigh(G)
        _NYSTROM[name] = dict(xs=xs, xnew=xnew, G=G, w=w[::-1].copy(), U=U[:, ::-1].copy(),
                              rec=N.subspace_iteration(G, L))
    return _NYSTROM[name]


@pytest.mark.parametrize("name", list(KINDS))
def test_nystrom_matrix_free(name):
    """Nystrom on the dot-product operator at (n, D, dim) = (1030, 3, 5), two slices in nsvd_dot_apply: arc-cosine, and
    the polynomial kernel of degree 3 whose rank C(6, 3) = 20 exceeds the basis m = 13. Assertions, tolerances and the
    residual / eigenvalue relation of tests/test_nystrom_gpu.py:test_solver_matrix_free; the yardstick is the float32
    Gram by torch ops with float32 eigh on the host. On the CPU recurrence (b) of tests/_nystrom_oracle.py converges in
    4 (arc-cosine) and 9 (polynomial) iterations, well within max_iters. Measured on an MI355X - iterations (recurrence
    (b)), worst true residual / lambda_0, eigenvalue error / lambda_0, |U^T U - I| (yardstick), worst eigenvector
    column err (yardstick; Davis-Kahan term), worst projection column rel (yardstick):

        arccos1   4 (4)   9.2e-7  1.8e-8  7.1e-9 (2.6e-9)  1.7e-8 (5.3e-9; 3.2e-7)  2.5e-7 (3.3e-7)
        poly3     8 (9)   7.5e-6  4.0e-8  9.6e-9 (4.7e-9)  3.0e-8 (4.8e-9; 6.6e-7)  1.7e-7 (2.6e-7)"""
    from neural_svd_amd import Nystrom
    TOL, n, D, L = 1e-5, 1030, 3, 5
    s = _nystrom_truth(name)
    xs, xnew, G, w, Ustar, rec = s["xs"], s["xnew"], s["G"], s["w"], s["U"][:, :L], s["rec"]
    assert rec["converged"] and N.eigen_gaps(w, L).min() >= N.MIN_GAP
    if name == "poly3":
        assert R.polynomial_rank(D, 3) == 20 > L + 8 and abs(w[20]) < 1e-12 * w[0] < w[19]
    op = make_op(name, D)
    xd = xs.to(DEV)
    ny = Nystrom(op, xd, L, tol=TOL, check_every=1)
    theta = ny.eigvals.double().cpu().numpy()
    U = ny.eigvecs.double().cpu().numpy()
    assert ny.eigvals.dtype == torch.float32 and tuple(ny.eigvals.shape) == (L,) and tuple(ny.eigvecs.shape) == (n, L)

    def k32(a, b):
        sab = a @ b.T
        if op.kind == R.POLYNOMIAL:
            return (op.gamma * sab + op.coef0) ** op.degree
        p = a.norm(dim=1)[:, None] * b.norm(dim=1)[None, :]
        c = (sab / p).clamp(-1.0, 1.0)
        t = torch.acos(c)
        return p / torch.pi * (torch.sin(t) + (torch.pi - t) * c).clamp(min=0.0)
    w32, U32 = np.linalg.eigh(k32(xd, xd).cpu().numpy())
    U32 = U32[:, ::-1][:, :L].astype(np.float64)
    I = np.eye(L)
    r = np.linalg.norm(G @ U - U * theta, axis=0)
    orth, orth_y = np.abs(U.T @ U - I).max(), np.abs(U32.T @ U32 - I).max()
    print(f"nystrom {name}: iterations {ny.iterations} (recurrence {rec['iterations']}), worst r / theta_0 "
          f"{r.max() / w[0]:.1e} (claimed {float(ny.residuals.max()):.1e}), eigenvalues "
          f"{np.abs(np.sort(theta)[::-1] - w[:L]).max() / w[0]:.1e}, UtU {orth:.1e} yardstick {orth_y:.1e}")
    assert ny.converged and len(ny.residuals) == L
    assert ny.iterations <= 2 * rec["iterations"]
    assert r.max() <= 2 * TOL * w[0]
    assert np.abs(np.sort(theta)[::-1] - w[:L]).max() <= 2 * TOL * w[0]
    assert orth <= max(2e-6, 4 * orth_y)
    gap = np.minimum(w[:L] - w[1:L + 1], np.append(np.inf, w[:L - 1] - w[1:L]))
    Ua, Uy = _align(U, Ustar), _align(U32, Ustar)
    err, yard = np.abs(Ua - Ustar).max(axis=0), np.abs(Uy - Ustar).max(axis=0)
    checked = 0
    for k in range(L):
        if gap[k] / w[k] >= 0.005:
            bound = max(4 * yard[k], 2 * r[k] / gap[k])
            assert err[k] <= bound, (k, err[k], yard[k], r[k], gap[k])
            checked += 1
    worst = int(np.argmax(err / np.maximum(4 * yard, 2 * r / gap)))
    print(f"    eigenvectors: {checked} of {L} columns checked; column {worst}: err {err[worst]:.1e} yardstick "
          f"{yard[worst]:.1e} Davis-Kahan {2 * r[worst] / gap[worst]:.1e}")
    assert checked >= 1
    # Nystrom(xnew) against the definition's formula evaluated with the object's OWN eigenpairs
    xn = xnew.to(DEV)
    got = ny(xn).double().cpu().numpy()
    Kn = R.dot_kernel_matrix(xnew, xs, op.kind, op.gamma, op.coef0, op.degree).numpy()
    want = Kn @ U / theta / np.sqrt(n)
    ref32 = (k32(xn, xd) @ ny.eigvecs / ny.eigvals / np.sqrt(n)).double().cpu().numpy()
    cmax = np.abs(want).max(axis=0)
    e, ey = np.abs(got - want).max(axis=0) / cmax, np.abs(ref32 - want).max(axis=0) / cmax
    worst = int(np.argmax(e / np.maximum(2e-6, 4 * ey)))
    print(f"    projection: worst column {worst}: rel {e[worst]:.1e} yardstick {ey[worst]:.1e}")
    assert got.shape == (40, L) and np.isfinite(got).all()
    assert np.all(e <= np.maximum(2e-6, 4 * ey)), (e, ey)


def test_nystrom_at_the_rank_of_a_polynomial_gram():
    """degree 2 at D = 3 has rank 10: a basis of m = dim + oversample = 10 columns, the most the Gram supports (see
    Nystrom's note on oversample), converges at once (lambda_11 = 0) and gives the float64 eigenvalues to 2 tol"""
    from neural_svd_amd import Nystrom
    from neural_svd_amd.kernel_ops import DotKernelOperator
    xs = torch.randn(200, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    op = DotKernelOperator(R.POLYNOMIAL, 3, gamma=GAMMA3, coef0=1.0, degree=2, device=DEV)
    ny = Nystrom(op, xs, 5, oversample=5, check_every=1)
    w = np.linalg.eigvalsh(R.dot_kernel_matrix(xs.cpu(), xs.cpu(), R.POLYNOMIAL, GAMMA3, 1.0, 2).numpy() / 200)[::-1]
    print(f"nystrom at the rank: iterations {ny.iterations}")
    assert ny.converged and ny.iterations <= 3
    assert np.abs(ny.eigvals.double().cpu().numpy() - w[:5]).max() <= 2e-5 * w[0]


def test_interface_refusals():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import DotKernelOperator, FusedKernelTrainer, kernel_spectrum
    op = DotKernelOperator(H.DOT_ARCCOS1, 3, sigma=1.0, device=DEV)
    x = op.sample(8, torch.Generator(device=DEV).manual_seed(0))
    assert tuple(x.shape) == (8, 3) and x.is_cuda

    def model(xe):
        return xe[:, :2] * 2.0
    Kf, f = op.get_approx_kernel_op(x)(model, x)
    want = R.dot_kernel_apply(x.cpu(), x.cpu(), model(x).cpu(), R.ARCCOS1, 1.0, 1.0, 2, 1.0 / 8)
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
        DotKernelOperator(H.DOT_ARCCOS1, 3, device="cpu")
    with pytest.raises(NsvdError, match="unsupported"):
        DotKernelOperator(H.DOT_ARCCOS1, 65, device=DEV)
    with pytest.raises(ValueError):
        DotKernelOperator(H.DOT_POLYNOMIAL, 3, gamma=0.0, device=DEV)
    with pytest.raises(ValueError):
        DotKernelOperator(H.DOT_POLYNOMIAL, 3, coef0=-1.0, device=DEV)
    with pytest.raises(NotImplementedError, match="comm"):
        FusedKernelTrainer(op, L=4, m=64, batch_size=64, comm=NS(multi=True, world=2, rank=0))
    fk = FusedKernelTrainer(op, L=4, m=64, batch_size=64)
    with pytest.raises(NsvdError, match="GPU"):
        fk.step(torch.zeros(64, 3))
