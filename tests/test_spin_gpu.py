"""GPU checks of SpIN on the matrix-free kernel operators: nsvd_spin_solve and nsvd_spin_jac_step against float64,
SpIN.compute_loss_kernel + backward against the fixture recorded from the reference's own SpIN (tests/golden/spin.npz)
and against the float64 oracle on other operators, and SpinKernelTrainer against the class path.

Tolerances (none is taken from what the code under test gives):
- golden comparison: per quantity max(1e-4, 4 x the float32 reference's error on that quantity in that case and step),
  both recorded in the fixture (_spin_oracle.bound).
- nsvd_spin_solve: float64 arithmetic on matrices with cond(sigma_avg + 1e-3 I) <= ~1e4 and L <= 64: forward error of
  Cholesky, inverse and the triple products ~ L cond 1.1e-16 <= 1e-10; bound 1e-9. The float32 outputs (sigma_avg, chol)
  carry one rounding, 6e-8: bound 1e-6.
- nsvd_spin_jac_step: float32 activations and deltas (hardware exp2 / log2 softplus: 1.8e-6 relative per layer, through
  at most three hidden layers into both operands: ~1.1e-5) and an fp32 MFMA sum over B1 <= 96 terms (sqrt(96) 6e-8 <
  1e-6 in norm): bound 2e-5 on the relative Frobenius error per tensor.
- oracle comparison on other operators, (L, m, hidden, B, D) = golden case `b`: per quantity max(1e-4, 4 x the worst
  float32 reference error on that quantity over case b's recorded steps) - the same model, batch and decay.
"""
import os

import numpy as np
import pytest
import torch

from tests import _spin_oracle as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "spin.npz"))


# ---- 1. the small solve ---------------------------------------------------------------------------------------------
_solve_ref = S.solve_ref


@pytest.mark.parametrize("decay", [0.01, 1.0])
@pytest.mark.parametrize("L", [2, 5, 16, 64])
def test_spin_solve_matches_float64(L, decay):
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(100 + L)
    f64 = torch.float64
    n, B1 = 4 * L + 3, 2 * L + 1
    state = torch.zeros((L, L), dtype=torch.float32, device=DEV)
    chol = torch.empty_like(state)
    le = torch.empty(L + 1, dtype=f64, device=DEV)
    gs, gp = torch.empty((L, L), dtype=f64, device=DEV), torch.empty((L, L), dtype=f64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref_state = torch.zeros((L, L), dtype=f64)
    for call in range(2):  # the second call meets non-zero state
        # (decay 1: sigma itself is factored; rows scaled so that cond(sigma + 1e-3 I) stays ~1e3)
        X = torch.randn(n, L, generator=g, dtype=f64) * (0.3 if decay == 1.0 else 1.0)
        Y = torch.randn(B1, L, generator=g, dtype=f64)
        Z = torch.randn(B1, L, generator=g, dtype=f64)
        S_raw, Pi_raw = X.T @ X, Y.T @ Z
        H.spin_solve(S_raw.to(DEV), 1.0 / n, Pi_raw.to(DEV), 1.0 / B1, decay, 1.0 / B1, state, chol, le, gs, gp, status)
        new, want = _solve_ref(ref_state, S_raw / n, Pi_raw / B1, decay)
        cond = float(torch.linalg.cond(new + 1e-3 * torch.eye(L, dtype=f64)))
        assert cond < 2e4, cond
        errs = dict(sigma_avg=S.rel_err(state.cpu(), new), chol=S.rel_err(chol.cpu(), want["chol"]),
                    loss=S.rel_err(le[:1].cpu(), want["loss"]), eigvals=S.rel_err(le[1:].cpu(), want["eigvals"]),
                    gsigma=S.rel_err(gs.cpu(), want["gsigma"]), gpi=S.rel_err(gp.cpu(), want["gpi"] / B1))
        print(f"spin_solve L={L} decay={decay} call={call} cond={cond:.2e} " +
              " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        assert int(status.item()) == 0
        assert errs["sigma_avg"] <= 1e-6 and errs["chol"] <= 1e-6
        assert max(errs["loss"], errs["eigvals"], errs["gsigma"], errs["gpi"]) <= 1e-9
        assert not bool(torch.triu(chol, 1).count_nonzero())
        ref_state = state.cpu().double()  # the state is float32: the next step starts from its rounded value


@pytest.mark.parametrize("L", [2, 16, 64])
def test_spin_solve_flags_an_indefinite_matrix(L):
    """a negative diagonal in the moving average: the status bit is set and nothing non-finite is stored"""
    from neural_svd_amd import hip_ops as H
    f64 = torch.float64
    state = -torch.eye(L, dtype=torch.float32, device=DEV)
    nan = float("nan")
    chol = torch.full((L, L), nan, dtype=torch.float32, device=DEV)
    le = torch.full((L + 1,), nan, dtype=f64, device=DEV)
    gs, gp = torch.full((L, L), nan, dtype=f64, device=DEV), torch.full((L, L), nan, dtype=f64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(3 * L, L, generator=g, dtype=f64)
    H.spin_solve((X.T @ X).to(DEV), 1.0 / (3 * L), (X.T @ X).to(DEV), 1.0 / (3 * L), 0.01, 1.0, state, chol, le, gs, gp,
                 status)
    assert int(status.item()) & H.RITZ_BAD_PIVOT
    for t in (state, chol, le, gs, gp):
        assert bool(torch.isfinite(t).all())
    assert not bool(chol.count_nonzero()) and not bool(gs.count_nonzero()) and not bool(le.count_nonzero())
    # the moving average itself was taken
    want = 0.99 * (-torch.eye(L, dtype=f64)) + 0.01 * (X.T @ X) / (3 * L)
    assert S.rel_err(state.cpu(), want) <= 1e-6


# ---- 2. the Jacobian contraction ------------------------------------------------------------------------------------
JAC_SHAPES = [(2, 8, (16, 16), 3, 1), (5, 8, (16, 24), 33, 3), (4, 64, (128, 128), 64, 2),
              (16, 64, (128, 128), 96, 64), (64, 8, (16,), 40, 4), (3, 8, (16, 16, 16), 25, 2)]


_pack = S.pack_tensors


@pytest.mark.parametrize("L,m,hidden,B1,D", JAC_SHAPES)
def test_spin_jac_step_matches_the_oracle(L, m, hidden, B1, D):
    from neural_svd_amd import hip_ops as H
    torch.manual_seed(11 * L + B1)
    fB, ws, bs = S.init_params(L, D, m, hidden, seed=500 + L)
    bs = [0.1 * torch.randn_like(b) for b in bs]
    shape = H.ModelShape(L=L, D=D, m=m, hidden=hidden)
    c, decay = 0.7, 0.3
    dev_t = [t.to(DEV).contiguous() for t in ws + bs]
    params = _pack(H, shape, dev_t, fB.to(DEV).contiguous())
    P = H.spin_state_floats(shape)
    J = torch.zeros((L, P), dtype=torch.float32, device=DEV)
    J64 = [torch.zeros((L,) + tuple(t.shape), dtype=torch.float64) for t in ws + bs]
    ws64, bs64 = [w.double() for w in ws], [b.double() for b in bs]
    snapshot = None
    for call in range(2):  # the second call's moving average meets non-zero state
        x = (1.5 / (1 + D) ** 0.5) * torch.randn(B1, D)
        gsigma = torch.randn(L, L, dtype=torch.float64)
        phi64 = S.model_forward(x.double(), fB.double(), ws64, bs64, c)
        phi = phi64.float().contiguous()
        j_new = S.jacobian_contraction_einsum(x.double(), phi.double(), fB.double(), ws64, bs64, c)
        J64 = [(1.0 - decay) * jo + decay * jn for jo, jn in zip(J64, j_new)]
        want_g = [torch.einsum("ac,ac...->c...", gsigma, j) for j in J64]
        grads = [torch.zeros_like(t) for t in dev_t]
        args = (shape, params, x.to(DEV), phi.to(DEV), c, gsigma.to(DEV), decay)
        if call == 1:
            snapshot = J.clone()
        H.spin_jac_step(*args, J, _pack(H, shape, grads))
        off = 0
        for i, (j64, g64, g) in enumerate(zip(J64, want_g, grads)):
            nel = j64[0].numel()
            ej = S.rel_err(J[:, off:off + nel].cpu(), j64.reshape(L, -1))
            eg = S.rel_err(g.cpu(), g64)
            print(f"spin_jac_step {(L, m, hidden, B1, D)} call={call} tensor={i} J={ej:.2e} grad={eg:.2e}")
            assert ej <= 2e-5 and eg <= 2e-5, (call, i, ej, eg)
            off += nel
        assert off == P
    # the same call from the same state: equal bits (no atomics)
    J2 = snapshot.clone()
    grads2 = [torch.zeros_like(t) for t in dev_t]
    H.spin_jac_step(*args, J2, _pack(H, shape, grads2))
    assert torch.equal(J2, J)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)
    # the step ADDS to what the gradient buffers hold
    grads3 = [torch.full_like(t, 0.25) for t in dev_t]
    H.spin_jac_step(*args, snapshot.clone(), _pack(H, shape, grads3))
    for a, b in zip(grads, grads3):
        assert torch.equal(0.25 + a, b)


def test_spin_jac_step_refuses_masks():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    with pytest.raises(NsvdError):
        H.spin_jac_workspace(H.ModelShape(L=4, D=2, m=8, hidden=(16,), has_exp_mask=True), 8, DEV)
    with pytest.raises(NsvdError):
        H.spin_jac_workspace(H.ModelShape(L=4, D=2, m=8, hidden=(16,)), 1, DEV)


# ---- 3. / 4. the class path -----------------------------------------------------------------------------------------
def _build(name_or_cs, fB, ws, bs, c):
    from neural_svd_amd.models import GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    from neural_svd_amd.spin import SpIN
    cs = S.CASES[name_or_cs] if isinstance(name_or_cs, str) else name_or_cs
    fm = GaussianFourierFeatureTransform(input_dim=cs["D"], mapping_size=cs["m"], scale=S.FOURIER_SCALE)
    base = ParallelMLP(input_dim=cs["D"], mlp_hidden_dims=list(cs["hidden"]), output_dim=1, num_copies=cs["L"],
                       nonlinearity="softplus", bias=True, feature_map=fm)
    model = WaveFunctions(base, boundary_mask=lambda x: 1.0, hard_mul_const=c)
    with torch.no_grad():
        fm._B.copy_(fB)
        for dst, src in zip(list(base.ws) + list(base.bs), list(ws) + list(bs)):
            dst.copy_(src)
    return SpIN(model, cs["L"], cs["decay"]).to(DEV)


def _class_step(spin, op, x, split):
    """one compute_loss_kernel + backward; returns the quantities the fixture records"""
    params = spin.model.trainable_tensors()
    spin.zero_grad()
    loss, aux = spin.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
    term2 = [p.grad.detach().clone() for p in params]
    loss.backward()
    q = dict(loss=loss.detach(), eigvals=aux["eigvals"], sigma_avg=spin.sigma_avg.data, chol=spin.chol.data, phi=aux["f"],
             Kphi=aux["Tf"])
    for i, p in enumerate(params):
        q[f"term2_{i}"], q[f"grad_{i}"] = term2[i], p.grad.detach()
    return {k: v.detach().double().cpu() for k, v in q.items()}


def _sgd(spin, lr):
    with torch.no_grad():
        for p in spin.model.trainable_tensors():
            p -= lr * p.grad


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_compute_loss_kernel_matches_the_reference(golden, name, split):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    fB, ws, bs, xs = S.load_case(golden, name)
    spin = _build(name, fB, ws, bs, S.case_c(name))
    op = RadialKernelOperator(H.RBF_GAUSSIAN, S.ELL, S.CASES[name]["D"], device=DEV)
    failures = []
    for it in range(S.NSTEPS):
        got = _class_step(spin, op, xs[it].to(DEV), split)
        want, _ = S.unpack_step(golden, name, split, it)
        for k, (ref, err32) in want.items():
            e = S.rel_err(S.sample(got[k]), ref)
            print(f"spin golden {name} split={int(split)} step={it} {k}: error {e:.2e} bound {S.bound(err32):.2e}")
            if not e <= S.bound(err32):
                failures.append((it, k, e, S.bound(err32)))
        _sgd(spin, S.LR)
    assert not failures, failures


def _case_b_bounds(golden):
    out = {}
    for split in (False, True):
        for it in range(S.NSTEPS):
            for k, (_, e) in S.unpack_step(golden, "b", split, it)[0].items():
                out[k] = max(out.get(k, 0.0), e)
    return {k: S.bound(e) for k, e in out.items()}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("kind", ["exponential", "polynomial"])
def test_compute_loss_kernel_matches_the_oracle_on_other_operators(golden, kind, split):
    """a radial and a dot-product operator the fixture does not cover, two steps with an SGD update between them: the
    gradient into Kphi goes through each operator's own swapped-argument product"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator, RadialKernelOperator
    from tests import _dot_oracle, _rbf_oracle
    cs = S.CASES["b"]
    fB, ws, bs, xs = S.load_case(golden, "b")
    if kind == "exponential":
        op = RadialKernelOperator(H.RBF_EXPONENTIAL, 2.0, cs["D"], device=DEV)
        kernel = lambda a, b: _rbf_oracle.radial_kernel_matrix(a, b, _rbf_oracle.EXPONENTIAL, 2.0)  # noqa: E731
    else:
        op = DotKernelOperator(H.DOT_POLYNOMIAL, cs["D"], gamma=0.5, coef0=1.0, degree=2, device=DEV)
        kernel = lambda a, b: _dot_oracle.dot_kernel_matrix(a, b, _dot_oracle.POLYNOMIAL, 0.5, 1.0, 2)  # noqa: E731
    # (hard_mul_const 0.5 and an SGD rate of 1e-3 keep cond(sigma_avg + 1e-3 I) under COND_MAX after the polynomial
    # kernel's larger update: 521 / 672 at the second step)
    lr = 1e-3
    spin = _build("b", fB, ws, bs, 0.5)
    orc = S.SpinOracle(fB, ws, bs, cs["decay"], kernel, 0.5, S.jacobian_contraction_einsum)
    bounds = _case_b_bounds(golden)
    failures = []
    for it in range(2):
        got = _class_step(spin, op, xs[it].to(DEV), split)
        res = orc.step(xs[it], split)
        assert float(res["cond"]) <= S.COND_MAX
        want = dict(loss=res["loss"], eigvals=res["eigvals"], sigma_avg=res["sigma_avg"], chol=res["chol"],
                    phi=res["phi"], Kphi=res["Kphi"])
        for i, (t2, g) in enumerate(zip(res["term2"], res["grad"])):
            want[f"term2_{i}"], want[f"grad_{i}"] = t2, g
        for k, ref in want.items():
            e = S.rel_err(got[k], ref)
            print(f"spin oracle {kind} split={int(split)} step={it} {k}: error {e:.2e} bound {bounds[k]:.2e}")
            if not e <= bounds[k]:
                failures.append((it, k, e, bounds[k]))
        _sgd(spin, lr)
        orc.sgd(res["grad"], lr)
    assert not failures, failures


# ---- 5. the trainer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("L,m,hidden,B", [(4, 8, (16, 16), 25), (5, 64, (128, 128), 64), (10, 96, (136, 40), 130),
                                          (9, 8, (260,), 33)])
def test_trainer_is_the_class_path_plus_opt_step(L, m, hidden, B, split):
    """three steps of SpinKernelTrainer = three steps of SpIN.compute_loss_kernel + backward + nsvd_opt_step on the same
    batches, bit for bit (the two gradient terms are added in the other order: a two-term float sum commutes); two
    trainer runs give equal bits; kernel_spectrum runs on the orthonormalised functions. The last two shapes: the
    trainer's reused Jacobian workspace against the class path's fresh one at more than one column tile (2 m = 192,
    kin = 260) and short blocks of a (L = 10: 5 + 5, L = 9: 5 + 4); B = 33 with split_batch: halves of 17 and 16 rows"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator, kernel_spectrum
    from neural_svd_amd.spin import SpinKernelTrainer
    D, decay, lr = 2, 0.05, 1e-3
    op = RadialKernelOperator(H.RBF_GAUSSIAN, S.ELL, D, device=DEV)
    kw = dict(L=L, m=m, hidden=hidden, batch_size=B, decay=decay, split_batch=split, lr=lr, rmsprop_decay=0.99,
              fourier_scale=S.FOURIER_SCALE, hard_mul_const=0.8, seed=3)
    xs = [op.sample(B, torch.Generator(device=DEV).manual_seed(40 + i)) for i in range(3)]
    runs = []
    for _ in range(2):
        tr = SpinKernelTrainer(op, **kw)
        init = [t.clone() for t in tr.P.views(tr.P.flat)]
        fB = tr.P.fourier_B.clone()
        losses = [tr.step(x).clone() for x in xs]
        tr.check()
        runs.append((tr, init, fB, losses))
    (tr, init, fB, losses), (tr2, _, _, losses2) = runs
    assert torch.equal(tr.P.flat, tr2.P.flat) and torch.equal(tr.j_avg, tr2.j_avg)
    assert torch.equal(tr.sigma_avg, tr2.sigma_avg) and all(torch.equal(a, b) for a, b in zip(losses, losses2))
    n = len(hidden) + 1
    spin = _build(dict(L=L, D=D, m=m, hidden=hidden, decay=decay), fB, init[:n], init[n:], 0.8)
    params = spin.model.trainable_tensors()
    cfg = H.opt_config("rmsprop", lr, alpha=0.99, eps=1e-10)
    sq = [torch.zeros_like(p.data) for p in params]
    for t, x in enumerate(xs):
        spin.zero_grad()
        loss, aux = spin.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
        loss.backward()
        assert torch.equal(loss.detach(), losses[t][0].float())
        for p, s in zip(params, sq):
            H.opt_step(cfg, p.data.view(-1), p.grad.contiguous().view(-1), s.view(-1), None, None, t)
    for p, got in zip(params, tr.P.views(tr.P.flat)):
        assert torch.equal(p.data, got)
    assert torch.equal(spin.sigma_avg.data, tr.sigma_avg) and torch.equal(spin.chol.data, tr.chol)
    assert torch.equal(spin.j_avg.data, tr.j_avg)
    x_eval = op.sample(256, torch.Generator(device=DEV).manual_seed(99))
    spin.eval()
    with torch.no_grad():
        spec = kernel_spectrum(op, spin.forward, x_eval, chunk=128)
        assert torch.equal(spin.forward(x_eval[:64]), tr.forward(x_eval[:64]))
    assert spec["eigvals"].shape == (L,) and np.isfinite(spec["eigvals"]).all()


OPT_RULES = [("sgd", 0.9, 3), ("adam", 0.0, 0), ("rmsprop", 0.5, 3)]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("optimizer,momentum,num_iters", OPT_RULES)
def test_trainer_optimizer_rules_are_the_class_path_plus_opt_step(optimizer, momentum, num_iters, split):
    """the rules beside plain RMSprop (a momentum buffer, no square average, the cosine schedule), which all three kernel
    trainers take from trainer.FlatModel: three steps of SpinKernelTrainer = three steps of the class path +
    nsvd_opt_step per tensor with its own state buffers and the scheduled rate, bit for bit (t = 3 = num_iters, where
    the rate is zero, is not reached)"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.spin import SpinKernelTrainer
    from neural_svd_amd.trainer import cosine_lr
    (L, m, hidden, B), D, decay, lr = (4, 8, (16, 16), 25), 2, 0.05, 1e-3
    op = RadialKernelOperator(H.RBF_GAUSSIAN, S.ELL, D, device=DEV)
    tr = SpinKernelTrainer(op, L=L, m=m, hidden=hidden, batch_size=B, decay=decay, split_batch=split, lr=lr,
                           optimizer=optimizer, rmsprop_decay=0.99, momentum=momentum, num_iters=num_iters,
                           fourier_scale=S.FOURIER_SCALE, hard_mul_const=0.8, seed=3)
    xs = [op.sample(B, torch.Generator(device=DEV).manual_seed(40 + i)) for i in range(3)]
    init, fB = [t.clone() for t in tr.P.views(tr.P.flat)], tr.P.fourier_B.clone()
    losses = [tr.step(x).clone() for x in xs]
    tr.check()
    n = len(hidden) + 1
    spin = _build(dict(L=L, D=D, m=m, hidden=hidden, decay=decay), fB, init[:n], init[n:], 0.8)
    params = spin.model.trainable_tensors()
    cfg = H.opt_config(optimizer, lr, alpha=0.99, eps=1e-10, momentum=momentum)
    uses_sq, uses_mom = H.opt_uses(cfg)
    assert (tr.P.mom is not None) == uses_mom and uses_sq == (optimizer != "sgd")
    sq = [torch.zeros_like(p.data).view(-1) if uses_sq else None for p in params]
    mom = [torch.zeros_like(p.data).view(-1) if uses_mom else None for p in params]
    for t, x in enumerate(xs):
        spin.zero_grad()
        loss, _ = spin.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
        loss.backward()
        assert torch.equal(loss.detach(), losses[t][0].float())
        for p, s, v in zip(params, sq, mom):
            H.opt_step(cfg, p.data.view(-1), p.grad.contiguous().view(-1), s, v, None, t,
                       lr=cosine_lr(lr, t, num_iters) if num_iters else None)
    for p, got in zip(params, tr.P.views(tr.P.flat)):
        assert torch.equal(p.data, got)
    assert not any(torch.equal(a, b) for a, b in zip(init, tr.P.views(tr.P.flat)))
    assert torch.equal(spin.sigma_avg.data, tr.sigma_avg) and torch.equal(spin.chol.data, tr.chol)
    assert torch.equal(spin.j_avg.data, tr.j_avg)


def test_trainer_refuses_an_unknown_optimizer_and_a_decay_outside_the_unit_interval():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.spin import SpinKernelTrainer
    op = RadialKernelOperator(H.RBF_GAUSSIAN, S.ELL, 2, device=DEV)
    with pytest.raises(NsvdError):
        SpinKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=25, optimizer="lbfgs")
    for decay in (-0.01, 1.5):
        with pytest.raises(ValueError, match="decay"):
            SpinKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=25, decay=decay)
