"""GPU checks of SpINx on the matrix-free kernel operators: nsvd_spinx_solve and nsvd_ts_rotate2 against float64,
SpINx.compute_loss_kernel + backward and update_weights_kernel against the fixture recorded from the reference's own
SpINx (tests/golden/spinx.npz) and against the float64 oracle on other operators, and SpinxKernelTrainer against the
class path.

Tolerances (none is taken from what the code under test gives):
- nsvd_spinx_solve: float64 arithmetic on matrices with cond(S + 1e-3 I) <= 1e3 (asserted) and L <= 64: the bounds
  test_spin_solve_matches_float64 holds nsvd_spin_solve to at cond < 2e4 - 1e-9 on the float64 outputs, 1e-6 on the
  float32 state (one rounding, 6e-8).
- nsvd_ts_rotate2: nsvd_ts_rotate's bound, 2e-7 relative - float64 sums, one rounding to float32 (6e-8 per element).
- golden comparison: per quantity max(1e-4, 4 x the float32 reference's error on that quantity in that case and step),
  both recorded in the fixture (_spin_oracle.bound).
- oracle comparison on other operators, (L, m, hidden, B, D) = golden case `b`: per quantity max(1e-4, 4 x the worst
  float32 reference error on that quantity over case b's recorded steps) - the same model, batch and decay.
- trainer against the class path: the same kernels on the same bits in the same order - equal bits.
"""
import os

import numpy as np
import pytest
import torch

from tests import _spinx_oracle as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F64 = torch.float64
T_NAMES = ("T_s", "T_pp", "T_kp", "T_pk", "T_kk")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "spinx.npz"))


# ---- 1. the small solve ---------------------------------------------------------------------------------------------
class _SolveBufs:
    """the outputs of nsvd_spinx_solve; they start as NaN so that every call has to write them"""

    def __init__(self, L, state=None):
        nan = float("nan")
        self.L = L
        self.state = torch.zeros((L, L), dtype=torch.float32, device=DEV) if state is None else state.to(DEV)
        self.chol = torch.full((L, L), nan, dtype=torch.float32, device=DEV)
        self.out64 = torch.full((2 * L + 2,), nan, dtype=F64, device=DEV)
        self.T = {k: torch.full((L, L), nan, dtype=F64, device=DEV) for k in T_NAMES}
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(self, S_raw, s_scale, Gpp, Gpk, Gkk, g_scale, w, tw, decay, update):
        from neural_svd_amd import hip_ops as H
        dev = [t.to(DEV).contiguous() for t in (Gpp, Gpk, Gkk)]
        S_dev = dev[0] if S_raw is Gpp else S_raw.to(DEV).contiguous()  # one pointer or two
        H.spinx_solve(S_dev, s_scale, dev[0], dev[1], dev[2], g_scale, w.to(DEV), None if tw is None else tw.to(DEV),
                      decay, update, self.state if update else None, self.chol if update else None, self.out64,
                      *[self.T[k] for k in T_NAMES], self.status)


def _solve_inputs(L, g, shared):
    """raw Grams of Phi (n rows; column scales in [0.5, 1.5]), P = its first B1 rows (all of them when shared), K a
    non-symmetric mix of P plus noise"""
    n = 4 * L + 3
    B1 = n if shared else 2 * L + 1
    Phi = torch.randn(n, L, generator=g, dtype=F64) * (0.5 + torch.rand(L, generator=g, dtype=F64))
    P = Phi[:B1]
    K = P @ torch.randn(L, L, generator=g, dtype=F64) / L ** 0.5 + 0.3 * torch.randn(B1, L, generator=g, dtype=F64)
    Gpp = P.T @ P
    return (Gpp if shared else Phi.T @ Phi), 1.0 / n, Gpp, P.T @ K, K.T @ K, 1.0 / B1


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("mode", ["random", "onehot_0", "onehot_L"])
@pytest.mark.parametrize("L", [2, 5, 16, 33, 64])
def test_spinx_solve_matches_float64(L, mode, shared):
    g = torch.Generator().manual_seed(1000 + 7 * L + len(mode))
    decay = 0.3
    bufs = _SolveBufs(L)
    ref_state = torch.zeros((L, L), dtype=F64)
    if mode == "random":
        w, tw = 0.5 + torch.rand(L + 1, generator=g, dtype=F64), 0.5 + torch.rand(L, generator=g, dtype=F64)
    else:
        w, tw = torch.zeros(L + 1, dtype=F64), None
        w[0 if mode == "onehot_0" else L] = float(L)
    for call in range(3):  # the second call meets non-zero state; the third leaves the state alone
        update = call < 2
        args = _solve_inputs(L, g, shared)
        state_before, chol_before = bufs.state.clone(), bufs.chol.clone()
        bufs.call(*args, w, tw, decay, update)
        out64, T, new, chol, cond = X.solve_ref(*args, w, tw, ref_state, decay)
        assert cond <= 1e3, cond
        got = bufs.out64.cpu()
        errs = dict(loss=X.rel_err(got[:1], out64[:1]), losses=X.rel_err(got[1:L + 2], out64[1:L + 2]),
                    eigvals=X.rel_err(got[L + 2:], out64[L + 2:]))
        errs.update({k: X.rel_err(bufs.T[k].cpu(), T[k]) for k in T_NAMES})
        print(f"spinx_solve L={L} {mode} shared={shared} call={call} cond={cond:.2e} " +
              " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        assert int(bufs.status.item()) == 0
        assert max(errs.values()) <= 1e-9, errs
        if update:
            es, ec = X.rel_err(bufs.state.cpu(), new), X.rel_err(bufs.chol.cpu(), chol)
            print(f"    state: sigma_avg={es:.2e} chol={ec:.2e}")
            assert es <= 1e-6 and ec <= 1e-6
            assert not bool(torch.triu(bufs.chol, 1).count_nonzero())
            ref_state = bufs.state.cpu().double()  # the state is float32: the next step starts from its rounded value
        else:
            assert torch.equal(bufs.state, state_before)
            assert torch.equal(bufs.chol.view(torch.int32), chol_before.view(torch.int32))
        for t in bufs.T.values():  # every call has to write every output
            t.fill_(float("nan"))
        bufs.out64.fill_(float("nan"))


def _assert_zero_outputs(bufs, chol_too):
    from neural_svd_amd import hip_ops as H
    assert int(bufs.status.item()) & H.RITZ_BAD_PIVOT
    outs = [bufs.out64] + list(bufs.T.values()) + ([bufs.chol] if chol_too else [])
    for t in outs + [bufs.state]:
        assert bool(torch.isfinite(t).all())
    for t in outs:
        assert not bool(t.count_nonzero())


@pytest.mark.parametrize("L", [2, 16, 64])
def test_spinx_solve_flags_a_negative_moving_average(L):
    """a negative diagonal in sigma_avg: the second factorisation fails, the status bit is set, every output is zero
    and the moving average itself was taken"""
    g = torch.Generator().manual_seed(7)
    args = _solve_inputs(L, g, False)
    bufs = _SolveBufs(L, state=-torch.eye(L, dtype=torch.float32))
    w = torch.ones(L + 1, dtype=F64)
    bufs.call(*args, w, None, 0.01, True)
    _assert_zero_outputs(bufs, True)
    want = 0.99 * (-torch.eye(L, dtype=F64)) + 0.01 * args[0] * args[1]
    assert X.rel_err(bufs.state.cpu(), want) <= 1e-6
    # the same inputs without the state update succeed
    bufs.status.zero_()
    bufs.call(*args, w, None, 0.01, False)
    assert int(bufs.status.item()) == 0 and bool(torch.isfinite(bufs.out64).all())


@pytest.mark.parametrize("update", [False, True])
@pytest.mark.parametrize("L", [2, 16, 64])
def test_spinx_solve_flags_an_indefinite_batch_matrix(L, update):
    g = torch.Generator().manual_seed(8)
    S_raw, s_scale, Gpp, Gpk, Gkk, g_scale = _solve_inputs(L, g, False)
    S_bad = S_raw - 2.0 * float(torch.linalg.eigvalsh(S_raw)[L // 2]) * torch.eye(L, dtype=F64)  # half the spectrum < 0
    state0 = torch.eye(L, dtype=torch.float32)
    bufs = _SolveBufs(L, state=state0.clone())
    bufs.call(S_bad, s_scale, Gpp, Gpk, Gkk, g_scale, torch.ones(L + 1, dtype=F64), None, 0.01, update)
    _assert_zero_outputs(bufs, update)
    if not update:
        assert torch.equal(bufs.state.cpu(), state0)
        assert bool(torch.isnan(bufs.chol).all())  # untouched


def test_spinx_solve_refusals():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    L = 4
    bufs = _SolveBufs(L)
    args = _solve_inputs(L, torch.Generator().manual_seed(1), True)
    w = torch.ones(L + 1, dtype=F64)
    with pytest.raises(NsvdError):
        bufs.call(*args, torch.ones(L, dtype=F64), None, 0.01, True)        # L weights
    with pytest.raises(NsvdError):
        bufs.call(*args, w, torch.ones(L + 1, dtype=F64), 0.01, True)       # L + 1 trace weights
    with pytest.raises(NsvdError):
        bufs.call(*args, w, None, 1.5, True)                                # decay
    with pytest.raises(NsvdError):
        bufs.call(*args, w.float(), None, 0.01, True)                       # float32 weights
    m = torch.zeros((L, L), dtype=F64, device=DEV)
    with pytest.raises(NsvdError):
        H.spinx_solve(m, 1.0, m, m, m, 1.0, w.to(DEV), None, 0.01, True, None, None, bufs.out64, m, m, m, m, m, bufs.status)
    assert bool(torch.isnan(bufs.out64).all())  # a refused call writes nothing


# ---- 2. the two-term rotation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 33, 64])
@pytest.mark.parametrize("n", [1, 31, 32, 257])
def test_ts_rotate2_against_float64(n, m):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    g = torch.Generator().manual_seed(n * 100 + m)
    wide = torch.randn(n, 2 * m + 5, generator=g).to(DEV)
    Xs, Ys = wide[:, :m], wide[:, m + 2:2 * m + 2]                      # padded row strides
    Tw = torch.randn(m, 2 * m + 3, generator=g, dtype=F64).to(DEV)
    T1, T2 = Tw[:, :m], Tw[:, m + 1:2 * m + 1]
    for k in sorted({1, m}):
        out_w = torch.full((n, k + 3), float("nan"), dtype=torch.float32, device=DEV)
        out = out_w[:, :k]
        got = H.ts_rotate2(Xs, T1, Ys, T2, k, out=out)
        want = Xs.double() @ T1[:, :k] + Ys.double() @ T2[:, :k]
        e = X.rel_err(got.cpu(), want.cpu())
        print(f"ts_rotate2 n={n} m={m} k={k}: rel {e:.1e}")
        assert e <= 2e-7
        assert bool(torch.isnan(out_w[:, k:]).all())                    # nothing past column k
        assert torch.equal(H.ts_rotate2(Xs, T1, Ys, T2, k), got)        # allocated output, equal bits
    Xc, Yc = Xs.contiguous(), Ys.contiguous()
    for bad in (Xc, Yc):
        with pytest.raises(NsvdError, match="alias"):
            H.ts_rotate2(Xc, T1, Yc, T2, m, out=bad)
    with pytest.raises(NsvdError):
        H.ts_rotate2(Xc, T1.float(), Yc, T2, m)
    with pytest.raises(NsvdError):
        H.ts_rotate2(Xc, T1, Yc[:, :1], T2, 1)


# ---- 3. / 4. the class path -----------------------------------------------------------------------------------------
def _build(cs, fB, ws, bs, c):
    from neural_svd_amd.models import GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    from neural_svd_amd.spinx import SpINx
    fm = GaussianFourierFeatureTransform(input_dim=cs["D"], mapping_size=cs["m"], scale=X.FOURIER_SCALE)
    base = ParallelMLP(input_dim=cs["D"], mlp_hidden_dims=list(cs["hidden"]), output_dim=1, num_copies=cs["L"],
                       nonlinearity="softplus", bias=True, feature_map=fm)
    model = WaveFunctions(base, boundary_mask=lambda x: 1.0, hard_mul_const=c)
    with torch.no_grad():
        fm._B.copy_(fB)
        for dst, src in zip(list(base.ws) + list(base.bs), list(ws) + list(bs)):
            dst.copy_(src)
    return SpINx(model, cs["L"], cs["decay"]).to(DEV)


def _class_step(spinx, op, x, split):
    """one compute_loss_kernel + backward; returns the quantities the fixture records"""
    params = spinx.model.trainable_tensors()
    spinx.zero_grad()
    loss, aux = spinx.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
    assert aux["eigvals"] is None and spinx.phi is aux["f"] and spinx.Tphi is aux["Tf"]
    loss.backward()
    q = dict(loss=loss.detach(), phi=aux["f"], Kphi=aux["Tf"], sigma_avg=spinx.sigma_avg.data, chol=spinx.chol.data)
    for i, p in enumerate(params):
        q[f"grad_{i}"] = p.grad.detach()
    return {k: v.detach().double().cpu() for k, v in q.items()}


def _sgd(spinx, lr):
    with torch.no_grad():
        for p in spinx.model.trainable_tensors():
            p -= lr * p.grad


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", sorted(X.CASES))
def test_compute_loss_kernel_matches_the_reference(golden, name, split):
    """every recorded step (three with unit weights, one with the non-uniform ones), then the weight update"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    cs = X.CASES[name]
    fB, ws, bs, xs = X.load_case(golden, name)
    spinx = _build(cs, fB, ws, bs, X.case_c(name))
    op = RadialKernelOperator(H.RBF_GAUSSIAN, X.ELL, cs["D"], device=DEV)
    failures = []
    for it in range(X.NSTEPS + 1):
        if it == X.NSTEPS:
            spinx.weights = X.nonuniform_weights(cs["L"]).float()
        got = _class_step(spinx, op, xs[it].to(DEV), split)
        want, _ = X.unpack_step(golden, name, split, it)
        for k, (ref, err32) in want.items():
            e = X.rel_err(X.sample(got[k]), ref)
            print(f"spinx golden {name} split={int(split)} step={it} {k}: error {e:.2e} bound {X.bound(err32):.2e}")
            if not e <= X.bound(err32):
                failures.append((it, k, e, X.bound(err32)))
        _sgd(spinx, X.LR)
    state = [spinx.sigma_avg.data.clone(), spinx.chol.data.clone()] + [p.data.clone() for p in spinx.model.parameters()]
    spinx.update_weights_kernel(op.get_approx_kernel_op, xs[X.NSTEPS].to(DEV), None, split)
    want, err32 = X.unpack_weights(golden, name, split)
    e = X.rel_err(spinx.weights, want)
    print(f"spinx golden {name} split={int(split)} weights: error {e:.2e} bound {X.bound(err32):.2e}")
    if not e <= X.bound(err32):
        failures.append(("weights", e, X.bound(err32)))
    assert tuple(spinx.weights.shape) == (cs["L"] + 1,) and not spinx.weights.requires_grad
    # no state other than the weights changed
    now = [spinx.sigma_avg.data, spinx.chol.data] + [p.data for p in spinx.model.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(state, now))
    assert not failures, failures


def test_backward_honours_the_incoming_gradient(golden):
    """ordinary autograd: (3 loss).backward() gives three times the gradient"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    cs = X.CASES["a"]
    fB, ws, bs, xs = X.load_case(golden, "a")
    op = RadialKernelOperator(H.RBF_GAUSSIAN, X.ELL, cs["D"], device=DEV)
    grads = []
    for scale in (1.0, 3.0):
        spinx = _build(cs, fB, ws, bs, 1.0)
        loss, _ = spinx.compute_loss_kernel(op.get_approx_kernel_op, xs[0].to(DEV), None, split_batch=True)
        (scale * loss).backward()
        grads.append([p.grad.clone() for p in spinx.model.trainable_tensors()])
    for a, b in zip(*grads):
        assert X.rel_err(b, 3.0 * a) <= 2e-7  # one float32 rounding of the product


def _case_b_bounds(golden):
    out = {}
    for split in (False, True):
        for it in range(X.NSTEPS + 1):
            for k, (_, e) in X.unpack_step(golden, "b", split, it)[0].items():
                out[k] = max(out.get(k, 0.0), e)
        out["weights"] = max(out.get("weights", 0.0), X.unpack_weights(golden, "b", split)[1])
    return {k: X.bound(e) for k, e in out.items()}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("kind", ["exponential", "polynomial"])
def test_compute_loss_kernel_matches_the_oracle_on_other_operators(golden, kind, split):
    """a radial and a dot-product operator the fixture does not cover, two steps with an SGD update between them and
    the weight update: the gradient into Kphi goes through each operator's own swapped-argument product"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator, RadialKernelOperator
    from tests import _dot_oracle, _rbf_oracle
    cs = X.CASES["b"]
    fB, ws, bs, xs = X.load_case(golden, "b")
    if kind == "exponential":
        op = RadialKernelOperator(H.RBF_EXPONENTIAL, 2.0, cs["D"], device=DEV)
        kernel = lambda a, b: _rbf_oracle.radial_kernel_matrix(a, b, _rbf_oracle.EXPONENTIAL, 2.0)  # noqa: E731
    else:
        op = DotKernelOperator(H.DOT_POLYNOMIAL, cs["D"], gamma=0.5, coef0=1.0, degree=2, device=DEV)
        kernel = lambda a, b: _dot_oracle.dot_kernel_matrix(a, b, _dot_oracle.POLYNOMIAL, 0.5, 1.0, 2)  # noqa: E731
    lr = 1e-3
    spinx = _build(cs, fB, ws, bs, X.case_c("b"))
    orc = X.SpinxOracle(fB, ws, bs, cs["decay"], kernel, X.case_c("b"))
    bounds = _case_b_bounds(golden)
    failures = []
    for it in range(2):
        got = _class_step(spinx, op, xs[it].to(DEV), split)
        res = orc.step(xs[it], split)
        assert float(res["cond"]) <= X.COND_MAX
        for k, ref in X.flat(res).items():
            e = X.rel_err(got[k], ref)
            print(f"spinx oracle {kind} split={int(split)} step={it} {k}: error {e:.2e} bound {bounds[k]:.2e}")
            if not e <= bounds[k]:
                failures.append((it, k, e, bounds[k]))
        _sgd(spinx, lr)
        orc.sgd(res["grad"], lr)
    spinx.update_weights_kernel(op.get_approx_kernel_op, xs[2].to(DEV), None, split)
    e = X.rel_err(spinx.weights, orc.ntk_weights(xs[2], split))
    print(f"spinx oracle {kind} split={int(split)} weights: error {e:.2e} bound {bounds['weights']:.2e}")
    if not e <= bounds["weights"]:
        failures.append(("weights", e, bounds["weights"]))
    assert not failures, failures


def test_update_weights_refuses_a_zero_norm(golden):
    """a model whose last layer is zero outputs phi = 0: Kphi = 0, every cotangent and so every NTK norm is zero;
    NsvdError, and no inf is stored"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    cs = X.CASES["a"]
    fB, ws, bs, xs = X.load_case(golden, "a")
    ws, bs = [w.clone() for w in ws], [b.clone() for b in bs]
    ws[-1].zero_()
    bs[-1].zero_()
    spinx = _build(cs, fB, ws, bs, 1.0)
    op = RadialKernelOperator(H.RBF_GAUSSIAN, X.ELL, cs["D"], device=DEV)
    before = spinx.weights.clone()
    with pytest.raises(NsvdError):
        spinx.update_weights_kernel(op.get_approx_kernel_op, xs[0].to(DEV), None, False)
    assert torch.equal(spinx.weights, before) and bool(torch.isfinite(spinx.weights).all())


# ---- 5. the trainer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("L,m,hidden,B", [(4, 8, (16, 16), 25), (5, 64, (128, 128), 64), (10, 96, (136, 40), 130)])
def test_trainer_is_the_class_path_plus_opt_step(L, m, hidden, B, split):
    """steps of SpinxKernelTrainer = steps of SpINx.compute_loss_kernel + backward + nsvd_opt_step on the same batches,
    bit for bit, before and after a weight update; two trainer runs give equal bits; the two weight updates agree to
    the class path's float32 storage of the weights"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.spinx import SpinxKernelTrainer
    D, decay, lr = 2, 0.05, 1e-3
    op = RadialKernelOperator(H.RBF_GAUSSIAN, X.ELL, D, device=DEV)
    kw = dict(L=L, m=m, hidden=hidden, batch_size=B, decay=decay, split_batch=split, lr=lr, rmsprop_decay=0.99,
              fourier_scale=X.FOURIER_SCALE, hard_mul_const=0.8, seed=3)
    xs = [op.sample(B, torch.Generator(device=DEV).manual_seed(40 + i)) for i in range(4)]
    runs = []
    for _ in range(2):
        tr = SpinxKernelTrainer(op, **kw)
        init = [t.clone() for t in tr.P.views(tr.P.flat)]
        fB = tr.P.fourier_B.clone()
        losses = [tr.step(x).clone() for x in xs[:3]]
        tr.check()
        runs.append((tr, init, fB, losses))
    (tr, init, fB, losses), (tr2, _, _, losses2) = runs
    assert torch.equal(tr.P.flat, tr2.P.flat) and torch.equal(tr.sigma_avg, tr2.sigma_avg)
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    assert tuple(tr.weights.shape) == (L + 1,) and tr.weights.is_cuda and tr.weights.dtype == F64
    n = len(hidden) + 1
    spinx = _build(dict(L=L, D=D, m=m, hidden=hidden, decay=decay), fB, init[:n], init[n:], 0.8)
    params = spinx.model.trainable_tensors()
    cfg = H.opt_config("rmsprop", lr, alpha=0.99, eps=1e-10)
    sq = [torch.zeros_like(p.data) for p in params]

    def class_step(t, x):
        spinx.zero_grad()
        loss, _ = spinx.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
        loss.backward()
        for p, s in zip(params, sq):
            H.opt_step(cfg, p.data.view(-1), p.grad.contiguous().view(-1), s.view(-1), None, None, t)
        return loss.detach()

    def same_state():
        for p, got in zip(params, tr.P.views(tr.P.flat)):
            assert torch.equal(p.data, got)
        assert torch.equal(spinx.sigma_avg.data, tr.sigma_avg) and torch.equal(spinx.chol.data, tr.chol)

    for t, x in enumerate(xs[:3]):
        assert torch.equal(class_step(t, x), losses[t][0].float())
    same_state()
    # the weight update: no state but the weights changes, on either side
    flat, sig, sqs = tr.P.flat.clone(), tr.sigma_avg.clone(), tr.P.sq.clone()
    w_tr = tr.update_weights(xs[3]).clone()
    assert torch.equal(tr.P.flat, flat) and torch.equal(tr.sigma_avg, sig) and torch.equal(tr.P.sq, sqs) and tr.t == 3
    spinx.update_weights_kernel(op.get_approx_kernel_op, xs[3], None, split)
    same_state()
    e = X.rel_err(spinx.weights, w_tr.cpu())
    print(f"trainer {(L, m, hidden, B)} split={split}: weights class vs trainer {e:.1e}")
    assert e <= 1e-6 and float(w_tr.min()) > 0 and not torch.equal(w_tr.cpu(), torch.ones(L + 1, dtype=F64))
    # one more step with these weights (the class path's float32 values on both sides)
    tr.weights.copy_(spinx.weights.double())
    loss_tr = tr.step(xs[3]).clone()
    tr.check()
    assert torch.equal(class_step(3, xs[3]), loss_tr[0].float())
    same_state()
    x_eval = op.sample(64, torch.Generator(device=DEV).manual_seed(99))
    with torch.no_grad():
        assert torch.equal(spinx.forward(x_eval), tr.forward(x_eval))


OPT_RULES = [("sgd", 0.9, 3), ("adam", 0.0, 0), ("rmsprop", 0.5, 3)]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("optimizer,momentum,num_iters", OPT_RULES)
def test_trainer_optimizer_rules_are_the_class_path_plus_opt_step(optimizer, momentum, num_iters, split):
    """the rules beside plain RMSprop (a momentum buffer, no square average, the cosine schedule), which all three kernel
    trainers take from trainer.FlatModel: three steps of SpinxKernelTrainer = three steps of the class path +
    nsvd_opt_step per tensor with its own state buffers and the scheduled rate, bit for bit (t = 3 = num_iters, where
    the rate is zero, is not reached)"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.spinx import SpinxKernelTrainer
    from neural_svd_amd.trainer import cosine_lr
    (L, m, hidden, B), D, decay, lr = (4, 8, (16, 16), 25), 2, 0.05, 1e-3
    op = RadialKernelOperator(H.RBF_GAUSSIAN, X.ELL, D, device=DEV)
    tr = SpinxKernelTrainer(op, L=L, m=m, hidden=hidden, batch_size=B, decay=decay, split_batch=split, lr=lr,
                            optimizer=optimizer, rmsprop_decay=0.99, momentum=momentum, num_iters=num_iters,
                            fourier_scale=X.FOURIER_SCALE, hard_mul_const=0.8, seed=3)
    xs = [op.sample(B, torch.Generator(device=DEV).manual_seed(40 + i)) for i in range(3)]
    init, fB = [t.clone() for t in tr.P.views(tr.P.flat)], tr.P.fourier_B.clone()
    losses = [tr.step(x).clone() for x in xs]
    tr.check()
    n = len(hidden) + 1
    spinx = _build(dict(L=L, D=D, m=m, hidden=hidden, decay=decay), fB, init[:n], init[n:], 0.8)
    params = spinx.model.trainable_tensors()
    cfg = H.opt_config(optimizer, lr, alpha=0.99, eps=1e-10, momentum=momentum)
    uses_sq, uses_mom = H.opt_uses(cfg)
    assert (tr.P.mom is not None) == uses_mom and uses_sq == (optimizer != "sgd")
    sq = [torch.zeros_like(p.data).view(-1) if uses_sq else None for p in params]
    mom = [torch.zeros_like(p.data).view(-1) if uses_mom else None for p in params]
    for t, x in enumerate(xs):
        spinx.zero_grad()
        loss, _ = spinx.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
        loss.backward()
        assert torch.equal(loss.detach(), losses[t][0].float())
        for p, s, v in zip(params, sq, mom):
            H.opt_step(cfg, p.data.view(-1), p.grad.contiguous().view(-1), s, v, None, t,
                       lr=cosine_lr(lr, t, num_iters) if num_iters else None)
    for p, got in zip(params, tr.P.views(tr.P.flat)):
        assert torch.equal(p.data, got)
    assert not any(torch.equal(a, b) for a, b in zip(init, tr.P.views(tr.P.flat)))
    assert torch.equal(spinx.sigma_avg.data, tr.sigma_avg) and torch.equal(spinx.chol.data, tr.chol)


def test_trainer_refuses_an_unknown_optimizer_and_a_decay_outside_the_unit_interval():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.spinx import SpinxKernelTrainer
    op = RadialKernelOperator(H.RBF_GAUSSIAN, X.ELL, 2, device=DEV)
    with pytest.raises(NsvdError):
        SpinxKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=25, optimizer="lbfgs")
    for decay in (-0.01, 1.5):
        with pytest.raises(ValueError, match="decay"):
            SpinxKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=25, decay=decay)
