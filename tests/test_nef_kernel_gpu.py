"""GPU checks of NeuralEF on the matrix-free kernel operators: nsvd_nef_rows_forward / nsvd_nef_rows_backward against
float64, NefKernelTrainer against the fixture recorded from the reference's own NeuralEigenfunctions
(tests/golden/nef_kernel.npz) and against the class path NeuralEigenfunctions.compute_loss_kernel on real operators.

Tolerances (none is taken from what the code under test gives):
- the two kernels accumulate in float64, so the bounds follow from the count of float32 roundings: the batch norm is one
  rounding of a float64 value (1 ulp), phi = u / n one more division by a rounded norm (4 ulps); du is formed in float64
  from the float32 inputs and rounded once, against the float64 formula on the same inputs:
  |du - du64| <= 8 eps32 (|g| + |phi s|) / n; the running norms see at most a dozen float32 roundings: 1e-6 relative.
- trainer against the fixture: per quantity max(1e-4, 4 x the float32 reference's error on that quantity in that case
  and step), both recorded in the fixture (_spin_oracle.bound): the rule test_spinx_gpu.py uses.
- trainer against the class path: 2e-4 relative - each side within 1e-4 of float64, the bound
  test_neuralef_shapes_gpu.py::test_compute_loss_kernel holds the class path to.
"""
import os

import numpy as np
import pytest
import torch

from tests import _nef_kernel_oracle as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F64 = torch.float64
EPS32 = float(torch.finfo(torch.float32).eps)
ROWS_SHAPES = [(2, 2, 1), (2, 1, 1), (3, 2, 2), (64, 64, 10), (65, 33, 33), (129, 65, 64), (130, 130, 64),
               (257, 129, 7), (1025, 513, 10),
               (8257, 4129, 5)]  # (beyond 8192 rows a workgroup takes several 64-row tiles: 128 rows, a ragged last block)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "nef_kernel.npz"))


# ---- 1. the two kernels ---------------------------------------------------------------------------------------------
def _ulp(v64):
    """the float32 spacing at |v| (v: float64 values)"""
    a = v64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _rows_input(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-3, 3, L) if L > 1 else torch.tensor([1e-3 if B % 2 else 1e3])
    return torch.randn(B, L, generator=g) * scale


def _fresh_state(L):
    return dict(nb=torch.ones(L, device=DEV), nu=torch.ones(L, device=DEV),
                init=torch.zeros(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("B,B1,L", ROWS_SHAPES)
def test_rows_forward_against_float64(B, B1, L):
    from neural_svd_amd import hip_ops as H
    u = _rows_input(B, L, 10 * B + L)
    split = B1 < B
    order = N.update_order(split)
    st = _fresh_state(L)
    ud = u.to(DEV)
    phi, stats = H.nef_rows_forward(ud, B1, st["nb"], st["nu"], st["init"], N.MOMENTUM, order)
    phi64, stats64 = N.normalize(u.double(), B1)
    assert tuple(phi.shape) == (B, L) and tuple(stats.shape) == (2, L)
    es = ((stats.cpu().double() - stats64).abs() / _ulp(stats64)).max()
    ep = ((phi.cpu().double() - phi64).abs() / _ulp(phi64)).max()
    print(f"rows_forward {(B, B1, L)}: stats {float(es):.2f} ulp, phi {float(ep):.2f} ulp")
    assert float(es) <= 1.0 and float(ep) <= 4.0
    # the columns do not share a norm: they span six decades
    if L > 1:
        assert float(stats64[0].max() / stats64[0].min()) > 1e4
    # the first update ever is a copy, `initialized` goes 0 -> 1; then the rules, in the caller's order
    assert int(st["init"].item()) == 1
    ref = dict(biased=None, unbiased=None, initialized=False)
    for h in order:
        N.running_update(ref, stats64[h])
    assert N.rel_err(st["nb"].cpu(), ref["biased"]) <= 1e-6 and N.rel_err(st["nu"].cpu(), ref["unbiased"]) <= 1e-6
    if not split:
        assert torch.equal(st["nb"], stats[0]) and torch.equal(st["nu"], stats[0])  # a copy
    # a second call meets initialised state: no copy
    H.nef_rows_forward(ud, B1, st["nb"], st["nu"], st["init"], N.MOMENTUM, order)
    for h in order:
        N.running_update(ref, stats64[h])
    assert N.rel_err(st["nb"].cpu(), ref["biased"]) <= 1e-6 and N.rel_err(st["nu"].cpu(), ref["unbiased"]) <= 1e-6
    assert int(st["init"].item()) == 1
    # equal bits from two runs, in place too, and no state touched without an order
    st2 = _fresh_state(L)
    phi2, stats2 = H.nef_rows_forward(ud, B1, st2["nb"], st2["nu"], st2["init"], N.MOMENTUM, order)
    assert torch.equal(phi2.view(torch.int32), phi.view(torch.int32)) and torch.equal(stats2, stats)
    inplace = ud.clone()
    out, _ = H.nef_rows_forward(inplace, B1, None, None, None, N.MOMENTUM, (), out=inplace)
    assert out.data_ptr() == inplace.data_ptr() and torch.equal(inplace.view(torch.int32), phi.view(torch.int32))
    st3 = _fresh_state(L)
    H.nef_rows_forward(ud, B1, st3["nb"], st3["nu"], st3["init"], N.MOMENTUM, ())
    assert int(st3["init"].item()) == 0 and torch.equal(st3["nb"], torch.ones(L, device=DEV))


def test_rows_forward_tells_the_update_orders_apart():
    from neural_svd_amd import hip_ops as H
    B, B1, L = 65, 33, 33
    u = _rows_input(B, L, 1)
    u[B1:] *= 3.0  # the two segments' norms differ by a factor
    _, stats64 = N.normalize(u.double(), B1)
    got = {}
    for order in ((0, 1, 1, 0), (1, 0, 0, 1)):
        st = _fresh_state(L)
        H.nef_rows_forward(u.to(DEV), B1, st["nb"], st["nu"], st["init"], N.MOMENTUM, order)
        ref = dict(biased=None, unbiased=None, initialized=False)
        for h in order:
            N.running_update(ref, stats64[h])
        assert N.rel_err(st["nb"].cpu(), ref["biased"]) <= 1e-6 and N.rel_err(st["nu"].cpu(), ref["unbiased"]) <= 1e-6
        got[order] = st["nb"].cpu()
    assert N.rel_err(got[(0, 1, 1, 0)], got[(1, 0, 0, 1)]) > 1e-2


@pytest.mark.parametrize("three", [False, True])
@pytest.mark.parametrize("B,B1,L", ROWS_SHAPES)
def test_rows_backward_against_float64(B, B1, L, three):
    from neural_svd_amd import hip_ops as H
    u = _rows_input(B, L, 10 * B + L)
    phi, stats = H.nef_rows_forward(u.to(DEV), B1, None, None, None, N.MOMENTUM, ())
    gen = torch.Generator().manual_seed(7 * B + L)
    cots = [torch.randn(B, L, generator=gen) * torch.logspace(2, -2, L) for _ in range(3 if three else 1)]
    dev = [c.to(DEV) for c in cots]
    d1, d2 = (dev[1], dev[2]) if three else (None, None)
    du = H.nef_rows_backward(phi, stats, B1, dev[0], d1, d2)
    # float64 on the SAME float32 inputs
    g64 = sum(c.double() for c in cots)
    p64, s64 = phi.cpu().double(), stats.cpu().double()
    want = N.normalize_backward(p64, s64, B1, g64)
    s_rows = torch.cat([(g64[:B1] * p64[:B1]).mean(0).expand(B1, L),
                        (g64[B1:] * p64[B1:]).mean(0).expand(B - B1, L) if B1 < B else g64[:0]])
    n_rows = torch.cat([s64[0].expand(B1, L), s64[1].expand(B - B1, L)])
    bound = 8 * EPS32 * (g64.abs() + (p64 * s_rows).abs()) / n_rows
    err = (du.cpu().double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"rows_backward {(B, B1, L)} three={three}: worst error / bound {worst:.3f}")
    assert bool((err <= bound).all())
    # equal bits from two runs; du may alias dphi
    assert torch.equal(H.nef_rows_backward(phi, stats, B1, dev[0], d1, d2).view(torch.int32), du.view(torch.int32))
    alias = dev[0].clone()
    out = H.nef_rows_backward(phi, stats, B1, alias, d1, d2, out=alias)
    assert out.data_ptr() == alias.data_ptr() and torch.equal(alias.view(torch.int32), du.view(torch.int32))
    # stats == NULL: the sum of the given cotangents, rounded once
    plain = H.nef_rows_backward(None, None, B1, dev[0], d1, d2)
    assert torch.equal(plain.cpu(), g64.float())


def test_rows_refusals():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    u = torch.randn(8, 4, device=DEV)
    st = _fresh_state(4)
    with pytest.raises(NsvdError):
        H.nef_rows_forward(torch.randn(8, 65, device=DEV), None, None, None, None, 0.9, ())       # L > 64
    with pytest.raises(NsvdError):
        H.nef_rows_forward(u, 0, None, None, None, 0.9, ())                                       # an empty segment
    with pytest.raises(NsvdError):
        H.nef_rows_forward(u, 8, st["nb"], st["nu"], st["init"], 0.9, (0, 1))                     # no segment 1
    with pytest.raises(NsvdError):
        H.nef_rows_forward(u, 4, st["nb"], st["nu"], st["init"], 0.9, (0, 1, 1, 0, 0))            # five updates
    with pytest.raises(NsvdError):
        H.nef_rows_forward(u, 4, None, None, None, 0.9, (0,))                                     # updates without state
    with pytest.raises(NsvdError):
        H.nef_rows_backward(None, None, 4, u, u.clone(), None)                                    # dphi1 without dphi2
    assert int(st["init"].item()) == 0 and torch.equal(st["nb"], torch.ones(4, device=DEV))


# ---- 2. the trainer against the fixture -----------------------------------------------------------------------------
def _trainer(op, cs, c, split, unbiased, mode, include_diag, B=None, **kw):
    from neural_svd_amd.neuralef import NefKernelTrainer
    args = dict(L=cs["L"], m=cs["m"], hidden=cs["hidden"], batch_size=cs["B"] if B is None else B, split_batch=split,
                unbiased=unbiased, include_diag=include_diag, batchnorm_mode=mode, lr=N.LR, optimizer="sgd",
                fourier_scale=N.FOURIER_SCALE, hard_mul_const=c, seed=3)
    args.update(kw)
    return NefKernelTrainer(op, **args)


def _trainer_quantities(tr):
    q = dict(loss=tr.loss, phi=tr.phi, Kphi=tr.Kphi, norm_biased=tr.norm_biased, norm_unbiased=tr.norm_unbiased)
    for i, g in enumerate(tr.P.views(tr.P.grad)):
        q[f"grad_{i}"] = g
    return {k: v.detach().double().cpu() for k, v in q.items()}


def _runs():
    return [(name, tag, split) for name in sorted(N.SHAPES) for tag, *_ in N.variants(name) for split in (False, True)]


@pytest.mark.parametrize("name,tag,split", _runs())
def test_trainer_matches_the_reference(golden, name, tag, split):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    _, unbiased, mode, include_diag = next(v for v in N.variants(name) if v[0] == tag)
    cs = N.SHAPES[name]
    fB, ws, bs, xs = N.load_case(golden, name)
    op = RadialKernelOperator(H.RBF_GAUSSIAN, N.ELL, cs["D"], device=DEV)
    tr = _trainer(op, cs, N.case_c(name), split, unbiased, mode, include_diag)
    tr.P.load(fB, ws, bs, None)
    failures = []
    for it in range(N.NSTEPS):
        tr.step(xs[it].to(DEV))
        got = _trainer_quantities(tr)
        for k, (ref, err32) in N.unpack_step(golden, name, tag, split, it).items():
            e = N.rel_err(N.sample(got[k]), ref)
            print(f"nef golden {name} {tag} split={int(split)} step={it} {k}: error {e:.2e} bound {N.bound(err32):.2e}")
            if not e <= N.bound(err32):
                failures.append((it, k, e, N.bound(err32)))
    assert tr.t == N.NSTEPS and int(tr.initialized.item()) == (0 if mode == "none" else 1)
    assert not failures, failures


# ---- 3. the trainer against the class path --------------------------------------------------------------------------
def _class_method(cs, fB, ws, bs, c, unbiased, mode, include_diag=False):
    from neural_svd_amd.models import GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    from neural_svd_amd.neuralef import NeuralEigenfunctions
    fm = GaussianFourierFeatureTransform(input_dim=cs["D"], mapping_size=cs["m"], scale=N.FOURIER_SCALE)
    base = ParallelMLP(input_dim=cs["D"], mlp_hidden_dims=list(cs["hidden"]), output_dim=1, num_copies=cs["L"],
                       nonlinearity="softplus", bias=True, feature_map=fm)
    model = WaveFunctions(base, boundary_mask=lambda x: 1.0, hard_mul_const=c)
    with torch.no_grad():
        fm._B.copy_(fB)
        for dst, src in zip(list(base.ws) + list(base.bs), list(ws) + list(bs)):
            dst.copy_(src)
    method = NeuralEigenfunctions(model, cs["L"], mode, unbiased=unbiased, include_diag=include_diag).to(DEV)
    return method.train(), model


def _class_step(method, model, op, x, split):
    method.zero_grad()
    loss, aux = method.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
    loss.backward()
    q = dict(loss=loss.detach().reshape(1), phi=aux["f"], Kphi=aux["Tf"])
    if hasattr(method.model, "_norm_biased"):
        q.update(norm_biased=method.model._norm_biased.data.reshape(-1),
                 norm_unbiased=method.model._norm_unbiased.data.reshape(-1))
    for i, p in enumerate(model.trainable_tensors()):
        q[f"grad_{i}"] = p.grad
    return {k: v.detach().double().cpu() for k, v in q.items()}


def _compare_with_class_path(op, L, m, hidden, B, split, unbiased, mode="unbiased", c=0.8):
    from neural_svd_amd import hip_ops as H
    cs = dict(L=L, m=m, hidden=hidden, B=B, D=op.dim)
    xs = [op.sample(B, torch.Generator(device=DEV).manual_seed(40 + i)) for i in range(3)]
    runs = []
    for _ in range(2):
        tr = _trainer(op, cs, c, split, unbiased, mode, False)
        init, fB = [t.clone() for t in tr.P.views(tr.P.flat)], tr.P.fourier_B.clone()
        steps = []
        for x in xs:
            tr.step(x)
            steps.append(_trainer_quantities(tr))
        runs.append((tr, init, fB, steps))
    (tr, init, fB, steps), (tr2, _, _, steps2) = runs
    # two trainer runs: equal bits
    assert torch.equal(tr.P.flat, tr2.P.flat) and torch.equal(tr.norm_biased, tr2.norm_biased)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(steps, steps2) for k in a)
    n = len(hidden) + 1
    method, model = _class_method(cs, fB, init[:n], init[n:], c, unbiased, mode)
    params = model.trainable_tensors()
    cfg = H.opt_config("sgd", N.LR)
    failures = []
    for t, x in enumerate(xs):
        want = _class_step(method, model, op, x, split)
        for k, ref in want.items():
            e = N.rel_err(steps[t][k], ref)
            print(f"nef trainer vs class {type(op).__name__} {(L, m, hidden, B)} split={int(split)} "
                  f"unbiased={int(unbiased)} step={t} {k}: {e:.2e}")
            if not e <= 2e-4:
                failures.append((t, k, e))
        for p in params:
            H.opt_step(cfg, p.data.view(-1), p.grad.contiguous().view(-1), None, None, None, t)
    x_eval = op.sample(64, torch.Generator(device=DEV).manual_seed(99))
    method.eval()
    with torch.no_grad():
        e = N.rel_err(tr.forward(x_eval).cpu(), method(x_eval).cpu())
    print(f"    forward in evaluation mode: {e:.2e}")
    if not e <= 2e-4:
        failures.append(("forward", e))
    assert tuple(tr(x_eval).shape) == (64, L)
    assert not failures, failures


@pytest.mark.parametrize("unbiased", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("L,m,hidden,B", [(4, 8, (16, 16), 25), (5, 64, (128, 128), 64), (10, 96, (136, 40), 130)])
def test_trainer_matches_the_class_path_on_a_radial_operator(L, m, hidden, B, split, unbiased):
    """three SGD steps of NefKernelTrainer against three of NeuralEigenfunctions.compute_loss_kernel + backward +
    nsvd_opt_step per tensor on the same batches; evaluation-mode forward; two trainer runs give equal bits"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    op = RadialKernelOperator(H.RBF_GAUSSIAN, N.ELL, 2, device=DEV)
    _compare_with_class_path(op, L, m, hidden, B, split, unbiased)


def test_trainer_matches_the_class_path_on_a_dot_operator():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator
    op = DotKernelOperator(H.DOT_POLYNOMIAL, 3, gamma=0.5, coef0=1.0, degree=2, device=DEV)
    _compare_with_class_path(op, 5, 64, (128, 128), 64, True, True)


# ---- 4. the remaining checks ----------------------------------------------------------------------------------------
def test_adam_step_is_the_class_path_gradient_plus_opt_step():
    """the optimiser rules come from FlatModel (tested for all three kernel trainers in test_spinx_gpu.py): one Adam
    step = nsvd_opt_step per tensor on the step's gradient, bit for bit, and that gradient is the class path's"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    op = RadialKernelOperator(H.RBF_GAUSSIAN, N.ELL, 2, device=DEV)
    cs = dict(L=4, m=8, hidden=(16, 16), B=25, D=2)
    lr = 1e-3
    tr = _trainer(op, cs, 0.8, True, True, "unbiased", False, optimizer="adam", lr=lr)
    init, fB = [t.clone() for t in tr.P.views(tr.P.flat)], tr.P.fourier_B.clone()
    x = op.sample(25, torch.Generator(device=DEV).manual_seed(40))
    tr.step(x)
    method, model = _class_method(cs, fB, init[:3], init[3:], 0.8, True, "unbiased")
    want = _class_step(method, model, op, x, True)
    cfg = H.opt_config("adam", lr, alpha=0.99, eps=1e-10)
    for i, (p0, g, now) in enumerate(zip(init, tr.P.views(tr.P.grad), tr.P.views(tr.P.flat))):
        assert N.rel_err(g.cpu(), want[f"grad_{i}"]) <= 2e-4
        p = p0.clone().view(-1)
        H.opt_step(cfg, p, g.contiguous().view(-1), torch.zeros_like(p), torch.zeros_like(p), None, 0)
        assert torch.equal(p, now.reshape(-1)) and not torch.equal(p0.reshape(-1), p)


def test_register_norm_and_mode_none():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    op = RadialKernelOperator(H.RBF_GAUSSIAN, N.ELL, 2, device=DEV)
    cs = dict(L=4, m=8, hidden=(16, 16), B=25, D=2)
    tr = _trainer(op, cs, 0.8, False, False, "biased", False)
    data = op.sample(100, torch.Generator(device=DEV).manual_seed(5))
    tr.register_norm(data)
    want = tr.model.evaluate(data).double().pow(2).mean(0).sqrt()
    assert N.rel_err(tr.norm_biased.cpu(), want.cpu()) <= 1e-6 and torch.equal(tr.norm_biased, tr.norm_unbiased)
    assert N.rel_err(tr.forward(data).double().pow(2).mean(0).cpu(), torch.ones(4, dtype=F64)) <= 1e-5
    plain = _trainer(op, cs, 0.8, False, False, "none", False)
    assert torch.equal(plain.forward(data), plain.model.evaluate(data))
    with pytest.raises(NsvdError, match="none"):
        plain.register_norm(data)


def test_trainer_refusals():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator, synthetic_psd_kernel
    from neural_svd_amd.neuralef import NefKernelTrainer
    op = RadialKernelOperator(H.RBF_GAUSSIAN, N.ELL, 2, device=DEV)
    with pytest.raises(NotImplementedError, match="MatrixFreeKernelOperator"):
        NefKernelTrainer(synthetic_psd_kernel(N=64, rank=8, dim=2, device=DEV), L=4, m=8, hidden=(16, 16), batch_size=16)
    for L in (0, 65):
        with pytest.raises(ValueError, match=r"L must be in 1\.\.64"):
            NefKernelTrainer(op, L=L, m=8, hidden=(16, 16), batch_size=16)
    with pytest.raises(ValueError, match="at least 2 rows"):
        NefKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=1, split_batch=True)
    with pytest.raises(ValueError, match="batchnorm_mode"):
        NefKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=16, batchnorm_mode="batch")
    with pytest.raises(NsvdError):
        NefKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=16, optimizer="lbfgs")
    tr = NefKernelTrainer(op, L=4, m=8, hidden=(16, 16), batch_size=16)
    with pytest.raises(NsvdError, match="coordinate batch"):
        tr.step(torch.zeros(15, 2, device=DEV))
    # L = 1 and a split batch of two rows (one-row segments) run
    one = NefKernelTrainer(op, L=1, m=8, hidden=(16, 16), batch_size=2, split_batch=True, unbiased=True)
    one.step()
    assert bool(torch.isfinite(one.loss).all()) and one.t == 1
