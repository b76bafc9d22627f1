"""GPU tests of the dense two-sided product and its trainer (csrc/kernel_apply_pair.hip, hip_ops.kernel_apply_pair,
kernel_ops.DenseCrossOperator, kernel_svd.DenseSvdTrainer): parity with the float64 restatement
(tests/_dense_pair_oracle.py), agreement with the two existing routes (two nsvd_kernel_apply calls on A and a transposed
copy; nsvd_rbf_apply_pair on the coordinates of a Gram matrix), bit reproducibility, caller-provided buffers, the class
path against float64 autograd, the trainer against the class path, a short run and the refusals."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _dense_pair_oracle as DP
from tests import _pair_oracle as P
from tests import _rbf_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 7.0  # what the column padding of A holds in these tests: anything finite is allowed there


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().numpy()
    b = np.asarray(torch.as_tensor(b).detach().double().cpu().numpy())
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def padded(A: torch.Tensor, extra_rows: int = 0) -> torch.Tensor:
    """A (N1, N2) float32 on the host -> the (N1 + extra_rows, ceil64(N2)) device copy, padding filled with PAD"""
    N1, N2 = A.shape
    out = torch.full((N1 + extra_rows, (N2 + 63) // 64 * 64), PAD, dtype=torch.float32)
    out[:N1, :N2] = A
    return out.to(DEV)


def problem(N1, N2, B1, B2, L, seed):
    """a seeded non-symmetric matrix, index batches drawn with replacement, g (B2, L) and f (B1, L)"""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randn(N1, N2, generator=gen) + 0.25
    rows, cols = torch.randint(N1, (B1,), generator=gen), torch.randint(N2, (B2,), generator=gen)
    g, f = torch.randn(B2, L, generator=gen), torch.randn(B1, L, generator=gen)
    return A, rows, cols, g, f


CASES = [(130, 67, 5, 400, 1), (300, 1000, 193, 70, 33), (1000, 300, 64, 64, 8), (2048, 2304, 512, 512, 64),
         (130, 200, 401, 90, 5), (300, 130, 1024, 1024, 70)]


def _check(shape):
    """relative L2 < 3e-5 on both outputs (tests/test_kernel_apply_gpu.py's bound for a float32 MFMA contraction over up
    to 10 000 terms), then again with rows[0] and cols[0] out of range: zero rows, no contribution"""
    from neural_svd_amd import hip_ops as H
    N1, N2, B1, B2, L = shape
    A, rows, cols, g, f = problem(*shape, seed=sum(shape))
    Ad = padded(A, extra_rows=2)
    if shape == (2048, 2304, 512, 512, 64):
        RG, CG = H.kernel_apply_pair_partition(*shape)
        assert RG > 1 and CG > 1, (RG, CG)
    for bad in (False, True):
        if bad:
            rows, cols = rows.clone(), cols.clone()
            rows[0], cols[0] = -1, N2 + 5
        ox, oy = H.kernel_apply_pair(Ad, N1, N2, rows.to(DEV), cols.to(DEV), g.to(DEV), f.to(DEV), 1.0 / B2, 1.0 / B1)
        wx, wy = DP.dense_apply_pair(A.numpy(), N1, N2, rows.numpy(), cols.numpy(), g.numpy(), f.numpy(), 1.0 / B2,
                                     1.0 / B1)
        ex, ey = rel(ox, wx), rel(oy, wy)
        print(f"dense pair {shape} bad={bad}: A g {ex:.2e}  A^T f {ey:.2e}")
        assert tuple(ox.shape) == (B1, L) and tuple(oy.shape) == (B2, L)
        assert ex < 3e-5 and ey < 3e-5, (ex, ey)
        if bad:
            assert not bool(ox[0].any()) and not bool(oy[0].any())
            assert not wx[0].any() and not wy[0].any()


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "-".join(map(str, s)))
def test_parity_with_float64(shape):
    _check(shape)


@pytest.mark.parametrize("N2,tail", [(1030, 1), (1100, 2), (1160, 3), (1230, 4)])
def test_every_length_of_the_last_slice(N2, tail):
    """B1 = 130 (one row group requests the rows of a successor tile) and 16 + tail column chunks: five slices in four
    column groups, so one group owns two slices (add-and-store flush), and its last slice has `tail` chunks; B2 = 200
    column indices drawn with replacement"""
    from neural_svd_amd import hip_ops as H
    shape = (300, N2, 130, 200, 65)
    assert H.kernel_apply_pair_partition(*shape) == (2, 4) and (N2 + 63) // 64 == 16 + tail
    _check(shape)


def test_agrees_with_two_kernel_apply_calls():
    """square non-symmetric A: out_x against kernel_apply(A, rows, cols, g), out_y against kernel_apply on a transposed
    copy with the roles swapped; 6e-5 relative - each side is within 3e-5 of float64"""
    from neural_svd_amd import hip_ops as H
    N, B, L = 1000, 256, 16
    A, rows, cols, g, f = problem(N, N, B, B, L, seed=5)
    Ad, At = padded(A), padded(A.T.contiguous())
    rows, cols, g, f = rows.to(DEV), cols.to(DEV), g.to(DEV), f.to(DEV)
    ox, oy = H.kernel_apply_pair(Ad, N, N, rows, cols, g, f, 1.0 / B, 1.0 / B)
    wx = H.kernel_apply(Ad, N, rows, cols, g, 1.0 / B)
    wy = H.kernel_apply(At, N, cols, rows, f, 1.0 / B)
    ex, ey = rel(ox, wx), rel(oy, wy)
    print(f"dense pair against two kernel_apply calls: A g {ex:.2e}  A^T f {ey:.2e}")
    assert ex < 6e-5 and ey < 6e-5


def test_agrees_with_the_matrix_free_route():
    """A = the Gaussian Gram of fixed points: apply_pair_raw on indices against rbf_apply_pair on points[idx]"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DenseCrossOperator, RadialKernelOperator
    N1, N2, D, B, L, ell = 300, 200, 3, 128, 8, 1.5
    gen = torch.Generator().manual_seed(17)
    px, py = torch.randn(N1, D, generator=gen), 0.5 * torch.randn(N2, D, generator=gen)
    A = R.radial_kernel_matrix(px, py, R.GAUSSIAN, ell).float()
    op = DenseCrossOperator(A.to(DEV), px.to(DEV), py.to(DEV))
    rop = RadialKernelOperator(H.RBF_GAUSSIAN, ell, D, 1.0, DEV)
    rows, cols = torch.randint(N1, (B,), generator=gen).to(DEV), torch.randint(N2, (B,), generator=gen).to(DEV)
    g, f = torch.randn(B, L, generator=gen).to(DEV), torch.randn(B, L, generator=gen).to(DEV)
    ox, oy = op.apply_pair_raw(rows, cols, g, f, 1.0 / B, 1.0 / B)
    wx, wy = rop.apply_pair_raw(op.points_x[rows].contiguous(), op.points_y[cols].contiguous(), g, f, 1.0 / B, 1.0 / B)
    ex, ey = rel(ox, wx), rel(oy, wy)
    print(f"dense pair against rbf_apply_pair: K g {ex:.2e}  K^T f {ey:.2e}")
    assert ex < 6e-5 and ey < 6e-5


def test_bit_reproducible_and_stream_independent():
    from neural_svd_amd import hip_ops as H
    shape = (2048, 2304, 512, 512, 64)
    N1, N2, B1, B2, L = shape
    A, rows, cols, g, f = problem(*shape, seed=3)
    cols[:40] = cols[0]  # many duplicates of one column: the scatter's order is fixed too
    Ad, rows, cols, g, f = padded(A), rows.to(DEV), cols.to(DEV), g.to(DEV), f.to(DEV)
    a = H.kernel_apply_pair(Ad, N1, N2, rows, cols, g, f, 0.5, 0.25)
    b = H.kernel_apply_pair(Ad, N1, N2, rows, cols, g, f, 0.5, 0.25)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = H.kernel_apply_pair(Ad, N1, N2, rows, cols, g, f, 0.5, 0.25)
    side.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_caller_buffers_and_a_short_workspace():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    shape = (300, 1000, 193, 70, 33)
    N1, N2, B1, B2, L = shape
    A, rows, cols, g, f = problem(*shape, seed=9)
    Ad, rows, cols, g, f = padded(A), rows.to(DEV), cols.to(DEV), g.to(DEV), f.to(DEV)
    a = H.kernel_apply_pair(Ad, N1, N2, rows, cols, g, f, 1.0, 2.0)
    ws = H.kernel_apply_pair_workspace(N1, N2, B1, B2, L, DEV)
    ws.fill_(255)  # (NaN patterns: nothing is read before it is written)
    ox, oy = torch.full((B1, L), 3.0, device=DEV), torch.full((B2, L), 3.0, device=DEV)
    b = H.kernel_apply_pair(Ad, N1, N2, rows, cols, g, f, 1.0, 2.0, ws=ws, out_x=ox, out_y=oy)
    assert b[0] is ox and b[1] is oy and torch.equal(a[0], ox) and torch.equal(a[1], oy)
    short = torch.empty(ws.numel() - 1, dtype=torch.uint8, device=DEV)
    ox.fill_(3.0)
    with pytest.raises(NsvdError):
        H.kernel_apply_pair(Ad, N1, N2, rows, cols, g, f, 1.0, 2.0, ws=short, out_x=ox, out_y=oy)
    assert bool((ox == 3.0).all())  # a refused call writes nothing


def _args(D, L, m, hidden, sequential):
    return NS(ndim=D, n_particles=1, use_fourier_feature=True, fourier_mapping_size=m, fourier_scale=0.3,
              fourier_deterministic=False, fourier_append_raw=False, mlp_hidden_dims=hidden, neigs=L, parallel=1,
              nonlinearity="softplus", apply_exp_mask=0, exp_mask_init_scale=1.0, hard_mul_const=1.0, apply_boundary=0,
              sort=0, loss=NS(neuralsvd=NS(step=1, sequential=sequential)))


def _index_method(op, args_f, args_g, seed):
    """NestedLoRA on op.index_models(f, g): f seeded with `seed`, g with `seed + 1`"""
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    torch.manual_seed(seed)
    net_f = get_wavefunctions(args_f)
    torch.manual_seed(seed + 1)
    net_g = get_wavefunctions(args_g)
    return get_evd_method(args_f, "neuralsvd", op.index_models(net_f, net_g)).to(DEV), net_f, net_g


def _cross_operator(N1, N2, Dx, Dy, seed):
    """a Gaussian-shaped rectangular matrix on two point sets of different dimensions (the first min(Dx, Dy)
    coordinates are compared), plus a seeded perturbation: entries of order one, nothing symmetric"""
    from neural_svd_amd.kernel_ops import DenseCrossOperator
    gen = torch.Generator().manual_seed(seed)
    px, py = torch.randn(N1, Dx, generator=gen), 0.5 * torch.randn(N2, Dy, generator=gen)
    d = min(Dx, Dy)
    A = (R.radial_kernel_matrix(px[:, :d], py[:, :d], R.GAUSSIAN, 1.5) +
         0.05 * torch.randn(N1, N2, generator=gen).double()).float()
    return DenseCrossOperator(A.to(DEV), px.to(DEV), py.to(DEV)), A


def _params64(net):
    p = O.Params([w.detach().double().cpu().requires_grad_() for w in net.base.ws],
                 [b.detach().double().cpu().requires_grad_() for b in net.base.bs],
                 net.base.feature_map._B.detach().double().cpu())
    return p


def test_class_path_against_float64_autograd():
    """NestedLoRA.compute_loss_kernel_svd on index columns against float64: the models restated by
    oracle/nsvd_oracle.py, the two products from the gathered block of tests/_dense_pair_oracle.py, the loss and
    d loss / d f, d loss / d g of NestedLoRALossFunctionSVD by tests/_pair_oracle.py:svd_step (sequential nesting: the
    masked gradient is the Function's own, not the derivative of the loss value), carried to the parameters by torch
    autograd in float64. Bounds: the loss within
    3e-5 max(1, |loss|) (tests/test_svd_loss_gpu.py's bound for the Function), the products within the family's 3e-5,
    every gradient norm within 1e-5 relative (tests/test_kernel_svd_gpu.py's golden comparison)."""
    N1, N2, Dx, Dy, L, B = 130, 90, 3, 2, 6, 96
    op, A = _cross_operator(N1, N2, Dx, Dy, seed=21)
    method, net_f, net_g = _index_method(op, _args(Dx, L, 12, "24,16", True), _args(Dy, L, 12, "24,16", True), 7)
    gen = torch.Generator().manual_seed(22)
    ix, iy = torch.randint(N1, (B,), generator=gen), torch.randint(N2, (B,), generator=gen)
    loss, aux = method.compute_loss_kernel_svd(op.get_approx_kernel_svd_op(), ix.to(DEV)[:, None], iy.to(DEV)[:, None])
    loss.backward()
    pf, pg = _params64(net_f), _params64(net_g)
    f64 = O.mlp_forward(O.fourier_features(op.points_x.double().cpu()[ix], pf.fourier_B), pf)
    g64 = O.mlp_forward(O.fourier_features(op.points_y.double().cpu()[iy], pg.fourier_B), pg)
    blk = torch.tensor(DP.gathered_block(A.numpy(), N1, N2, ix.numpy(), iy.numpy()))
    Tg, Tadjf = blk @ g64.detach() / B, blk.T @ f64.detach() / B
    v, M = method.vector_mask.double().cpu(), method.matrix_mask.double().cpu()
    want, df, dg = P.svd_step(f64.detach(), Tg, g64.detach(), Tadjf, v, M)
    torch.autograd.backward([f64, g64], [df, dg])
    el = abs(float(loss.detach()) - float(want))
    et, ea = rel(aux["Tg"], Tg), rel(aux["Tadjf"], Tadjf)
    print(f"dense class path: loss {float(loss.detach()):.7f} want {float(want):.7f} ({el:.2e}); Tg {et:.2e} "
          f"Tadjf {ea:.2e}")
    assert el <= 3e-5 * max(1.0, abs(float(want))) and et < 3e-5 and ea < 3e-5
    checked = 0
    for side, net, p in (("f", net_f, pf), ("g", net_g, pg)):
        for kind, mine, ref in (("ws", net.base.ws, p.ws), ("bs", net.base.bs, p.bs)):
            for i, (t, r) in enumerate(zip(mine, ref)):
                got, w = float(t.grad.double().norm()), float(r.grad.norm())
                print(f"dense class path grad {side}.{kind}.{i}: norm {got:.8e} want {w:.8e} rel {abs(got - w) / w:.2e}")
                assert abs(got - w) < 1e-5 * w, (side, kind, i)
                checked += 1
    assert checked == 12  # three weight and three bias tensors a side


@pytest.mark.parametrize("rule", ["rmsprop", "sgd"])
def test_dense_svd_trainer_matches_the_class_path(rule):
    """DenseSvdTrainer.step on given index batches against the class-path loop (compute_loss_kernel_svd on index
    columns, loss.backward(), torch.optim over both models) for 3 steps, with the bounds of
    tests/test_kernel_svd_gpu.py:test_kernel_svd_trainer_matches_the_class_path; sgd: momentum 0.9 under the cosine
    schedule of num_iters = 3, as there."""
    from neural_svd_amd.kernel_svd import DenseSvdTrainer
    N1, N2, Dx, Dy, L, B, m, lr = 600, 500, 3, 2, 8, 256, 64, 1e-3
    op, _ = _cross_operator(N1, N2, Dx, Dy, seed=31)
    kt = DenseSvdTrainer(op, L=L, m=m, hidden=(128, 128), batch_size=B, sequential=False, lr=lr, rmsprop_decay=0.99,
                         rmsprop_eps=1e-8, fourier_scale=0.05, seed=11,
                         **(dict(optimizer="sgd", momentum=0.9, num_iters=3) if rule == "sgd" else {}))
    assert kt.shapes[0].D == Dx and kt.shapes[1].D == Dy
    af, ag = _args(Dx, L, m, "128,128", False), _args(Dy, L, m, "128,128", False)
    af.fourier_scale = ag.fourier_scale = 0.05
    method, net_f, net_g = _index_method(op, af, ag, 0)
    pairs = ((kt.Pf, net_f), (kt.Pg, net_g))
    with torch.no_grad():
        for P_, net in pairs:
            sd = P_.state_dict()
            for n, p in net.named_parameters():
                p.copy_(sd["model." + n].reshape(p.shape))
            net.base.feature_map._B.copy_(sd["model.base.feature_map._B"])
    if rule == "sgd":
        opt = torch.optim.SGD(method.parameters(), lr=lr, momentum=0.9)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=3)
    else:
        opt, sched = torch.optim.RMSprop(method.parameters(), lr=lr, alpha=0.99, eps=1e-8), None
    svd_op = op.get_approx_kernel_svd_op()
    for t in range(3):
        ix, iy = kt.sample()
        la = kt.step(ix, iy).clone()
        opt.zero_grad()
        lb, _ = method.compute_loss_kernel_svd(svd_op, ix[:, None], iy[:, None])
        lb.backward()
        opt.step()
        if sched is not None:
            sched.step()
        lb = lb.detach()
        print(f"dense svd trainer {rule} step {t}: flat {float(la[0]):.7f} class {float(lb):.7f}")
        assert abs(float(la[0]) - float(lb)) < 2e-5 * max(1.0, abs(float(lb))), (t, float(la[0]), float(lb))
    for P_, net in pairs:
        sd = P_.state_dict()
        for n, p in net.named_parameters():
            got = sd["model." + n].reshape(p.shape)
            d = float((got - p.detach()).double().norm() / p.detach().double().norm().clamp_min(1e-30))
            print(f"dense svd trainer {rule} {n}: relative difference {d:.2e}")
            assert d < (2e-4 if ".bs." in n else 2e-5), (n, d)
    assert bool(torch.isfinite(kt.step()).all())  # a fresh draw of its own works too
    assert tuple(kt.f(op.points_x[:5]).shape) == tuple(kt.g(op.points_y[:5]).shape) == (5, L)


def test_short_run_moves_towards_the_leading_singular_value():
    """N1 = 600, N2 = 500, B = 256, L = 4, 300 steps: the loss of the first batch, evaluated again after the run, is
    lower, and the leading quotient has moved towards svdvals(A)[0] / sqrt(N1 N2). How close it gets is a property of
    the schedule: reported, not asserted."""
    from neural_svd_amd.kernel_svd import DenseSvdTrainer
    N1, N2, L, B = 600, 500, 4, 256
    op, A = _cross_operator(N1, N2, 2, 2, seed=41)
    s = np.linalg.svd(A.double().numpy(), compute_uv=False)[:L] / np.sqrt(N1 * N2)
    kt = DenseSvdTrainer(op, L=L, m=64, batch_size=B, sequential=True, lr=1e-3, seed=3)
    q0 = kt.quotients()["svals"]
    ix, iy = kt.sample()
    l0 = float(kt.step(ix, iy)[0])
    for _ in range(298):
        kt.step()
    l1 = float(kt.step(ix, iy)[0])
    q1 = kt.quotients()["svals"]
    print(f"dense svd run: loss {l0:.5f} -> {l1:.5f}; quotients " + " ".join(f"{v:.4f}" for v in q0) + " -> " +
          " ".join(f"{v:.4f}" for v in q1) + " | svdvals / sqrt(N1 N2) " + " ".join(f"{v:.4f}" for v in s))
    assert np.isfinite(l0) and np.isfinite(l1) and l1 < l0
    assert abs(q1[0] - s[0]) < abs(q0[0] - s[0])


def test_quotients_against_float64():
    """op.quotients on fixed functions against the float64 evaluation of the same sums"""
    N1, N2 = 130, 90
    op, A = _cross_operator(N1, N2, 3, 2, seed=51)
    F = lambda x: torch.stack([x[:, 0], x[:, 1] * x[:, 2] + 1.0], 1)  # noqa: E731
    G = lambda y: torch.stack([y[:, 0] + 0.5, y[:, 1] ** 2], 1)  # noqa: E731
    out = op.quotients(F, G)
    F64, G64, A64 = F(op.points_x.double().cpu()).numpy(), G(op.points_y.double().cpu()).numpy(), A.double().numpy()
    nf, ng = (F64 ** 2).sum(0) / N1, (G64 ** 2).sum(0) / N2
    want = np.einsum("il,ij,jl->l", F64, A64, G64) / (N1 * N2) / np.sqrt(nf * ng)
    assert np.abs(out["svals"] - want).max() < 3e-5 * np.abs(want).max()
    assert np.abs(out["norms_f"] / nf - 1).max() < 1e-6 and np.abs(out["norms_g"] / ng - 1).max() < 1e-6


def test_refusals():
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_svd import DenseSvdTrainer, KernelSvdTrainer
    N1, N2, Dx, Dy, L, B = 130, 90, 3, 2, 4, 64
    op, _ = _cross_operator(N1, N2, Dx, Dy, seed=61)
    method, _, _ = _index_method(op, _args(Dx, L, 12, "24,16", True), _args(Dy, L, 12, "24,16", True), 1)
    svd_op = op.get_approx_kernel_svd_op()
    ix, iy = op.sample_indices(B)
    assert ix.dtype == torch.int64 and tuple(ix.shape) == tuple(iy.shape) == (B,)
    assert int(ix.max()) < N1 and int(iy.max()) < N2
    with pytest.raises(NotImplementedError, match="importance"):
        method.compute_loss_kernel_svd(svd_op, ix[:, None], iy[:, None], importance=torch.ones(B, device=DEV))
    with pytest.raises(NsvdError, match="GPU"):
        method.compute_loss_kernel_svd(svd_op, ix.cpu()[:, None], iy[:, None])
    with pytest.raises(NsvdError, match="128"):
        DenseSvdTrainer(op, L=L, m=64, hidden=(64, 64), batch_size=B)
    with pytest.raises(NotImplementedError):
        DenseSvdTrainer(object(), L=L, m=64, batch_size=B)
    with pytest.raises(NotImplementedError):  # the matrix-free trainer keeps refusing what is not matrix-free
        KernelSvdTrainer(op, L=L, m=64, batch_size=B)
    kt = DenseSvdTrainer(op, L=L, m=64, batch_size=B)
    with pytest.raises(NsvdError, match="both"):
        kt.step(ix)
    with pytest.raises(NsvdError, match="both"):
        kt.step(idx_y=iy)
    with pytest.raises(NsvdError, match="index batch"):
        kt.step(ix[:32], iy[:32])
    with pytest.raises(NsvdError, match="index batch"):
        kt.step(ix.cpu(), iy)
    loss, aux = method.compute_loss_kernel_svd(svd_op, ix[:, None], iy[:, None])  # the same without the faults
    assert bool(torch.isfinite(loss)) and tuple(aux["Tg"].shape) == tuple(aux["Tadjf"].shape) == (B, L)
    assert bool(torch.isfinite(kt.step(ix, iy)).all())
