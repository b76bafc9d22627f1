"""GPU, two devices: kernels that ask for more than 64 KiB of dynamic LDS launch on a SECOND device of the process.

The dynamic-LDS limit of such a kernel is raised once per device and kernel on first use (csrc/nsvd_common.h,
nsvd_lds_opt_in); before, most launch sites raised it once per process, on whichever device came first. One call from
each of three families runs on cuda:0 and then on cuda:1 in this process, on the same seeded inputs:

- a matrix-free product, H.dot_apply at B1 = B2 = 64, D = 3, L = 4: dot_lds_bytes(Dp = 8) =
  (17408 + 2 (64 (8 + 4) + 64)) 4 = 76 288 bytes;
- the CDK loss forward at B = 64, L = 8: TILE_FLOATS 4 = 17408 x 4 = 69 632 bytes;
- the SpIN solve at L = 46, the smallest size above 64 KiB by solve_lds_bytes(L) = (4 L (L | 1) + 2 L) 8:
  69 920 bytes (L = 45: 65 520).

The kernels use no atomics and the launches do not depend on the device: the results of cuda:1 equal those of cuda:0
bit for bit. Skipped where fewer than two devices are visible.

A second test calls three wrappers with their tensors on cuda:1 while cuda:0 is the current device (the device guard
of neural_svd_amd/hip_ops.py), at the smallest shapes that reach their kernels."""
import pytest
import torch

DOT_LDS_BYTES = (17408 + 2 * (64 * (8 + 4) + 64)) * 4
CDK_LDS_BYTES = 17408 * 4
SPIN_L = 46


def _spin_lds_bytes(L):
    return (4 * L * (L | 1) + 2 * L) * 8


def _dot(dev):
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(1)
    x, y, f = (torch.randn(s, generator=g).to(dev) for s in ((64, 3), (64, 3), (64, 4)))
    return [H.dot_apply(x, y, f, H.DOT_POLYNOMIAL, 0.5, 1.0, 3, 1.0 / 64)]


def _cdk(dev):
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(2)
    B, L = 64, 8
    f, gg = torch.randn(B, L, generator=g).to(dev), torch.randn(B, L, generator=g).to(dev)
    v = torch.ones(L + 1).to(dev)
    M = torch.tril(torch.ones(L + 1, L + 1)).to(dev)
    ws = H.cdk_workspace(B, L, True, dev)
    loss = torch.empty(3, device=dev)
    rj, ri = torch.empty(B, device=dev), torch.empty(B * (B - 1), device=dev)
    H.cdk_loss_forward(f, gg, None, v, M, True, loss, rj, ri, ws)
    return [loss, rj, ri]


def _spin(dev):
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(3)
    L, f64 = SPIN_L, torch.float64
    n, B1 = 4 * L + 3, 2 * L + 1
    X = torch.randn(n, L, generator=g, dtype=f64)
    Y, Z = torch.randn(B1, L, generator=g, dtype=f64), torch.randn(B1, L, generator=g, dtype=f64)
    state = torch.zeros((L, L), dtype=torch.float32, device=dev)
    chol = torch.empty_like(state)
    le = torch.empty(L + 1, dtype=f64, device=dev)
    gs, gp = torch.empty((L, L), dtype=f64, device=dev), torch.empty((L, L), dtype=f64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    H.spin_solve((X.T @ X).to(dev), 1.0 / n, (Y.T @ Z).to(dev), 1.0 / B1, 0.01, 1.0 / B1, state, chol, le, gs, gp, status)
    return [state, chol, le, gs, gp, status]


def _rbf_pair(dev):
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(4)
    x, y, gg, f = (torch.randn(s, generator=g).to(dev) for s in ((64, 3), (64, 3), (64, 4), (64, 4)))
    return list(H.rbf_apply_pair(x, y, gg, f, H.RBF_GAUSSIAN, 1.5, 1.0 / 64, 1.0 / 64))


def _gather_heads(dev):
    from neural_svd_amd import hip_ops as H
    W, B, Ll = 2, 32, 2
    gath = torch.randn(W, 2, B, Ll, generator=torch.Generator().manual_seed(5)).to(dev)
    f, Tf = torch.empty(B, W * Ll, device=dev), torch.empty(B, W * Ll, device=dev)
    scratch = H.evd_scratch(B, W * Ll, dev).zero_()
    H.evd_gather_heads(gath, f, Tf, H.MASK_SEQUENTIAL, None, scratch)
    return [f, Tf, scratch]


def _gather_head_blocks(dev):
    from neural_svd_amd import hip_ops as H
    W, B, L = 2, 32, 3  # rank 0 holds two heads, rank 1 one: its block's tail is never read
    gath = torch.randn(W, 2 * B * 2, generator=torch.Generator().manual_seed(6))
    gath[1, 2 * B:] = float("nan")
    gath = gath.to(dev)
    f, Tf = torch.empty(B, L, device=dev), torch.empty(B, L, device=dev)
    scratch = H.evd_scratch(B, L, dev).zero_()
    H.evd_gather_head_blocks(gath, L, f, Tf, H.MASK_SEQUENTIAL, None, scratch)
    return [f, Tf, scratch]


def test_lds_byte_counts():
    assert DOT_LDS_BYTES == 76288 and CDK_LDS_BYTES == 69632
    assert _spin_lds_bytes(SPIN_L - 1) == 65520 <= 64 * 1024 < _spin_lds_bytes(SPIN_L) == 69920


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")
@pytest.mark.parametrize("family", ["dot_apply", "cdk_loss_forward", "spin_solve"])
def test_second_device_matches_first(family):
    run = dict(dot_apply=_dot, cdk_loss_forward=_cdk, spin_solve=_spin)[family]
    outs = []
    for i in (0, 1):
        dev = torch.device("cuda", i)
        with torch.cuda.device(dev):
            res = run(dev)
            torch.cuda.synchronize(dev)
        outs.append([t.cpu() for t in res])
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a.double()).all())
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")
@pytest.mark.parametrize("wrapper", ["rbf_apply_pair", "evd_gather_heads", "evd_gather_head_blocks"])
def test_tensors_off_the_current_device_launch_where_they_live(wrapper):
    """The device guard (hip_ops._on_tensor_device) on the three wrappers that lacked it: with the tensors on cuda:1
    while cuda:0 is current, the call takes a stream of cuda:1 and gives, bit for bit, what the same call gives with
    cuda:1 current (before, it handed the library a stream of cuda:0)."""
    run = dict(rbf_apply_pair=_rbf_pair, evd_gather_heads=_gather_heads, evd_gather_head_blocks=_gather_head_blocks)[wrapper]
    dev, outs = torch.device("cuda", 1), []
    for current in (1, 0):
        with torch.cuda.device(current):
            res = run(dev)
            assert torch.cuda.current_device() == current
        torch.cuda.synchronize(dev)
        outs.append([t.cpu() for t in res])
    for a, b in zip(*outs):
        assert a.dtype == torch.uint8 or bool(torch.isfinite(a).all())
        assert torch.equal(a, b)
