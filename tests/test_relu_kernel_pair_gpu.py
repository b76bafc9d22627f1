"""GPU tests of the deep ReLU kinds of the two-sided dot-product kernel operator (nsvd_dot_apply_pair with
NSVD_DOT_RELU_NNGP / NSVD_DOT_RELU_NTK, hip_ops.dot_apply_pair) against their float64 restatement
(tests/_relu_kernel_oracle.py) on BOTH outputs, and against the two one-sided calls. rel = max |got - want| / max |want|;
the bound is max(2e-6, 4 * yardstick), the yardstick being the same quantity composed in float32 from library calls on
the same GPU (_relu_kernel_oracle.relu_kernel_matrix32, @ g and .T @ f). The axis values are those of
tests/test_dot_apply_pair_gpu.py: two row groups from B1 = 65, two column slices from B2 = 257, and B2 = 1030 with
B1 = 130 is the multi-part shape (5 slices in 4 column groups, 3 x tiles in 2 row groups)."""
import numpy as np
import pytest
import torch

from tests import _relu_kernel_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"nngp": R.RELU_NNGP, "ntk": R.RELU_NTK}
BASE = (65, 200, 3, 5)  # B1, B2, D, L
DEPTH, GAMMA, COEF0 = 3, 2.0, float(np.float32(0.1))
B1_SPLIT, B2_SPLIT = 65, 257
B2_MULTI = 1030


def rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _shapes():
    b1, b2, d, l = BASE
    s = [(v, b2, d, l) for v in (1, 64, 65, 130)]
    s += [(b1, v, d, l) for v in (1, 63, 64, 65, 130, B2_SPLIT)]
    # 17 and 64 are the two sides of the kernel's own boundary between two workgroups per CU (D <= 48) and one
    s += [(b1, b2, v, l) for v in (2, 3, 8, 9, 17, 64)]
    s += [(b1, b2, d, v) for v in (1, 64, 65, 130)]
    s += [(130, B2_MULTI, 64, 130), (B2_MULTI, 130, 64, 130), (B1_SPLIT, B2_SPLIT, 3, 5)]  # corners
    return sorted(set(s))


def _inputs(B1, B2, D, L):
    gen = torch.Generator().manual_seed(1000 * B1 + 100 * B2 + 10 * D + L)
    x = torch.randn(B1, D, generator=gen).float()
    y = (0.5 * torch.randn(B2, D, generator=gen)).float()  # a cross-domain pair: y half as wide as x
    g = torch.randn(B2, L, generator=gen)
    f = torch.randn(B1, L, generator=gen)
    return x, y, g, f


def _check(x, y, g, f, kind, gamma, coef0, depth, what):
    """both outputs, their float32 yardsticks and the two-call route against the oracle on the SAME float32 inputs"""
    from neural_svd_amd import hip_ops as H
    sg, sf = 1.0 / y.shape[0], 1.0 / x.shape[0]
    want = R.relu_kernel_apply_pair(x, y, g, f, kind, gamma, coef0, depth, sg, sf)
    xd, yd, gd, fd = x.to(DEV), y.to(DEV), g.to(DEV), f.to(DEV)
    got = H.dot_apply_pair(xd, yd, gd, fd, kind, gamma, coef0, depth, sg, sf)
    k32 = R.relu_kernel_matrix32(xd, yd, kind, gamma, coef0, depth)
    yard = (sg * (k32 @ gd), sf * (k32.T @ fd))
    two = (H.dot_apply(xd, yd, gd, kind, gamma, coef0, depth, sg), H.dot_apply(yd, xd, fd, kind, gamma, coef0, depth, sf))
    for i, name in enumerate(("out_x", "out_y")):
        e, ey = rel(got[i], want[i]), rel(yard[i], want[i])
        e2 = rel(got[i], two[i])
        bound = max(2e-6, 4.0 * ey)
        print(f"relu dot_apply_pair {what} {name}: rel {e:.2e} yardstick {ey:.2e} bound {bound:.2e} | vs two calls {e2:.2e}")
        assert bool(torch.isfinite(got[i]).all())
        assert e < bound, (what, name, e, ey, bound)
        assert e2 < bound, (what, name, "two calls", e2, bound)
    return got


def test_partition_of_the_shapes_used():
    from neural_svd_amd import hip_ops as H
    b1, b2, d, l = BASE
    assert H.dot_apply_pair_partition(B1_SPLIT, B2_SPLIT, d, l) == (2, 2)
    assert H.dot_apply_pair_partition(*BASE) == (2, 1)
    assert H.dot_apply_pair_partition(130, B2_MULTI, 64, 130) == (2, 4)
    assert H.dot_apply_pair_partition(B2_MULTI, 130, 64, 130) == (16, 1)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B1,B2,D,L", _shapes())
def test_against_float64(B1, B2, D, L, kind):
    """depth 3, (gamma, coef0) = (2, 0.1), one axis at a time around (65, 200, 3, 5) plus the corners; both outputs
    also against two nsvd_dot_apply calls with the arguments swapped"""
    x, y, g, f = _inputs(B1, B2, D, L)
    _check(x, y, g, f, KINDS[kind], GAMMA, COEF0, DEPTH, f"{kind} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("gamma,coef0", ((1.0, 0.0), (0.5, 1.0)))
@pytest.mark.parametrize("depth", (1, 2, 8))
def test_depths_and_variances(depth, gamma, coef0, kind):
    x, y, g, f = _inputs(*BASE)
    _check(x, y, g, f, KINDS[kind], gamma, coef0, depth, f"{kind} depth={depth} gamma={gamma} coef0={coef0}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_both_products_are_fed_the_same_kernel_value(kind):
    """B1 = B2 = 65, g = f = I, scales 1: every sum has one kernel value and exact zeros, so out_x = K and
    out_y = K^T bit for bit if both contractions were fed the same number - and if the 63 padded rows of either side
    (coef0-derived values, not 0) stayed out; again with x is y"""
    from neural_svd_amd import hip_ops as H
    B, D = 65, 3
    x, y, _, _ = _inputs(B, B, D, B)
    eye = torch.eye(B, device=DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    ox, oy = H.dot_apply_pair(xd, yd, eye, eye, KINDS[kind], GAMMA, COEF0, DEPTH, 1.0, 1.0)
    assert torch.equal(oy, ox.T.contiguous())
    want = R.relu_kernel_matrix(x, y, KINDS[kind], GAMMA, COEF0, DEPTH)
    e, ey = rel(ox, want), rel(R.relu_kernel_matrix32(xd, yd, KINDS[kind], GAMMA, COEF0, DEPTH), want)
    print(f"relu dot_apply_pair {kind} kernel matrix: rel {e:.2e} yardstick {ey:.2e}")
    assert e < max(2e-6, 4.0 * ey)
    ox, oy = H.dot_apply_pair(xd, xd, eye, eye, KINDS[kind], GAMMA, COEF0, DEPTH, 1.0, 1.0)
    assert torch.equal(oy, ox.T.contiguous())


@pytest.mark.parametrize("kind", list(KINDS))
def test_padded_rows_of_both_sides_are_not_seen(kind):
    """B1 = B2 = 8 leaves 56 padded rows on each side, whose kernel values are coef0-derived (coef0 = 1: of the size of
    every other). With g = f = ones a seen padded row would add its value to every sum."""
    x, y, _, _ = _inputs(8, 8, 3, 5)
    ones = torch.ones(8, 5)
    _check(x, y, ones, ones, KINDS[kind], GAMMA, 1.0, DEPTH, f"{kind} padded rows")
    x, y, _, _ = _inputs(65, 65, 3, 5)
    ones = torch.ones(65, 5)
    _check(x, y, ones, ones, KINDS[kind], GAMMA, 1.0, DEPTH, f"{kind} padded rows, second tile")


@pytest.mark.parametrize("kind", list(KINDS))
def test_zero_rows(kind):
    """a zero row in x (row 64 of 65: the second x tile) and a zero row in y: finite, the oracle's values; with
    coef0 = 0 the matching rows of out_x and out_y are exactly 0"""
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 65, 65, 3, 5
    x, y, g, f = _inputs(B1, B2, D, L)
    x[64] = 0.0
    y[7] = 0.0
    _check(x, y, g, f, KINDS[kind], GAMMA, COEF0, DEPTH, f"{kind} zero rows")
    ox, oy = _check(x, y, g, f, KINDS[kind], 1.0, 0.0, DEPTH, f"{kind} zero rows, coef0 = 0")
    assert bool((ox[64] == 0.0).all()) and bool((oy[7] == 0.0).all())
    K, KT = H.dot_apply_pair(x.to(DEV), y.to(DEV), torch.eye(B2, device=DEV), torch.eye(B1, device=DEV), KINDS[kind],
                             GAMMA, COEF0, 1, 1.0, 1.0)
    assert torch.equal(KT, K.T.contiguous()) and bool(torch.isfinite(K).all())
    assert bool((K[64] == COEF0).all()) and bool((K[:, 7] == COEF0).all())


def test_two_calls_give_the_same_bits():
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, B2_MULTI, 16, 65
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    for kind in KINDS.values():
        a = H.dot_apply_pair(x, y, g, f, kind, GAMMA, COEF0, DEPTH, 1.0 / B2, 1.0 / B1)
        b = H.dot_apply_pair(x, y, g, f, kind, GAMMA, COEF0, DEPTH, 1.0 / B2, 1.0 / B1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ws = H.dot_apply_pair_workspace(B1, B2, D, L, DEV)
        ws.fill_(0xFF)
        ox, oy = torch.empty_like(a[0]), torch.empty_like(a[1])
        r = H.dot_apply_pair(x, y, g, f, kind, GAMMA, COEF0, DEPTH, 1.0 / B2, 1.0 / B1, ws=ws, out_x=ox, out_y=oy)
        assert r[0] is ox and r[1] is oy and torch.equal(ox, a[0]) and torch.equal(oy, a[1])


def test_refusals_leave_both_outputs_untouched():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    B1, B2, D, L = BASE
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    ox, oy = torch.full((B1, L), 7.0, device=DEV), torch.full((B2, L), 7.0, device=DEV)
    nan, inf = float("nan"), float("inf")

    def call(*a, **k):
        return H.dot_apply_pair(*a, out_x=ox, out_y=oy, **k)
    for kind in KINDS.values():
        for gamma, coef0, depth in ((1.0, 0.0, 0), (1.0, 0.0, 9), (1.0, 0.0, -1), (0.0, 0.0, 3), (-1.0, 0.0, 3),
                                    (nan, 0.0, 3), (inf, 0.0, 3), (1.0, -0.5, 3), (1.0, nan, 3), (1.0, inf, 3)):
            with pytest.raises(NsvdError, match="invalid"):
                call(x, y, g, f, kind, gamma, coef0, depth, 1.0, 1.0)
    for kind in (2, 5):  # 2 stays unassigned
        with pytest.raises(NsvdError, match="invalid"):
            call(x, y, g, f, kind, 1.0, 0.0, 3, 1.0, 1.0)
    torch.cuda.synchronize()
    assert bool((ox == 7.0).all()) and bool((oy == 7.0).all())
    for kind in KINDS.values():
        ox.fill_(7.0), oy.fill_(7.0)
        call(x, y, g, f, kind, 1.0, 0.0, 8, 1.0, 1.0)
        assert not bool((ox == 7.0).any()) and not bool((oy == 7.0).any())
        assert bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oy).all())
