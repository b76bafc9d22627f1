"""GPU tests of the two-sided dot-product kernel operator (nsvd_dot_apply_pair, hip_ops.dot_apply_pair) against its
float64 restatement (tests/_dot_pair_oracle.py), on BOTH outputs. rel = max |got - want| / max |want|; the bound is
max(2e-6, 4 * yardstick), the yardstick being tests/test_dot_apply_gpu.py's: the rel of the same quantity composed in
float32 from library calls on the same GPU (x @ y.T, the map, @ g and .T @ f) against the same oracle. gamma and coef0
are float32 values, so that the oracle sees the inputs the kernel sees.

How a call splits (nsvd_dot_apply_pair_partition; the rule and the slice length are the radial pair's, found by the host
loop in test_partition_reaches_several_parts and asserted there): two row groups from B1 = 65, two column slices from
B2 = 257. B2 = 1030 with B1 = 130 is the multi-part shape: 5 slices in 4 column groups (one owns TWO slices and adds its
second K g tile to its first in memory; the last slice has ONE chunk), 3 x tiles in 2 row groups (one owns two)."""
import numpy as np
import pytest
import torch

from tests import _dot_pair_oracle as P
from tests.test_dot_apply_gpu import VARIANTS, f32, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = (65, 200, 3, 5)  # B1, B2, D, L
B1_SPLIT, B2_SPLIT = 65, 257
B2_MULTI = 1030


def kernel32(x, y, kind, gamma, coef0, degree):
    s = x @ y.T
    if kind == P.POLYNOMIAL:
        return (gamma * s + coef0) ** degree
    p = x.norm(dim=1)[:, None] * y.norm(dim=1)[None, :]
    c = (s / p).clamp(-1.0, 1.0)
    t = torch.acos(c)
    k = p / torch.pi * (torch.sin(t) + (torch.pi - t) * c).clamp(min=0.0)
    return torch.where(p > 0, k, torch.zeros_like(k))


def yardstick(x, y, g, f, kind, gamma, coef0, degree, scale_g, scale_f):
    k = kernel32(x, y, kind, gamma, coef0, degree)
    return scale_g * (k @ g), scale_f * (k.T @ f)


def _shapes():
    b1, b2, d, l = BASE
    s = [(v, b2, d, l) for v in (1, 63, 64, 65, 130)]
    s += [(b1, v, d, l) for v in (1, 63, 64, 65, 130, 200, B2_SPLIT)]
    # D is a contraction length, padded to 8: both sides of every padding step; 17 and 63 are the two sides of the
    # kernel's own boundary between two workgroups per CU (D <= 48) and one
    s += [(b1, b2, v, l) for v in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64)]
    s += [(b1, b2, d, v) for v in (1, 5, 64, 65, 130)]
    s += [(1, 1, 1, 1), (130, B2_MULTI, 64, 130), (B2_MULTI, 130, 64, 130), (1, B2_MULTI, 64, 1), (130, 1, 1, 130),
          (B1_SPLIT, B2_SPLIT, 3, 5)]  # corners
    return sorted(set(s))


def _inputs(B1, B2, D, L):
    gen = torch.Generator().manual_seed(1000 * B1 + 100 * B2 + 10 * D + L)
    x = torch.randn(B1, D, generator=gen).float()
    y = (0.5 * torch.randn(B2, D, generator=gen)).float()  # a cross-domain pair: y half as wide as x
    g = torch.randn(B2, L, generator=gen)
    f = torch.randn(B1, L, generator=gen)
    return x, y, g, f


def _check(x, y, g, f, kind, gamma, coef0, degree, what):
    """both outputs, their float32 yardsticks and the two-call route against the oracle on the SAME float32 inputs;
    returns ((rel_x, yardstick_x), (rel_y, yardstick_y))"""
    from neural_svd_amd import hip_ops as H
    sg, sf = 1.0 / y.shape[0], 1.0 / x.shape[0]
    want = P.dot_kernel_apply_pair(x, y, g, f, kind, gamma, coef0, degree, sg, sf)
    xd, yd, gd, fd = x.to(DEV), y.to(DEV), g.to(DEV), f.to(DEV)
    got = H.dot_apply_pair(xd, yd, gd, fd, kind, gamma, coef0, degree, sg, sf)
    yard = yardstick(xd, yd, gd, fd, kind, gamma, coef0, degree, sg, sf)
    two = (H.dot_apply(xd, yd, gd, kind, gamma, coef0, degree, sg), H.dot_apply(yd, xd, fd, kind, gamma, coef0, degree, sf))
    res = []
    for i, name in enumerate(("out_x", "out_y")):
        e, ey = rel(got[i], want[i]), rel(yard[i], want[i])
        e2 = rel(got[i], two[i])
        bound = max(2e-6, 4.0 * ey)
        print(f"dot_apply_pair {what} {name}: rel {e:.2e} yardstick {ey:.2e} bound {bound:.2e} | vs two calls {e2:.2e}")
        assert bool(torch.isfinite(got[i]).all())
        assert e < bound, (what, name, e, ey, bound)
        assert e2 < bound, (what, name, "two calls", e2, bound)
        res.append((e, ey))
    return res


def test_partition_reaches_several_parts():
    from neural_svd_amd import hip_ops as H
    b1, b2, d, l = BASE
    first_rows = next(B for B in range(1, 4097) if H.dot_apply_pair_partition(B, b2, d, l)[0] >= 2)
    first_cols = next(B for B in range(1, 4097) if H.dot_apply_pair_partition(b1, B, d, l)[1] >= 2)
    assert (first_rows, first_cols) == (B1_SPLIT, B2_SPLIT)
    assert H.dot_apply_pair_partition(B1_SPLIT, B2_SPLIT, d, l) == (2, 2)
    assert H.dot_apply_pair_partition(*BASE) == (2, 1)
    assert H.dot_apply_pair_partition(1, 1, 1, 1) == (1, 1)
    # the multi-part shape: 5 slices in 4 column groups and 3 x tiles in 2 row groups
    assert H.dot_apply_pair_partition(130, B2_MULTI, 64, 130) == (2, 4) == P.pair_split(130, B2_MULTI, 130)
    assert (B2_MULTI + 63) // 64 == 17 and (17 + 3) // 4 == 5 and (130 + 63) // 64 == 3
    # and its mirror: 17 x tiles in 16 row groups (one owns two), one slice of three chunks
    assert H.dot_apply_pair_partition(B2_MULTI, 130, 64, 130) == (16, 1)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B1,B2,D,L", _shapes())
def test_against_float64(B1, B2, D, L, variant):
    """One axis at a time around (65, 200, 3, 5) plus the corners; gamma = 1 / D, coef0 = 1 keep the polynomial's base
    O(1) at every D; both outputs also against two nsvd_dot_apply calls with the arguments swapped."""
    kind, degree = VARIANTS[variant]
    x, y, g, f = _inputs(B1, B2, D, L)
    _check(x, y, g, f, kind, f32(1.0 / D), 1.0, degree, f"{variant} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B2,tail", [(1030, 1), (1100, 2), (1160, 3), (1230, 4)])
def test_every_length_of_the_last_slice(B2, tail, variant):
    """B1 = 130 (one row group stages a successor x tile) and 16 + tail y chunks: five slices in four column groups, so
    one group owns two slices (add-and-store flush), and its last slice has `tail` chunks"""
    from neural_svd_amd import hip_ops as H
    B1, D, L = 130, 5, 65
    assert H.dot_apply_pair_partition(B1, B2, D, L) == (2, 4) and (B2 + 63) // 64 == 16 + tail
    kind, degree = VARIANTS[variant]
    x, y, g, f = _inputs(B1, B2, D, L)
    _check(x, y, g, f, kind, f32(1.0 / D), 1.0, degree, f"{variant} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_both_products_are_fed_the_same_kernel_value(variant):
    """B1 = B2 = 65, g = f = I, scales 1: every sum has one kernel value and exact zeros, so out_x = K and
    out_y = K^T bit for bit if both contractions were fed the same number; again with x is y."""
    from neural_svd_amd import hip_ops as H
    kind, degree = VARIANTS[variant]
    B, D = 65, 3
    gamma = f32(1.0 / D)
    x, y, _, _ = _inputs(B, B, D, B)
    eye = torch.eye(B, device=DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    ox, oy = H.dot_apply_pair(xd, yd, eye, eye, kind, gamma, 1.0, degree, 1.0, 1.0)
    assert torch.equal(oy, ox.T.contiguous())
    want = P.DO.dot_kernel_matrix(x, y, kind, gamma, 1.0, degree)
    e, ey = rel(ox, want), rel(kernel32(xd, yd, kind, gamma, 1.0, degree), want)
    print(f"dot_apply_pair {variant} kernel matrix: rel {e:.2e} yardstick {ey:.2e}")
    assert e < max(2e-6, 4.0 * ey)
    ox, oy = H.dot_apply_pair(xd, xd, eye, eye, kind, gamma, 1.0, degree, 1.0, 1.0)
    assert torch.equal(oy, ox.T.contiguous())
    assert rel(ox, P.DO.dot_kernel_matrix(x, x, kind, gamma, 1.0, degree)) < max(2e-6, 4.0 * ey)


def test_arccos_edge_rows():
    """a zero row in x (row 64 of 65: the second x tile) and a zero row in y: the matching rows of out_x and out_y are
    exactly 0 and nothing is NaN; an antiparallel pair (y_1 = -2 x_0: cos t = -1, the bracket clamps at 0) and a
    parallel one (y_2 = 3 x_1) sit in the same batch, against float64 under the usual bound."""
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 65, 65, 3, 5
    x, y, g, f = _inputs(B1, B2, D, L)
    x[64] = 0.0
    y[7] = 0.0
    y[1] = -2.0 * x[0]
    y[2] = 3.0 * x[1]
    _check(x, y, g, f, P.ARCCOS1, 1.0, 1.0, 2, "arccos1 edge rows")
    xd, yd = x.to(DEV), y.to(DEV)
    ox, oy = H.dot_apply_pair(xd, yd, g.to(DEV), f.to(DEV), P.ARCCOS1, 1.0, 1.0, 2, 1.0, 1.0)
    assert bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oy).all())
    assert bool((ox[64] == 0.0).all()) and bool((oy[7] == 0.0).all())
    # the kernel matrix itself: the zero row and column exactly 0, the antiparallel pair 0 within rounding of the bracket
    K, KT = H.dot_apply_pair(xd, yd, torch.eye(B2, device=DEV), torch.eye(B1, device=DEV), P.ARCCOS1, 1.0, 1.0, 2, 1.0, 1.0)
    assert torch.equal(KT, K.T.contiguous()) and bool(torch.isfinite(K).all())
    assert bool((K[64] == 0.0).all()) and bool((K[:, 7] == 0.0).all()) and float(K.min()) >= 0.0
    nx0 = float(x[0].double().norm())
    assert abs(float(K[0, 1])) <= 1e-5 * 2.0 * nx0 * nx0
    n1 = float(x[1].double().norm())
    assert abs(float(K[1, 2]) - 3.0 * n1 * n1) <= 1e-6 * 3.0 * n1 * n1


def test_overflowing_kernel_values_stay_in_their_rows():
    """polynomial, coef0 = 1e30, degree 2: every kernel value is +inf. B1 = B2 = 8 leaves 56 padded rows on each side,
    whose kernel values the kernel must force to 0 (inf * 0 from the zero padding of g^T and f^T would be NaN); with
    g = f = ones both outputs are all +inf and nothing is NaN."""
    from neural_svd_amd import hip_ops as H
    B, D, L = 8, 3, 5
    x, y, _, _ = _inputs(B, B, D, L)
    ones = torch.ones(B, L, device=DEV)
    ox, oy = H.dot_apply_pair(x.to(DEV), y.to(DEV), ones, ones, P.POLYNOMIAL, 1.0, 1e30, 2, 1.0, 1.0)
    for got in (ox, oy):
        assert not bool(torch.isnan(got).any())
        assert bool((got == float("inf")).all()), got


def test_two_calls_give_the_same_bits():
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, B2_MULTI, 16, 65
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    for kind in (P.POLYNOMIAL, P.ARCCOS1):
        a = H.dot_apply_pair(x, y, g, f, kind, 0.25, 1.0, 3, 1.0 / B2, 1.0 / B1)
        b = H.dot_apply_pair(x, y, g, f, kind, 0.25, 1.0, 3, 1.0 / B2, 1.0 / B1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ws = H.dot_apply_pair_workspace(B1, B2, D, L, DEV)
        ox, oy = torch.empty_like(a[0]), torch.empty_like(a[1])
        r = H.dot_apply_pair(x, y, g, f, kind, 0.25, 1.0, 3, 1.0 / B2, 1.0 / B1, ws=ws, out_x=ox, out_y=oy)
        assert r[0] is ox and r[1] is oy and torch.equal(ox, a[0]) and torch.equal(oy, a[1])


def test_workspace_contents_do_not_matter():
    """a workspace of 0xFF bytes (NaNs) against a zero-filled one: equal bits, finite"""
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, B2_MULTI, 5, 65
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    ws = H.dot_apply_pair_workspace(B1, B2, D, L, DEV)
    outs = []
    for fill in (0xFF, 0x00):
        ws.fill_(fill)
        ox, oy = H.dot_apply_pair(x, y, g, f, P.ARCCOS1, 1.0, 1.0, 2, 1.0 / B2, 1.0 / B1, ws=ws)
        assert bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oy).all())
        outs.append((ox, oy))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_outputs_and_workspace_stay_inside_their_buffers():
    """both outputs and the workspace sit inside larger buffers with 256 sentinel words on each side"""
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, B2_MULTI, 3, 65
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    bx = torch.full((512 + B1 * L,), -7.0, device=DEV)
    by = torch.full((512 + B2 * L,), -7.0, device=DEV)
    ox, oy = bx[256:256 + B1 * L].view(B1, L), by[256:256 + B2 * L].view(B2, L)
    nws = H.dot_apply_pair_workspace(B1, B2, D, L, "meta").numel()
    assert nws % 256 == 0
    bw = torch.full((2048 + nws,), 0xA5, dtype=torch.uint8, device=DEV)  # 256 words = 1024 bytes a side
    off = (-bw.data_ptr()) % 256 + 1024
    ws = bw[off:off + nws]
    assert ws.data_ptr() % 256 == 0 and off + nws + 1024 <= bw.numel()
    H.dot_apply_pair(x, y, g, f, P.POLYNOMIAL, 0.5, 1.0, 2, 1.0 / B2, 1.0 / B1, ws=ws, out_x=ox, out_y=oy)
    torch.cuda.synchronize()
    for buf in (bx, by):
        assert bool((buf[:256] == -7.0).all()) and bool((buf[-256:] == -7.0).all())
    assert bool((bw[:off] == 0xA5).all()) and bool((bw[off + nws:] == 0xA5).all())
    want = H.dot_apply_pair(x, y, g, f, P.POLYNOMIAL, 0.5, 1.0, 2, 1.0 / B2, 1.0 / B1)
    assert torch.equal(ox, want[0]) and torch.equal(oy, want[1])


def test_refusals_leave_both_outputs_untouched():
    from neural_svd_amd import _lib, hip_ops as H
    from neural_svd_amd._lib import NsvdError
    B1, B2, D, L = BASE
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    ox, oy = torch.full((B1, L), 7.0, device=DEV), torch.full((B2, L), 7.0, device=DEV)
    ws = H.dot_apply_pair_workspace(B1, B2, D, L, DEV)
    POLY = P.POLYNOMIAL

    def call(*a, **k):
        return H.dot_apply_pair(*a, out_x=ox, out_y=oy, **k)
    with pytest.raises(NsvdError, match="invalid"):  # unknown kind
        call(x, y, g, f, 2, 1.0, 1.0, 2, 1.0, 1.0)
    for degree in (0, 9):
        with pytest.raises(NsvdError, match="invalid"):
            call(x, y, g, f, POLY, 1.0, 1.0, degree, 1.0, 1.0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(NsvdError, match="invalid"):
            call(x, y, g, f, POLY, bad, 1.0, 2, 1.0, 1.0)
        with pytest.raises(NsvdError, match="invalid"):
            call(x, y, g, f, POLY, 1.0, bad, 2, 1.0, 1.0)
    with pytest.raises(NsvdError, match="invalid"):  # short workspace
        call(x, y, g, f, POLY, 1.0, 1.0, 2, 1.0, 1.0, ws=ws[:ws.numel() - 256])
    with pytest.raises(NsvdError, match="invalid"):  # misaligned workspace
        call(x, y, g, f, POLY, 1.0, 1.0, 2, 1.0, 1.0,
             ws=torch.empty(ws.numel() + 256, dtype=torch.uint8, device=DEV)[4:])
    x65, y65 = torch.zeros(B1, 65, device=DEV), torch.zeros(B2, 65, device=DEV)
    with pytest.raises(NsvdError, match="unsupported"):
        call(x65, y65, g, f, POLY, 1.0, 1.0, 2, 1.0, 1.0)
    with pytest.raises(NsvdError, match="unsupported"):
        H.dot_apply_pair_workspace(B1, B2, 65, L, DEV)
    with pytest.raises(NsvdError, match="unsupported"):
        H.dot_apply_pair_partition(B1, B2, 65, L)
    with pytest.raises(NsvdError):  # shapes that do not belong together
        call(x, y, g, f[:-1], POLY, 1.0, 1.0, 2, 1.0, 1.0)
    with pytest.raises(NsvdError):
        call(x, y[:-1], g, f, POLY, 1.0, 1.0, 2, 1.0, 1.0)
    # null pointers, non-positive sizes and aliased outputs cannot come through the tensor wrapper: the C entry point
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = dict(x=x.data_ptr(), y=y.data_ptr(), g=g.data_ptr(), f=f.data_ptr(), out_x=ox.data_ptr(),
                out_y=oy.data_ptr(), ws=ws.data_ptr())

    def raw(p, b1=B1, b2=B2, d=D, l=L):
        return lib.nsvd_dot_apply_pair(p["x"], b1, p["y"], b2, d, p["g"], p["f"], l, POLY, 1.0, 1.0, 2, 1.0, 1.0,
                                       p["out_x"], p["out_y"], p["ws"], ws.numel(), stream)
    for null in ptrs:
        with pytest.raises(NsvdError, match="invalid"):
            _lib.check(raw(dict(ptrs, **{null: None})), f"nsvd_dot_apply_pair({null} = NULL)")
    for sizes in (dict(b1=0), dict(b2=0), dict(d=0), dict(l=0), dict(b1=-1)):
        with pytest.raises(NsvdError, match="invalid"):
            _lib.check(raw(ptrs, **sizes), f"nsvd_dot_apply_pair({sizes})")
    assert B2 > B1
    for alias in (dict(out_x=oy.data_ptr()), dict(out_y=ox.data_ptr()),            # the outputs on each other
                  dict(out_x=oy.data_ptr(), out_y=oy.data_ptr() + 4 * L * (B1 - 1)),  # ... sharing one row
                  dict(out_y=g.data_ptr()), dict(out_x=f.data_ptr())):               # an output on an input
        with pytest.raises(NsvdError, match="invalid"):
            _lib.check(raw(dict(ptrs, **alias)), f"nsvd_dot_apply_pair({list(alias)} aliased)")
    with pytest.raises(NsvdError, match="GPU"):
        call(x.cpu(), y, g, f, POLY, 1.0, 1.0, 2, 1.0, 1.0)
    torch.cuda.synchronize()
    assert bool((ox == 7.0).all()) and bool((oy == 7.0).all())
    # and the same arguments without the faults are accepted; x may be y and f may be g
    call(x, y, g, f, POLY, 1.0, 1.0, 2, 1.0, 1.0, ws=ws)
    assert not bool((ox == 7.0).any()) and not bool((oy == 7.0).any())
    sq = H.dot_apply_pair(y, y, g, g, P.ARCCOS1, 1.0, 1.0, 2, 1.0, 1.0)
    assert bool(torch.isfinite(sq[0]).all()) and bool(torch.isfinite(sq[1]).all())
