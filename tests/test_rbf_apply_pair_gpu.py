"""GPU tests of the two-sided radial kernel operator (nsvd_rbf_apply_pair, hip_ops.rbf_apply_pair) against its float64
restatement (tests/_pair_oracle.py), on BOTH outputs. rel = max |got - want| / max |want|; the bound is
max(2e-6, 4 * yardstick), the yardstick being tests/test_rbf_apply_gpu.py's: the rel of the same quantity composed in
float32 on the same GPU from direct differences (K @ g and K.T @ f) against the same oracle.

How a call splits (nsvd_rbf_apply_pair_partition; found by the host loop in test_partition_reaches_several_parts and
asserted there): two row groups from B1 = 65 (two 64-row x tiles), two column slices from B2 = 257 (five 64-row chunks:
two slices of at most four). B2_SPLIT = 1030 (17 chunks, 5 slices in 4 column groups: the last group owns TWO slices and
adds its second K g tile to its first in memory, its last slice has ONE chunk) with B1 = 130 (3 x tiles in 2 row groups:
one owns a run of two) is the multi-part shape."""
import pytest
import torch

from tests import _pair_oracle as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"gaussian": P.GAUSSIAN, "exponential": P.EXPONENTIAL}
BASE = (65, 200, 3, 5)  # B1, B2, D, L
B1_SPLIT, B2_SPLIT = 65, 257
B2_MULTI = 1030


def rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def yardstick(x, y, g, f, kind, ell, scale_g, scale_f):
    d2 = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    k = torch.exp(-d2 / (2.0 * ell ** 2)) if kind == P.GAUSSIAN else torch.exp(-d2.sqrt() / ell)
    return scale_g * (k @ g), scale_f * (k.T @ f)


def _shapes():
    b1, b2, d, l = BASE
    s = [(v, b2, d, l) for v in (1, 63, 64, 65, 130)]              # B1 < B2
    s += [(b1, v, d, l) for v in (1, 63, 64, 65, 130, 200, B2_SPLIT)]  # B1 > B2 below 65
    s += [(b1, b2, v, l) for v in (1, 2, 3, 4, 5, 16, 17, 64)]
    s += [(b1, b2, d, v) for v in (1, 5, 64, 65, 130)]
    s += [(1, 1, 1, 1), (130, B2_MULTI, 64, 130), (B2_MULTI, 130, 64, 130), (1, B2_MULTI, 64, 1), (130, 1, 1, 130),
          (B1_SPLIT, B2_SPLIT, 3, 5)]  # corners
    return sorted(set(s))


def _inputs(B1, B2, D, L, shift=0.0):
    gen = torch.Generator().manual_seed(1000 * B1 + 100 * B2 + 10 * D + L)
    x = (torch.randn(B1, D, generator=gen) + shift).float()
    y = (0.5 * torch.randn(B2, D, generator=gen) + shift).float()
    g = torch.randn(B2, L, generator=gen)
    f = torch.randn(B1, L, generator=gen)
    return x, y, g, f


def _check(x, y, g, f, kind, ell, what, bounds=None):
    """both outputs and their float32 yardsticks against the oracle on the SAME float32 inputs;
    returns ((rel_x, yardstick_x), (rel_y, yardstick_y))"""
    from neural_svd_amd import hip_ops as H
    sg, sf = 1.0 / y.shape[0], 1.0 / x.shape[0]
    want = P.radial_kernel_apply_pair(x, y, g, f, kind, ell, sg, sf)
    xd, yd, gd, fd = x.to(DEV), y.to(DEV), g.to(DEV), f.to(DEV)
    got = H.rbf_apply_pair(xd, yd, gd, fd, kind, ell, sg, sf)
    yard = yardstick(xd, yd, gd, fd, kind, ell, sg, sf)
    res = []
    for i, name in enumerate(("out_x", "out_y")):
        e, ey = rel(got[i], want[i]), rel(yard[i], want[i])
        bound = max(2e-6, 4.0 * ey) if bounds is None else bounds[i]
        print(f"rbf_apply_pair {what} {name}: rel {e:.2e} yardstick {ey:.2e} bound {bound:.2e}")
        assert bool(torch.isfinite(got[i]).all())
        assert e < bound, (what, name, e, ey, bound)
        res.append((e, ey))
    return res


def test_partition_reaches_several_parts():
    from neural_svd_amd import hip_ops as H
    b1, b2, d, l = BASE
    first_rows = next(B for B in range(1, 4097) if H.rbf_apply_pair_partition(B, b2, d, l)[0] >= 2)
    first_cols = next(B for B in range(1, 4097) if H.rbf_apply_pair_partition(b1, B, d, l)[1] >= 2)
    assert (first_rows, first_cols) == (B1_SPLIT, B2_SPLIT)
    assert H.rbf_apply_pair_partition(B1_SPLIT, B2_SPLIT, d, l) == (2, 2)
    assert H.rbf_apply_pair_partition(*BASE) == (2, 1)
    assert H.rbf_apply_pair_partition(1, 1, 1, 1) == (1, 1)
    # the multi-part shape: fewer column groups than slices and fewer row groups than x tiles
    assert H.rbf_apply_pair_partition(130, B2_MULTI, 16, 65) == (2, 4) and P.pair_split(130, B2_MULTI, 65) == (2, 4)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B1,B2,D,L", _shapes())
def test_against_float64(B1, B2, D, L, kind):
    """One axis at a time around (65, 200, 3, 5) plus the corners; ell = sqrt(D) keeps the kernel values O(1) at every
    D; y is drawn half as wide as x (a cross-domain pair)."""
    x, y, g, f = _inputs(B1, B2, D, L)
    _check(x, y, g, f, KINDS[kind], float(D) ** 0.5, f"{kind} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B2,tail", [(1030, 1), (1100, 2), (1160, 3), (1230, 4)])
def test_every_length_of_the_last_slice(B2, tail, kind):
    """B1 = 130 (one row group stages a successor x tile) and 16 + tail y chunks: five slices in four column groups, so
    one group owns two slices (add-and-store flush), and its last slice has `tail` chunks"""
    from neural_svd_amd import hip_ops as H
    B1, D, L = 130, 5, 65
    assert H.rbf_apply_pair_partition(B1, B2, D, L) == (2, 4) and (B2 + 63) // 64 == 16 + tail
    x, y, g, f = _inputs(B1, B2, D, L)
    _check(x, y, g, f, KINDS[kind], float(D) ** 0.5, f"{kind} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_same_tensors_on_both_sides(kind):
    """x is y and f is g (the same tensors): K is symmetric, so the two outputs are the same quantity - they agree
    within the bound of either against float64 (their sums run in different orders)."""
    from neural_svd_amd import hip_ops as H
    B, D, L = 130, 3, 5
    x, _, g, _ = _inputs(B, B, D, L)
    (ex, yx), (ey, yy) = _check(x, x, g, g, KINDS[kind], 1.3, f"{kind} x is y, f is g")
    xd, gd = x.to(DEV), g.to(DEV)
    ox, oy = H.rbf_apply_pair(xd, xd, gd, gd, KINDS[kind], 1.3, 1.0 / B, 1.0 / B)
    e = rel(oy, ox)
    bound = max(2e-6, 4.0 * max(yx, yy))
    print(f"rbf_apply_pair {kind} out_y against out_x: rel {e:.2e} bound {bound:.2e}")
    assert e < bound


@pytest.mark.parametrize("kind", list(KINDS))
def test_both_products_are_fed_the_same_kernel_value(kind):
    """B1 = B2 = 65, g = f = I, scales 1: every sum has one kernel value and exact zeros, so out_x = K and
    out_y = K^T bit for bit if both contractions were fed the same number. out_x itself is the kernel matrix (checked as
    tests/test_rbf_apply_gpu.py:test_kernel_matrix_itself does, with x is y)."""
    from neural_svd_amd import hip_ops as H
    B, D = 65, 3
    x, y, _, _ = _inputs(B, B, D, B)
    eye = torch.eye(B, device=DEV)
    ox, oy = H.rbf_apply_pair(x.to(DEV), y.to(DEV), eye, eye, KINDS[kind], 1.3, 1.0, 1.0)
    assert torch.equal(oy, ox.T.contiguous())
    want = P.R.radial_kernel_matrix(x, y, KINDS[kind], 1.3)
    yard = yardstick(x.to(DEV), y.to(DEV), eye, eye, KINDS[kind], 1.3, 1.0, 1.0)[0]
    e, ey = rel(ox, want), rel(yard, want)
    print(f"rbf_apply_pair {kind} kernel matrix: rel {e:.2e} yardstick {ey:.2e}")
    assert e < max(2e-6, 4.0 * ey)
    xd = x.to(DEV)
    ox, oy = H.rbf_apply_pair(xd, xd, eye, eye, KINDS[kind], 1.3, 1.0, 1.0)
    assert torch.equal(oy, ox.T.contiguous())
    assert float((ox.diagonal() - 1.0).abs().max()) <= 1e-6
    assert float(ox.max()) <= 1.0 + 1e-6 and float(ox.min()) >= 0.0


@pytest.mark.parametrize("kind", list(KINDS))
def test_far_rows_give_exact_zeros(kind):
    from neural_svd_amd import hip_ops as H
    x = torch.zeros(2, 3)
    x[1, 0] = 1e3
    xd, eye2 = x.to(DEV), (2.0 * torch.eye(2)).to(DEV)
    ox, oy = H.rbf_apply_pair(xd, xd, eye2, eye2, KINDS[kind], 1.0, 0.5, 0.5)
    for got in (ox, oy):
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got.cpu(), torch.eye(2)), got


def test_shifted_points_meet_the_unshifted_bound():
    """D = 16, ell = 1, every coordinate shifted by +100: the distances come from direct differences, so the shifted
    case meets the bound of the unshifted one, on both outputs."""
    B1, B2, D, L = 65, 200, 16, 5
    x, y, g, f = _inputs(B1, B2, D, L)
    r = _check(x, y, g, f, P.GAUSSIAN, 1.0, "unshifted D=16 ell=1")
    bounds = [max(2e-6, 4.0 * ey) for _, ey in r]
    xs, ys, _, _ = _inputs(B1, B2, D, L, shift=100.0)
    _check(xs, ys, g, f, P.GAUSSIAN, 1.0, "shifted +100 D=16 ell=1", bounds=bounds)


def test_two_calls_give_the_same_bits():
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, B2_MULTI, 16, 65
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    a = H.rbf_apply_pair(x, y, g, f, P.GAUSSIAN, 4.0, 1.0 / B2, 1.0 / B1)
    b = H.rbf_apply_pair(x, y, g, f, P.GAUSSIAN, 4.0, 1.0 / B2, 1.0 / B1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ws = H.rbf_apply_pair_workspace(B1, B2, D, L, DEV)
    ox, oy = torch.empty_like(a[0]), torch.empty_like(a[1])
    r = H.rbf_apply_pair(x, y, g, f, P.GAUSSIAN, 4.0, 1.0 / B2, 1.0 / B1, ws=ws, out_x=ox, out_y=oy)
    assert r[0] is ox and r[1] is oy and torch.equal(ox, a[0]) and torch.equal(oy, a[1])


def test_workspace_contents_do_not_matter():
    """a workspace of 0xFF bytes (NaNs) against a zero-filled one: equal bits, finite"""
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, B2_MULTI, 5, 65
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    ws = H.rbf_apply_pair_workspace(B1, B2, D, L, DEV)
    outs = []
    for fill in (0xFF, 0x00):
        ws.fill_(fill)
        ox, oy = H.rbf_apply_pair(x, y, g, f, P.EXPONENTIAL, 2.0, 1.0 / B2, 1.0 / B1, ws=ws)
        assert bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oy).all())
        outs.append((ox, oy))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_outputs_stay_inside_their_buffers():
    """both outputs sit inside larger buffers with 256 sentinel words on each side"""
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 130, B2_MULTI, 3, 65
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    bx = torch.full((512 + B1 * L,), -7.0, device=DEV)
    by = torch.full((512 + B2 * L,), -7.0, device=DEV)
    ox, oy = bx[256:256 + B1 * L].view(B1, L), by[256:256 + B2 * L].view(B2, L)
    H.rbf_apply_pair(x, y, g, f, P.GAUSSIAN, 1.5, 1.0 / B2, 1.0 / B1, out_x=ox, out_y=oy)
    torch.cuda.synchronize()
    for buf in (bx, by):
        assert bool((buf[:256] == -7.0).all()) and bool((buf[-256:] == -7.0).all())
    want = H.rbf_apply_pair(x, y, g, f, P.GAUSSIAN, 1.5, 1.0 / B2, 1.0 / B1)
    assert torch.equal(ox, want[0]) and torch.equal(oy, want[1])


def test_refusals_leave_out_untouched():
    from neural_svd_amd import _lib, hip_ops as H
    from neural_svd_amd._lib import NsvdError
    B1, B2, D, L = BASE
    x, y, g, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    ox, oy = torch.full((B1, L), 7.0, device=DEV), torch.full((B2, L), 7.0, device=DEV)
    ws = H.rbf_apply_pair_workspace(B1, B2, D, L, DEV)

    def call(*a, **k):
        return H.rbf_apply_pair(*a, out_x=ox, out_y=oy, **k)
    for ell in (0.0, -1.0, float("nan")):
        with pytest.raises(NsvdError, match="invalid"):
            call(x, y, g, f, P.GAUSSIAN, ell, 1.0, 1.0)
    with pytest.raises(NsvdError, match="invalid"):
        call(x, y, g, f, 2, 1.0, 1.0, 1.0)
    with pytest.raises(NsvdError, match="invalid"):
        call(x, y, g, f, P.GAUSSIAN, 1.0, 1.0, 1.0, ws=ws[:ws.numel() - 256])
    with pytest.raises(NsvdError, match="invalid"):
        call(x, y, g, f, P.GAUSSIAN, 1.0, 1.0, 1.0,
             ws=torch.empty(ws.numel() + 256, dtype=torch.uint8, device=DEV)[4:])
    x65, y65 = torch.zeros(B1, 65, device=DEV), torch.zeros(B2, 65, device=DEV)
    with pytest.raises(NsvdError, match="unsupported"):
        call(x65, y65, g, f, P.GAUSSIAN, 1.0, 1.0, 1.0)
    with pytest.raises(NsvdError, match="unsupported"):
        H.rbf_apply_pair_workspace(B1, B2, 65, L, DEV)
    with pytest.raises(NsvdError, match="unsupported"):
        H.rbf_apply_pair_partition(B1, B2, 65, L)
    with pytest.raises(NsvdError):  # shapes that do not belong together
        call(x, y, g, f[:-1], P.GAUSSIAN, 1.0, 1.0, 1.0)
    with pytest.raises(NsvdError):
        call(x, y[:-1], g, f, P.GAUSSIAN, 1.0, 1.0, 1.0)
    # null pointers cannot come through the tensor wrapper: the C entry point itself
    lib = _lib.load()
    ptrs = dict(x=x.data_ptr(), y=y.data_ptr(), g=g.data_ptr(), f=f.data_ptr(), out_x=ox.data_ptr(),
                out_y=oy.data_ptr(), ws=ws.data_ptr())
    for null in ptrs:
        p = dict(ptrs, **{null: None})
        rc = lib.nsvd_rbf_apply_pair(p["x"], B1, p["y"], B2, D, p["g"], p["f"], L, P.GAUSSIAN, 1.0, 1.0, 1.0,
                                     p["out_x"], p["out_y"], p["ws"], ws.numel(),
                                     torch.cuda.current_stream().cuda_stream)
        with pytest.raises(NsvdError, match="invalid"):
            _lib.check(rc, f"nsvd_rbf_apply_pair({null} = NULL)")
    with pytest.raises(NsvdError, match="GPU"):
        call(x.cpu(), y, g, f, P.GAUSSIAN, 1.0, 1.0, 1.0)
    torch.cuda.synchronize()
    assert bool((ox == 7.0).all()) and bool((oy == 7.0).all())
    # and the same arguments without the faults are accepted
    call(x, y, g, f, P.GAUSSIAN, 1.0, 1.0, 1.0, ws=ws)
    assert not bool((ox == 7.0).any()) and not bool((oy == 7.0).any())
