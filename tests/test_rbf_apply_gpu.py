"""GPU tests of the matrix-free radial kernel operator (nsvd_rbf_apply, hip_ops.rbf_apply) against its float64
restatement (tests/_rbf_oracle.py). rel = max |got - want| / max |want|; the bound is max(2e-6, 4 * yardstick), the
yardstick being the rel of the same quantity composed in float32 on the same GPU from direct differences
(((x[:, None] - y[None]) ** 2).sum(-1), exp, @ f) against the same oracle."""
import ctypes

import pytest
import torch

from tests import _rbf_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"gaussian": R.GAUSSIAN, "exponential": R.EXPONENTIAL}
BASE = (65, 200, 3, 5)  # B1, B2, D, L
B2_SPLIT = 1030         # 17 chunks of 64 reference rows: the split rule cuts them into two slices (asserted below)


def rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def yardstick(x, y, f, kind, ell, scale):
    d2 = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    k = torch.exp(-d2 / (2.0 * ell ** 2)) if kind == R.GAUSSIAN else torch.exp(-d2.sqrt() / ell)
    return scale * (k @ f)


def _shapes():
    b1, b2, d, l = BASE
    s = [(v, b2, d, l) for v in (1, 63, 64, 65, 130)]
    s += [(b1, v, d, l) for v in (1, 63, 64, 65, 200, B2_SPLIT)]
    s += [(b1, b2, v, l) for v in (1, 2, 3, 16, 17, 64)]  # one distance form (direct differences) at every D
    s += [(b1, b2, d, v) for v in (1, 5, 64, 65, 130)]
    s += [(1, 1, 1, 1), (130, B2_SPLIT, 64, 130), (1, B2_SPLIT, 64, 1), (130, 1, 1, 130)]  # corners
    return sorted(set(s))


def _inputs(B1, B2, D, L, shift=0.0):
    g = torch.Generator().manual_seed(1000 * B1 + 100 * B2 + 10 * D + L)
    x = (torch.randn(B1, D, generator=g) + shift).float()
    y = (torch.randn(B2, D, generator=g) + shift).float()
    f = torch.randn(B2, L, generator=g)
    return x, y, f


def _check(x, y, f, kind, ell, what, bound=None):
    """got and the float32 yardstick against the oracle on the SAME float32 inputs; returns (rel, yardstick rel)"""
    from neural_svd_amd import hip_ops as H
    scale = 1.0 / y.shape[0]
    want = R.radial_kernel_apply(x, y, f, kind, ell, scale)
    xd, yd, fd = x.to(DEV), y.to(DEV), f.to(DEV)
    got = H.rbf_apply(xd, yd, fd, kind, ell, scale)
    e, ey = rel(got, want), rel(yardstick(xd, yd, fd, kind, ell, scale), want)
    bound = max(2e-6, 4.0 * ey) if bound is None else bound
    print(f"rbf_apply {what}: rel {e:.2e} yardstick {ey:.2e} bound {bound:.2e}")
    assert bool(torch.isfinite(got).all())
    assert e < bound, (what, e, ey, bound)
    return e, ey


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B1,B2,D,L", _shapes())
def test_against_float64(B1, B2, D, L, kind):
    """One axis at a time around (65, 200, 3, 5) plus the corners; ell = sqrt(D) keeps the kernel values O(1) at every
    D. B2 = 1030 takes two slices of the reference rows. Measured on an MI355X (rel / yardstick, worst of each group;
    every case took the 2e-6 floor or a bound within 3.1e-6; the kernel matrix cases: 9.6e-8 / 8.9e-8):

        group            gaussian            exponential
        B1 in 1..130     5.2e-7 / 6.0e-7     5.9e-7 / 7.6e-7
        B2 in 1..1030    3.1e-7 / 4.7e-7     2.9e-7 / 4.3e-7
        D in 1..64       3.5e-7 / 5.7e-7     3.0e-7 / 7.4e-7
        L in 1..130      3.1e-7 / 6.9e-7     3.1e-7 / 5.6e-7
        corners          3.2e-7 / 6.2e-7     3.7e-7 / 3.6e-7"""
    assert R.split_slices(BASE[0], BASE[1], BASE[3]) == 1 and R.split_slices(BASE[0], B2_SPLIT, BASE[3]) == 2
    x, y, f = _inputs(B1, B2, D, L)
    _check(x, y, f, KINDS[kind], float(D) ** 0.5, f"{kind} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_matrix_itself(kind):
    """x is y (the same tensor) and f = B2 * I: the output is the kernel matrix - ones on the diagonal (d = 0, the
    exponential kind's sqrt(0) included), nothing above 1."""
    from neural_svd_amd import hip_ops as H
    B, D = 65, 3
    x, _, _ = _inputs(B, B, D, B)
    f = float(B) * torch.eye(B)
    _check(x, x, f, KINDS[kind], 1.3, f"{kind} kernel matrix")
    xd = x.to(DEV)
    got = H.rbf_apply(xd, xd, f.to(DEV), KINDS[kind], 1.3, 1.0 / B)
    assert float((got.diagonal() - 1.0).abs().max()) <= 1e-6
    assert float(got.max()) <= 1.0 + 1e-6 and float(got.min()) >= 0.0


@pytest.mark.parametrize("kind", list(KINDS))
def test_far_rows_give_exact_zeros(kind):
    from neural_svd_amd import hip_ops as H
    x = torch.zeros(2, 3)
    x[1, 0] = 1e3
    xd = x.to(DEV)
    got = H.rbf_apply(xd, xd, (2.0 * torch.eye(2)).to(DEV), KINDS[kind], 1.0, 0.5)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.cpu(), torch.eye(2)), got


def test_shifted_points_meet_the_unshifted_bound():
    """D = 16, ell = 1, every coordinate shifted by +100: the distances come from direct differences, so the shifted
    case meets the bound of the unshifted one. Measured: unshifted 3.5e-7 (yardstick 3.1e-7), shifted 4.9e-7 (yardstick 2.9e-7), bound 2e-6."""
    B1, B2, D, L = 65, 200, 16, 5
    x, y, f = _inputs(B1, B2, D, L)
    e0, ey0 = _check(x, y, f, R.GAUSSIAN, 1.0, "unshifted D=16 ell=1")
    bound = max(2e-6, 4.0 * ey0)
    xs, ys, _ = _inputs(B1, B2, D, L, shift=100.0)
    _check(xs, ys, f, R.GAUSSIAN, 1.0, "shifted +100 D=16 ell=1", bound=bound)


def test_two_calls_give_the_same_bits():
    from neural_svd_amd import hip_ops as H
    x, y, f = (t.to(DEV) for t in _inputs(130, B2_SPLIT, 16, 65))
    a = H.rbf_apply(x, y, f, R.GAUSSIAN, 4.0, 1.0 / B2_SPLIT)
    b = H.rbf_apply(x, y, f, R.GAUSSIAN, 4.0, 1.0 / B2_SPLIT)
    assert torch.equal(a, b)
    ws = H.rbf_apply_workspace(130, B2_SPLIT, 16, 65, DEV)
    out = torch.empty_like(a)
    assert H.rbf_apply(x, y, f, R.GAUSSIAN, 4.0, 1.0 / B2_SPLIT, ws=ws, out=out) is out and torch.equal(out, a)


def test_refusals_leave_out_untouched():
    from neural_svd_amd import _lib, hip_ops as H
    from neural_svd_amd._lib import NsvdError
    B1, B2, D, L = 65, 200, 3, 5
    x, y, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    out = torch.full((B1, L), 7.0, device=DEV)
    ws = H.rbf_apply_workspace(B1, B2, D, L, DEV)
    with pytest.raises(NsvdError, match="invalid"):
        H.rbf_apply(x, y, f, R.GAUSSIAN, 0.0, 1.0, out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.rbf_apply(x, y, f, R.GAUSSIAN, -1.0, 1.0, out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.rbf_apply(x, y, f, R.GAUSSIAN, float("nan"), 1.0, out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.rbf_apply(x, y, f, 2, 1.0, 1.0, out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.rbf_apply(x, y, f, R.GAUSSIAN, 1.0, 1.0, ws=ws[:ws.numel() - 256], out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.rbf_apply(x, y, f, R.GAUSSIAN, 1.0, 1.0, ws=torch.empty(ws.numel() + 256, dtype=torch.uint8, device=DEV)[4:],
                    out=out)
    x65, y65 = torch.zeros(B1, 65, device=DEV), torch.zeros(B2, 65, device=DEV)
    with pytest.raises(NsvdError, match="unsupported"):
        H.rbf_apply(x65, y65, f, R.GAUSSIAN, 1.0, 1.0, out=out)
    with pytest.raises(NsvdError, match="unsupported"):
        H.rbf_apply_workspace(B1, B2, 65, L, DEV)
    # null pointers cannot come through the tensor wrapper: the C entry point itself
    lib = _lib.load()
    ptrs = dict(x=x.data_ptr(), y=y.data_ptr(), f=f.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr())
    for null in ptrs:
        p = dict(ptrs, **{null: None})
        rc = lib.nsvd_rbf_apply(p["x"], B1, p["y"], B2, D, p["f"], L, R.GAUSSIAN, 1.0, 1.0, p["out"], p["ws"],
                                ws.numel(), torch.cuda.current_stream().cuda_stream)
        with pytest.raises(NsvdError, match="invalid"):
            _lib.check(rc, f"nsvd_rbf_apply({null} = NULL)")
    with pytest.raises(NsvdError, match="GPU"):
        H.rbf_apply(x.cpu(), y, f, R.GAUSSIAN, 1.0, 1.0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # and the same arguments without the faults are accepted
    H.rbf_apply(x, y, f, R.GAUSSIAN, 1.0, 1.0, ws=ws, out=out)
    assert not bool((out == 7.0).any())
