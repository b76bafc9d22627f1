"""GPU tests of the matrix-free dot-product kernel operator (nsvd_dot_apply, hip_ops.dot_apply) against its float64
restatement (tests/_dot_oracle.py), case for case as tests/test_rbf_apply_gpu.py. rel = max |got - want| / max |want|;
the bound is max(2e-6, 4 * yardstick), the yardstick being the rel of the same quantity composed in float32 from library
calls on the same GPU (x @ y.T, the map, @ f) against the same oracle. gamma and coef0 are float32 values, so that the
oracle sees the inputs the kernel sees."""
import numpy as np
import pytest
import torch

from tests import _dot_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# variant -> (kind, degree)
VARIANTS = {"arccos1": (R.ARCCOS1, 2), "poly1": (R.POLYNOMIAL, 1), "poly2": (R.POLYNOMIAL, 2), "poly3": (R.POLYNOMIAL, 3),
            "poly8": (R.POLYNOMIAL, 8)}
BASE = (65, 200, 3, 5)  # B1, B2, D, L
B2_SPLIT = 1030         # 17 chunks of 64 reference rows: the split rule cuts them into two slices (asserted below)
B2_FIRST_SPLIT = 961    # 16 chunks: the smallest B2 at which the rule takes two slices at this B1, L (asserted below)


def f32(v):
    return float(np.float32(v))


def rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def yardstick(x, y, f, kind, gamma, coef0, degree, scale):
    s = x @ y.T
    if kind == R.POLYNOMIAL:
        k = (gamma * s + coef0) ** degree
    else:
        p = x.norm(dim=1)[:, None] * y.norm(dim=1)[None, :]
        c = (s / p).clamp(-1.0, 1.0)
        t = torch.acos(c)
        k = p / torch.pi * (torch.sin(t) + (torch.pi - t) * c).clamp(min=0.0)
        k = torch.where(p > 0, k, torch.zeros_like(k))
    return scale * (k @ f)


def _shapes():
    b1, b2, d, l = BASE
    s = [(v, b2, d, l) for v in (1, 63, 64, 65, 130)]
    s += [(b1, v, d, l) for v in (1, 63, 64, 65, 200, B2_FIRST_SPLIT, B2_SPLIT)]
    # D is a contraction length here, padded to 8: both sides of every padding step, and the steps of narrower paddings
    s += [(b1, b2, v, l) for v in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64)]
    s += [(b1, b2, d, v) for v in (1, 5, 64, 65, 130)]
    s += [(1, 1, 1, 1), (130, B2_SPLIT, 64, 130), (1, B2_SPLIT, 64, 1), (130, 1, 1, 130)]  # corners
    return sorted(set(s))


def _inputs(B1, B2, D, L):
    g = torch.Generator().manual_seed(1000 * B1 + 100 * B2 + 10 * D + L)
    x = torch.randn(B1, D, generator=g).float()
    y = torch.randn(B2, D, generator=g).float()
    f = torch.randn(B2, L, generator=g)
    return x, y, f


def _check(x, y, f, kind, gamma, coef0, degree, what):
    """got and the float32 yardstick against the oracle on the SAME float32 inputs; returns (rel, yardstick rel)"""
    from neural_svd_amd import hip_ops as H
    scale = 1.0 / y.shape[0]
    want = R.dot_kernel_apply(x, y, f, kind, gamma, coef0, degree, scale)
    xd, yd, fd = x.to(DEV), y.to(DEV), f.to(DEV)
    got = H.dot_apply(xd, yd, fd, kind, gamma, coef0, degree, scale)
    e, ey = rel(got, want), rel(yardstick(xd, yd, fd, kind, gamma, coef0, degree, scale), want)
    bound = max(2e-6, 4.0 * ey)
    print(f"dot_apply {what}: rel {e:.2e} yardstick {ey:.2e} bound {bound:.2e}")
    assert bool(torch.isfinite(got).all())
    assert e < bound, (what, e, ey, bound)
    return e, ey


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B1,B2,D,L", _shapes())
def test_against_float64(B1, B2, D, L, variant):
    """One axis at a time around (65, 200, 3, 5) plus the corners; gamma = 1 / D, coef0 = 1 keep the polynomial's base
    O(1) at every D. B2 = 961 and 1030 take two slices of the reference rows. Measured on an MI355X (rel / yardstick,
    worst of each group):

        group            arccos1            poly1              poly2              poly3              poly8
        B1 in 1..130     2.6e-7 / 3.5e-7    3.1e-7 / 4.5e-7    2.5e-7 / 5.1e-7    3.0e-7 / 3.4e-7    4.2e-7 / 5.6e-7
        B2 in 1..1030    3.8e-7 / 6.7e-7    2.8e-7 / 1.3e-6    3.4e-7 / 1.2e-6    2.8e-7 / 6.5e-7    1.5e-6 / 1.8e-6
        D in 1..64       3.4e-7 / 5.6e-7    3.5e-7 / 6.2e-7    3.2e-7 / 5.1e-7    3.0e-7 / 6.2e-7    4.2e-7 / 1.2e-6
        L in 1..130      2.2e-7 / 4.8e-7    2.8e-7 / 7.0e-7    2.7e-7 / 4.1e-7    2.7e-7 / 6.2e-7    4.2e-7 / 5.7e-7
        corners          3.1e-7 / 6.7e-7    8.8e-7 / 8.8e-7    4.6e-7 / 4.6e-7    2.6e-7 / 1.0e-6    3.4e-7 / 5.0e-7

    (150 cases; the largest bound any case was given is 7.3e-6; the kernel-matrix diagonals: arc-cosine 1.7e-7,
    polynomial 1.1e-7 / 2.2e-7 / 3.2e-7 / 8.2e-7 at degrees 1 / 2 / 3 / 8)"""
    assert R.split_slices(BASE[0], BASE[1], BASE[3]) == 1 and R.split_slices(BASE[0], B2_SPLIT, BASE[3]) == 2
    assert R.split_slices(BASE[0], B2_FIRST_SPLIT - 1, BASE[3]) == 1 and R.split_slices(BASE[0], B2_FIRST_SPLIT, BASE[3]) == 2
    kind, degree = VARIANTS[variant]
    x, y, f = _inputs(B1, B2, D, L)
    _check(x, y, f, kind, f32(1.0 / D), 1.0, degree, f"{variant} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_matrix_itself(variant):
    """x is y (the same tensor) and f = B2 * I: the output is the kernel matrix. Arc-cosine: |x_i|^2 on the diagonal to
    1e-6 relative (t ~ 4e-4 there costs 1e-7: the bracket is stationary at t = 0), nothing negative. Polynomial:
    (gamma |x_i|^2 + c)^p on the diagonal, to degree * 1e-6 relative (each factor carries the rounding of its base)."""
    from neural_svd_amd import hip_ops as H
    kind, degree = VARIANTS[variant]
    B, D = 65, 3
    gamma, coef0 = f32(1.0 / D), 0.5
    x, _, _ = _inputs(B, B, D, B)
    f = float(B) * torch.eye(B)
    _check(x, x, f, kind, gamma, coef0, degree, f"{variant} kernel matrix")
    xd = x.to(DEV)
    got = H.dot_apply(xd, xd, f.to(DEV), kind, gamma, coef0, degree, 1.0 / B).cpu().double()
    n2 = (x.double() ** 2).sum(1)
    if kind == R.ARCCOS1:
        d = float(((got.diagonal() - n2).abs() / n2).max())
        print(f"arccos1 diagonal against |x_i|^2: {d:.2e}")
        assert d <= 1e-6
        assert float(got.min()) >= 0.0
    else:
        want = (gamma * n2 + coef0) ** degree
        d = float(((got.diagonal() - want).abs() / want).max())
        print(f"{variant} diagonal against (gamma |x_i|^2 + c)^p: {d:.2e}")
        assert d <= degree * 1e-6


def test_zero_row_and_antiparallel_pair():
    """arc-cosine kind: a zero row gives exact zeros (row and column), an antiparallel pair something finite and >= 0
    (its exact value is 0; float32 leaves at most the rounding of cos t, ~(2e-7)^(3/2) |x||y|); polynomial kind: the zero
    row gives coef0^degree exactly."""
    from neural_svd_amd import hip_ops as H
    x = torch.randn(8, 3, generator=torch.Generator().manual_seed(5))
    x[0] = 0.0
    x[2] = -1.7 * x[1]
    xd = x.to(DEV)
    f = (8.0 * torch.eye(8)).to(DEV)   # with scale = 1 / 8: the kernel matrix, exactly
    got = H.dot_apply(xd, xd, f, R.ARCCOS1, 1.0, 1.0, 2, 0.125).cpu()
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0
    assert bool((got[0] == 0).all()) and bool((got[:, 0] == 0).all())
    for i, j in ((1, 2), (2, 1)):
        assert 0.0 <= float(got[i, j]) <= 1e-6 * float(x[1].norm() * x[2].norm())
    want = R.dot_kernel_matrix(x, x, R.ARCCOS1)
    assert float((got.double() - want).abs().max() / want.abs().max()) < 2e-6
    got = H.dot_apply(xd, xd, f, R.POLYNOMIAL, 0.5, 0.75, 3, 0.125).cpu()
    assert bool((got[0] == 0.75 ** 3).all()) and bool((got[:, 0] == 0.75 ** 3).all())
    # a coef0 whose power overflows: +inf where float32 gives it, and the padded reference rows (56 of this chunk) stay out
    got = H.dot_apply(xd, xd, torch.ones(8, 1, device=DEV), R.POLYNOMIAL, 1.0, 1e30, 2, 0.125).cpu()
    assert bool((got == float("inf")).all()), got


def test_two_calls_give_the_same_bits():
    from neural_svd_amd import hip_ops as H
    x, y, f = (t.to(DEV) for t in _inputs(130, B2_SPLIT, 16, 65))
    for kind, degree in ((R.ARCCOS1, 2), (R.POLYNOMIAL, 3)):
        a = H.dot_apply(x, y, f, kind, 0.0625, 1.0, degree, 1.0 / B2_SPLIT)
        b = H.dot_apply(x, y, f, kind, 0.0625, 1.0, degree, 1.0 / B2_SPLIT)
        assert torch.equal(a, b)
        ws = H.dot_apply_workspace(130, B2_SPLIT, 16, 65, DEV)
        out = torch.empty_like(a)
        assert H.dot_apply(x, y, f, kind, 0.0625, 1.0, degree, 1.0 / B2_SPLIT, ws=ws, out=out) is out
        assert torch.equal(out, a)


def test_refusals_leave_out_untouched():
    from neural_svd_amd import _lib, hip_ops as H
    from neural_svd_amd._lib import NsvdError
    B1, B2, D, L = 65, 200, 3, 5
    x, y, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    out = torch.full((B1, L), 7.0, device=DEV)
    ws = H.dot_apply_workspace(B1, B2, D, L, DEV)
    P = R.POLYNOMIAL
    for kind, gamma, coef0, degree in ((2, 1.0, 1.0, 2), (-1, 1.0, 1.0, 2), (P, 1.0, 1.0, 0), (P, 1.0, 1.0, 9),
                                       (P, float("nan"), 1.0, 2), (P, float("inf"), 1.0, 2), (P, 1.0, float("nan"), 2),
                                       (P, 1.0, float("-inf"), 2)):
        with pytest.raises(NsvdError, match="invalid"):
            H.dot_apply(x, y, f, kind, gamma, coef0, degree, 1.0, out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.dot_apply(x, y, f, P, 1.0, 1.0, 2, 1.0, ws=ws[:ws.numel() - 256], out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.dot_apply(x, y, f, P, 1.0, 1.0, 2, 1.0, ws=torch.empty(ws.numel() + 256, dtype=torch.uint8, device=DEV)[4:],
                    out=out)
    x65, y65 = torch.zeros(B1, 65, device=DEV), torch.zeros(B2, 65, device=DEV)
    with pytest.raises(NsvdError, match="unsupported"):
        H.dot_apply(x65, y65, f, P, 1.0, 1.0, 2, 1.0, out=out)
    with pytest.raises(NsvdError, match="unsupported"):
        H.dot_apply_workspace(B1, B2, 65, L, DEV)
    # null pointers and non-positive sizes cannot come through the tensor wrapper: the C entry point itself
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = dict(x=x.data_ptr(), y=y.data_ptr(), f=f.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr())
    for null in ptrs:
        p = dict(ptrs, **{null: None})
        rc = lib.nsvd_dot_apply(p["x"], B1, p["y"], B2, D, p["f"], L, P, 1.0, 1.0, 2, 1.0, p["out"], p["ws"],
                                ws.numel(), stream)
        with pytest.raises(NsvdError, match="invalid"):
            _lib.check(rc, f"nsvd_dot_apply({null} = NULL)")
    for sizes in ((0, B2, D, L), (B1, 0, D, L), (B1, B2, 0, L), (B1, B2, D, 0), (-1, B2, D, L)):
        rc = lib.nsvd_dot_apply(ptrs["x"], sizes[0], ptrs["y"], sizes[1], sizes[2], ptrs["f"], sizes[3], P, 1.0, 1.0, 2,
                                1.0, ptrs["out"], ptrs["ws"], ws.numel(), stream)
        with pytest.raises(NsvdError, match="invalid"):
            _lib.check(rc, f"nsvd_dot_apply{sizes}")
    with pytest.raises(NsvdError, match="GPU"):
        H.dot_apply(x.cpu(), y, f, P, 1.0, 1.0, 2, 1.0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the arc-cosine kind ignores gamma, coef0 and degree: what the polynomial kind refuses is accepted there
    H.dot_apply(x, y, f, R.ARCCOS1, float("nan"), float("nan"), 0, 1.0, ws=ws, out=out)
    assert not bool((out == 7.0).any()) and bool(torch.isfinite(out).all())
    # and the same arguments without the faults are accepted
    out.fill_(7.0)
    H.dot_apply(x, y, f, P, 1.0, 1.0, 2, 1.0, ws=ws, out=out)
    assert not bool((out == 7.0).any())
