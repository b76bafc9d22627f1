"""CPU checks of the dot-product kernel SVD path's ground truth: the closed-form singular values of the polynomial
kernel between two Gaussian measures (kernel_ops.polynomial_cross_singular_values, exact from moments) against a
Gauss-Hermite quadrature SVD, and the host-side queries of nsvd_dot_apply_pair."""
import ctypes
import math

import numpy as np
import pytest

from tests import _dot_oracle as DO
from tests import _dot_pair_oracle as DP

# sigma_x, sigma_y, gamma, coef0, degree
PARAMS = ((1.0, 0.5, 0.5, 1.0, 2), (1.3, 0.7, 1.0, 0.5, 3), (1.0, 1.0, 0.25, 1.0, 4), (1.1, 0.6, 0.8, 0.0, 3))


def quadrature_singular_values(sigma_x, sigma_y, gamma, coef0, degree, dim):
    """the SVD of diag(sqrt w_x) K diag(sqrt w_y) on Gauss-Hermite nodes: 120 in 1-D, a 40 x 40 tensor grid in 2-D
    (exact for the polynomial integrands up to rounding: degree 2 x 4 = 8 per variable at most)"""
    t, w = np.polynomial.hermite.hermgauss(120 if dim == 1 else 40)
    wq = w / np.sqrt(np.pi)
    if dim == 1:
        nodes, wts = t[:, None], wq
    else:
        nodes = np.stack(np.meshgrid(t, t, indexing="ij"), axis=-1).reshape(-1, 2)
        wts = (wq[:, None] * wq[None, :]).reshape(-1)
    xs, ys = np.sqrt(2.0) * sigma_x * nodes, np.sqrt(2.0) * sigma_y * nodes
    u = gamma * (xs @ ys.T) + coef0
    K = u.copy()
    for _ in range(degree - 1):
        K = K * u
    return np.linalg.svd(np.sqrt(wts)[:, None] * K * np.sqrt(wts)[None, :], compute_uv=False)


def expected_rank(dim, coef0, degree):
    return DO.polynomial_rank(dim, degree) if coef0 > 0 else math.comb(dim + degree - 1, degree)


@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("sigma_x,sigma_y,gamma,coef0,degree", PARAMS)
def test_closed_form_against_quadrature_svd(sigma_x, sigma_y, gamma, coef0, degree, dim):
    from neural_svd_amd.kernel_ops import polynomial_cross_singular_values
    n = 24
    q = quadrature_singular_values(sigma_x, sigma_y, gamma, coef0, degree, dim)[:n]
    s = polynomial_cross_singular_values(sigma_x, sigma_y, gamma, coef0, degree, dim, n)
    err = np.abs(s - q).max()
    print(f"sigma {sigma_x} {sigma_y} gamma {gamma} coef0 {coef0} degree {degree} dim {dim}: s_0 {s[0]:.7f} "
          f"max error {err:.1e} non-zero {np.count_nonzero(s)}")
    assert s.dtype == np.float64 and s.shape == (n,)
    assert np.all(np.diff(s) <= 0.0)
    assert err < 1e-10 * s[0]
    # the count of non-zero values is the rank; the values beyond it are exact zeros
    r = expected_rank(dim, coef0, degree)
    assert np.count_nonzero(s) == r and np.all(s[r:] == 0.0) and np.all(s[:r] > 1e-8 * s[0])


def test_the_issue_example_and_the_order_of_the_measures():
    from neural_svd_amd.kernel_ops import polynomial_cross_singular_values
    s = polynomial_cross_singular_values(1.0, 0.5, 0.5, 1.0, 2, 1, 3)
    assert np.abs(s - np.array([1.0707606, 0.5, 0.1167394])).max() < 1e-6
    # K and K^T share their singular values: the order of the two measures does not matter
    for sx, sy, gamma, coef0, degree in PARAMS:
        for dim in (1, 2, 3):
            a = polynomial_cross_singular_values(sx, sy, gamma, coef0, degree, dim, 12)
            b = polynomial_cross_singular_values(sy, sx, gamma, coef0, degree, dim, 12)
            assert np.abs(a - b).max() <= 1e-13 * a[0], (sx, sy, dim)
    # a request shorter than the rank is a prefix
    assert np.array_equal(polynomial_cross_singular_values(1.0, 0.5, 0.5, 1.0, 2, 2, 2),
                          polynomial_cross_singular_values(1.0, 0.5, 0.5, 1.0, 2, 2, 9)[:2])
    with pytest.raises(ValueError):
        polynomial_cross_singular_values(1.0, 0.5, 0.5, 1.0, 0, 1, 3)
    with pytest.raises(ValueError):
        polynomial_cross_singular_values(0.0, 0.5, 0.5, 1.0, 2, 1, 3)


def test_workspace_and_partition_queries():
    from neural_svd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.nsvd_abi_version() == 6
    q, part = lib.nsvd_dot_apply_pair_workspace_bytes, lib.nsvd_dot_apply_pair_partition
    rg, cs = ctypes.c_int(-5), ctypes.c_int(-5)
    for bad in ((0, 8, 2, 2), (8, 0, 2, 2), (8, 8, 0, 2), (8, 8, 65, 2), (8, 8, 2, 0), (-1, 8, 2, 2)):
        assert q(*bad) == 0, bad
        assert part(*bad, ctypes.byref(rg), ctypes.byref(cs)) != 0 and (rg.value, cs.value) == (-5, -5), bad
    assert part(8, 8, 65, 2, ctypes.byref(rg), ctypes.byref(cs)) == _lib.EUNSUPPORTED
    assert part(8, 8, 2, 2, None, ctypes.byref(cs)) == _lib.EINVAL and part(8, 8, 2, 2, ctypes.byref(rg), None) == _lib.EINVAL
    for shape in ((1, 1, 1, 1), (65, 200, 3, 5), (65, 257, 3, 5), (130, 1030, 64, 130), (1030, 130, 64, 130),
                  (8192, 8192, 16, 64), (8192, 8192, 64, 64)):
        assert q(*shape) == DP.pair_workspace_bytes(*shape) and q(*shape) % 256 == 0, shape
        assert part(*shape, ctypes.byref(rg), ctypes.byref(cs)) == 0
        assert (rg.value, cs.value) == DP.pair_split(shape[0], shape[1], shape[3]), shape
        # the radial pair's partition is the same rule
        rr, rc = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.nsvd_rbf_apply_pair_partition(*shape, ctypes.byref(rr), ctypes.byref(rc)) == 0
        assert (rr.value, rc.value) == (rg.value, cs.value), shape
    assert [DP.pair_split(65, 200, 5), DP.pair_split(65, 257, 5), DP.pair_split(130, 1030, 130),
            DP.pair_split(1030, 130, 130), DP.pair_split(8192, 8192, 64)] == [(2, 1), (2, 2), (2, 4), (16, 1), (32, 16)]


def test_workspace_is_monotone_and_the_copies_are_capped():
    """more rows never need less workspace; never more than 32 partial copies of either output, up to 65 536 rows"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd import _lib
    q = _lib.load().nsvd_dot_apply_pair_workspace_bytes
    sizes = (1, 63, 64, 65, 130, 257, 1030, 4096, 8192, 8193, 16384, 40000, 65536)
    for D, L in ((1, 1), (3, 5), (16, 64), (64, 130)):
        for fixed in (1, 200, 8192):
            a = [q(B, fixed, D, L) for B in sizes]
            b = [q(fixed, B, D, L) for B in sizes]
            assert a == sorted(a) and b == sorted(b), (D, L, fixed)
            assert all(v > 0 and v % 256 == 0 for v in a + b)
        for B1 in sizes:
            for B2 in sizes:
                rg, cs = H.dot_apply_pair_partition(B1, B2, D, L)
                assert 1 <= rg <= min(32, (B1 + 63) // 64) and 1 <= cs <= min(32, (B2 + 255) // 256), (B1, B2, D, L)
    assert q(200, 200, 65, 5) == 0 and q(200, 200, 64, 5) > 0


def test_python_refusals_without_a_gpu():
    import torch
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    x, y, g, f = torch.zeros(8, 2), torch.zeros(9, 2), torch.zeros(9, 3), torch.zeros(8, 3)
    with pytest.raises(NsvdError, match="GPU"):
        H.dot_apply_pair(x, y, g, f, H.DOT_POLYNOMIAL, 1.0, 1.0, 2, 1.0, 1.0)
    with pytest.raises(NsvdError):
        H.dot_apply_pair(x, y, g, f[:, :2], H.DOT_POLYNOMIAL, 1.0, 1.0, 2, 1.0, 1.0)
    with pytest.raises(NsvdError, match="unsupported"):
        H.dot_apply_pair_workspace(8, 8, 65, 3, "cpu")
    with pytest.raises(NsvdError, match="unsupported"):
        H.dot_apply_pair_partition(8, 8, 65, 3)
    with pytest.raises(NsvdError, match="invalid"):
        H.dot_apply_pair_partition(0, 8, 2, 3)
