"""CPU checks of the dot-product kernel operator's ground truth (tests/_dot_oracle.py, float64): the finite rank of the
polynomial Gram, the arc-cosine kernel against its defining expectation by quadrature, its edge cases, the host-side
ABI queries of nsvd_dot_apply and the refusals of the Python surface that need no GPU."""
import math

import numpy as np
import pytest
import torch

from tests import _dot_oracle as R


def _points(n, D, seed=0):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_polynomial_gram_has_the_rank_of_its_monomials():
    """n = 200 points at (D, degree) = (3, 2): the Gram has numerical rank C(5, 2) = 10 - the 11th eigenvalue is below
    1e-12 of the first (measured 1.1e-16), the 10th is not (8.5e-2)."""
    x = _points(200, 3)
    G = R.dot_kernel_matrix(x, x, R.POLYNOMIAL, 1.0 / 3, 1.0, 2)
    lam = torch.linalg.eigvalsh(G).flip(0)
    assert R.polynomial_rank(3, 2) == 10 and R.polynomial_rank(3, 3) == 20
    print(f"lam_10 / lam_1 = {float(lam[9] / lam[0]):.2e}, |lam_11| / lam_1 = {float(lam[10].abs() / lam[0]):.2e}")
    assert float(lam[10].abs()) < 1e-12 * float(lam[0])
    assert float(lam[9]) > 1e-3 * float(lam[0])
    # the power by multiplication is the power
    assert torch.allclose(G, (x @ x.T / 3 + 1.0) ** 2, rtol=1e-12, atol=1e-14)
    assert torch.equal(R.dot_kernel_matrix(x, x, R.POLYNOMIAL, 0.5, 0.25, 1), 0.5 * (x @ x.T) + 0.25)
    with pytest.raises(ValueError):
        R.dot_kernel_matrix(x, x, R.POLYNOMIAL, 1.0, 1.0, 9)


def test_arccos_diagonal_is_the_squared_norm():
    for D in (1, 2, 3, 16, 64):
        x = _points(50, D, seed=D)
        G = R.dot_kernel_matrix(x, x, R.ARCCOS1)
        n2 = (x * x).sum(1)
        assert float(((G.diagonal() - n2).abs() / n2).max()) < 1e-14
        assert torch.allclose(G, G.T, rtol=1e-14, atol=0) and float(G.min()) >= 0.0


def test_arccos_is_the_relu_expectation_in_two_dimensions():
    """k(x, y) = 2 E_w[relu(w.x) relu(w.y)], w ~ N(0, I_2). With w = r u(phi): E[r^2] over the radial density
    r exp(-r^2 / 2) is 2, so k = (2 / pi) int_0^2pi relu(u.x) relu(u.y) dphi. The integrand is smooth on the arc where
    both factors are positive (phi - a_x in [max(-pi/2, d - pi/2), min(pi/2, d + pi/2)], d the angle from x to y) and 0
    off it: 48-point Gauss-Legendre on that arc. Relative to |x||y|: below 1e-10 (measured 3.9e-15)."""
    x, y = _points(23, 2, seed=1), _points(31, 2, seed=2)
    y[0] = -2.0 * x[0]   # an antiparallel pair: an empty arc
    y[1] = 0.5 * x[1]    # a parallel one: the whole half circle
    G = R.dot_kernel_matrix(x, y, R.ARCCOS1)
    t, w = np.polynomial.legendre.leggauss(48)
    t, w = torch.tensor(t), torch.tensor(w)
    ax, ay = torch.atan2(x[:, 1], x[:, 0]), torch.atan2(y[:, 1], y[:, 0])
    d = torch.remainder(ay[None, :] - ax[:, None] + math.pi, 2.0 * math.pi) - math.pi
    lo = torch.maximum(torch.full_like(d, -math.pi / 2), d - math.pi / 2) + ax[:, None]
    hi = torch.minimum(torch.full_like(d, math.pi / 2), d + math.pi / 2) + ax[:, None]
    half = ((hi - lo) / 2).clamp(min=0.0)
    phi = ((hi + lo) / 2)[..., None] + half[..., None] * t                  # (23, 31, 48)
    u = torch.stack([torch.cos(phi), torch.sin(phi)], dim=-1)               # (23, 31, 48, 2)
    rx = torch.relu((u * x[:, None, None, :]).sum(-1))
    ry = torch.relu((u * y[None, :, None, :]).sum(-1))
    want = (2.0 / math.pi) * half * ((rx * ry) * w).sum(-1)
    err = float(((G - want).abs() / (x.norm(dim=1)[:, None] * y.norm(dim=1)[None, :])).max())
    print(f"arc-cosine kernel against the relu expectation: {err:.1e}")
    assert err < 1e-10
    assert float(G[0, 0]) == 0.0 or abs(float(G[0, 0])) < 1e-20


def test_arccos_zero_rows_and_antiparallel_rows():
    x = torch.tensor([[0.0, 0.0, 0.0], [1.0, -2.0, 0.5], [-1.0, 2.0, -0.5], [3.0, 0.1, 0.2]], dtype=torch.float64)
    G = R.dot_kernel_matrix(x, x, R.ARCCOS1)
    assert bool(torch.isfinite(G).all()) and float(G.min()) >= 0.0
    assert bool((G[0] == 0).all()) and bool((G[:, 0] == 0).all())
    assert float(G[1, 2]) >= 0.0 and float(G[1, 2]) < 1e-15
    # nearly antiparallel: the bracket is ~(pi - t)^3 / 3, never negative
    for eps in (1e-3, 1e-6, 1e-9):
        a = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
        b = torch.tensor([[-1.0, eps]], dtype=torch.float64)
        v = float(R.dot_kernel_matrix(a, b, R.ARCCOS1))
        assert 0.0 <= v <= eps ** 3, (eps, v)


def test_abi_version_and_workspace_queries():
    from neural_svd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.nsvd_abi_version() == 6
    q = lib.nsvd_dot_apply_workspace_bytes
    for bad in ((0, 8, 2, 2), (8, 0, 2, 2), (8, 8, 0, 2), (8, 8, 65, 2), (8, 8, 2, 0), (-1, 8, 2, 2)):
        assert q(*bad) == 0, bad
    for shape in ((1, 1, 1, 1), (65, 200, 3, 5), (65, 1030, 3, 5), (65, 200, 8, 5), (65, 200, 9, 5),
                  (130, 200, 64, 130), (8192, 8192, 16, 64)):
        assert q(*shape) == R.workspace_bytes(*shape) and q(*shape) % 256 == 0, shape
    assert [R.split_slices(65, 200, 5), R.split_slices(65, 1030, 5), R.split_slices(8192, 8192, 64)] == [1, 2, 4]
    # two slices from 16 chunks on: 961 is the smallest B2 that takes two at the base shape, 1030 (17 chunks) an odd split
    assert R.split_slices(65, 960, 5) == 1 and R.split_slices(65, 961, 5) == 2


def test_python_surface_refusals_without_a_gpu():
    import neural_svd_amd
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import DotKernelOperator, MatrixFreeKernelOperator, RadialKernelOperator
    assert neural_svd_amd.DotKernelOperator is DotKernelOperator
    assert (H.DOT_POLYNOMIAL, H.DOT_ARCCOS1) == (R.POLYNOMIAL, R.ARCCOS1)
    assert issubclass(DotKernelOperator, MatrixFreeKernelOperator) and issubclass(RadialKernelOperator, MatrixFreeKernelOperator)
    for kw in (dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(coef0=-0.5),
               dict(coef0=float("nan")), dict(degree=0), dict(degree=9), dict(degree=2.5), dict(sigma=0.0)):
        with pytest.raises(ValueError):
            DotKernelOperator(H.DOT_POLYNOMIAL, 3, **kw)
    with pytest.raises(ValueError):
        DotKernelOperator(2, 3)
    with pytest.raises(NsvdError, match="GPU"):  # the arc-cosine kind ignores gamma, coef0, degree: past them, to the device
        DotKernelOperator(H.DOT_ARCCOS1, 3, gamma=0.0, coef0=-1.0, degree=0, device="cpu")
    with pytest.raises(NsvdError, match="dimension"):
        DotKernelOperator(H.DOT_ARCCOS1, 65)
    with pytest.raises(NsvdError, match="GPU"):
        DotKernelOperator(H.DOT_ARCCOS1, 3, device="cpu")
    x, y, f = torch.zeros(4, 3), torch.zeros(5, 3), torch.zeros(5, 2)
    with pytest.raises(NsvdError, match="GPU"):
        H.dot_apply(x, y, f, H.DOT_ARCCOS1, 1.0, 1.0, 2, 1.0)
    with pytest.raises(NsvdError, match="2-D"):
        H.dot_apply(x[0], y, f, H.DOT_ARCCOS1, 1.0, 1.0, 2, 1.0)
    with pytest.raises(NsvdError, match="y must be"):
        H.dot_apply(x, torch.zeros(5, 4), f, H.DOT_ARCCOS1, 1.0, 1.0, 2, 1.0)
    with pytest.raises(NsvdError, match="unsupported"):
        H.dot_apply_workspace(4, 5, 65, 2, "cpu")
