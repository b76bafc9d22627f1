"""CPU checks of the radial kernel operator's ground truth: the float64 oracle against the golden's definition, the
closed-form Mercer spectrum of the Gaussian kernel under a Gaussian measure (values and eigen-equation), and the
host-side ABI queries of nsvd_rbf_apply."""
import numpy as np
import torch

from oracle import nsvd_oracle as O
from tests import _rbf_oracle as R


def test_gaussian_kind_is_the_goldens_definition():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(37, 5, generator=g, dtype=torch.float64)
    y = torch.randn(51, 5, generator=g, dtype=torch.float64) + 0.3
    f = torch.randn(51, 7, generator=g, dtype=torch.float64)
    want = O.gaussian_kernel_apply(x, y, f, 1.7)
    got = R.radial_kernel_apply(x, y, f, R.GAUSSIAN, 1.7, 1.0 / 51)
    assert float((got - want).abs().max() / want.abs().max()) < 1e-14
    # the exponential kind at a hand-checked pair: d = 5, ell = 2
    e = R.radial_kernel_apply(torch.tensor([[0.0, 0.0]]), torch.tensor([[3.0, 4.0]]), torch.tensor([[2.0]]),
                              R.EXPONENTIAL, 2.0, 0.5)
    assert abs(float(e) - np.exp(-2.5)) < 1e-15


def test_gaussian_kernel_eigvals_closed_form():
    from neural_svd_amd.kernel_ops import gaussian_kernel_eigvals
    one_d = gaussian_kernel_eigvals(1.0, 1.5, 1, 6)
    assert one_d.dtype == np.float64 and one_d.tolist() == [0.75 * 0.25 ** k for k in range(6)]
    two_d = gaussian_kernel_eigvals(1.0, 1.5, 2, 10)
    assert two_d.tolist() == [0.5625] + [0.140625] * 2 + [0.03515625] * 3 + [0.0087890625] * 4


def test_eigen_equation_by_gauss_hermite_quadrature():
    """E_p[k(x, y) phi_k(y)] = lambda_k phi_k(x) for p = N(0, sigma^2), k < 6, at seven x in [-3, 3]: 120-point
    Gauss-Hermite quadrature in float64. Residual relative to max_x |lambda_k phi_k(x)|: 6e-16 (k = 0) to 3e-14 (k = 5) measured; also at a
    second (sigma, ell) whose constants are not dyadic."""
    from neural_svd_amd.kernel_ops import gaussian_kernel_eigenfunctions, gaussian_kernel_eigvals
    t, w = np.polynomial.hermite.hermgauss(120)
    xs = torch.linspace(-3.0, 3.0, 7, dtype=torch.float64).reshape(-1, 1)
    for sigma, ell in ((1.0, 1.5), (0.7, 0.9)):
        y = torch.tensor(np.sqrt(2.0) * sigma * t).reshape(-1, 1)
        wq = torch.tensor(w / np.sqrt(np.pi))
        lam = torch.tensor(gaussian_kernel_eigvals(sigma, ell, 1, 6))
        K = R.radial_kernel_matrix(xs, y, R.GAUSSIAN, ell)
        lhs = K @ (wq[:, None] * gaussian_kernel_eigenfunctions(y, sigma, ell, 6))
        rhs = lam[None, :] * gaussian_kernel_eigenfunctions(xs, sigma, ell, 6)
        res = ((lhs - rhs).abs().max(dim=0).values / rhs.abs().max(dim=0).values).tolist()
        print(f"sigma {sigma} ell {ell}: eigen-equation residuals " + " ".join(f"{r:.1e}" for r in res))
        assert max(res) < 1e-12, res


def test_two_dimensional_modes_are_products():
    from neural_svd_amd.kernel_ops import gaussian_kernel_eigenfunctions, gaussian_kernel_modes
    vals, idx = gaussian_kernel_modes(1.0, 1.5, 2, 6)
    assert idx.tolist() == [[0, 0], [1, 0], [0, 1], [2, 0], [1, 1], [0, 2]]
    x = torch.randn(9, 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    phi2 = gaussian_kernel_eigenfunctions(x, 1.0, 1.5, 6)
    phi1 = [gaussian_kernel_eigenfunctions(x[:, d:d + 1], 1.0, 1.5, 3) for d in range(2)]
    for col, (k0, k1) in enumerate(idx.tolist()):
        assert torch.allclose(phi2[:, col], phi1[0][:, k0] * phi1[1][:, k1], rtol=1e-14, atol=0)


def test_abi_version_and_workspace_queries():
    from neural_svd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.nsvd_abi_version() == 6
    q = lib.nsvd_rbf_apply_workspace_bytes
    for bad in ((0, 8, 2, 2), (8, 0, 2, 2), (8, 8, 0, 2), (8, 8, 65, 2), (8, 8, 2, 0), (-1, 8, 2, 2)):
        assert q(*bad) == 0, bad
    for shape in ((1, 1, 1, 1), (65, 200, 3, 5), (65, 1030, 3, 5), (130, 200, 64, 130), (8192, 8192, 16, 64)):
        assert q(*shape) == R.workspace_bytes(*shape) and q(*shape) % 256 == 0, shape
    # the split rule as the tests restate it: one slice at the small shapes, two at B2 = 1030, four at the bench size
    assert [R.split_slices(65, 200, 5), R.split_slices(65, 1030, 5), R.split_slices(8192, 8192, 64)] == [1, 2, 4]
