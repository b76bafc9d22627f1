"""CPU checks of the kernel SVD path's ground truth: the closed-form singular values of the Gaussian kernel between two
Gaussian measures against a quadrature SVD, their agreement with the one-measure eigenvalues, the host-side ABI queries
of nsvd_rbf_apply_pair, and the Python refusals that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _pair_oracle as P

PARAMS = ((1.0, 0.5, 1.5), (0.7, 1.3, 0.9), (2.0, 0.4, 1.0), (1.0, 1.0, 1.5), (0.3, 0.6, 2.5))  # sigma_x, sigma_y, ell


@pytest.mark.parametrize("sigma_x,sigma_y,ell", PARAMS)
def test_closed_form_against_quadrature_svd(sigma_x, sigma_y, ell):
    """s_n = s_0 rho^n against the SVD of diag(sqrt w_x) K diag(sqrt w_y) on 160 x 160 Gauss-Hermite nodes, n < 8, in
    1-D; in 2-D the products of the quadrature values, in the closed form's order. Bound 1e-10 (absolute; s_0 <= 1)."""
    from neural_svd_amd.kernel_ops import gaussian_cross_modes, gaussian_cross_singular_values
    q = P.quadrature_singular_values(sigma_x, sigma_y, ell, 8)
    s = gaussian_cross_singular_values(sigma_x, sigma_y, ell, 1, 8)
    print(f"sigma_x {sigma_x} sigma_y {sigma_y} ell {ell}: s_0 {s[0]:.6f} rho {s[1] / s[0]:.6f} "
          f"max error {np.abs(s - q).max():.1e}")
    assert s.dtype == np.float64 and np.abs(s - q).max() < 1e-10
    vals, idx = gaussian_cross_modes(sigma_x, sigma_y, ell, 2, 10)
    assert idx.tolist() == [[0, 0], [1, 0], [0, 1], [2, 0], [1, 1], [0, 2], [3, 0], [2, 1], [1, 2], [0, 3]]
    assert np.abs(vals - q[idx[:, 0]] * q[idx[:, 1]]).max() < 1e-10
    assert np.all(np.diff(vals) <= 1e-15)


def test_the_issue_example_and_the_one_measure_limit():
    from neural_svd_amd.kernel_ops import gaussian_cross_singular_values, gaussian_kernel_eigvals
    s = gaussian_cross_singular_values(1.0, 0.5, 1.5, 1, 3)
    assert abs(s[0] - 0.82028) < 5e-6 and abs(s[1] / s[0] - 0.14952) < 5e-6
    for sigma, ell, dim in ((1.0, 1.5, 1), (0.7, 0.9, 3), (2.0, 1.0, 2)):
        a, b = gaussian_cross_singular_values(sigma, sigma, ell, dim, 12), gaussian_kernel_eigvals(sigma, ell, dim, 12)
        assert np.abs(a - b).max() < 1e-14, (sigma, ell, dim)
    # the order of the two measures does not matter to the values (K and K^T share them)
    assert np.array_equal(gaussian_cross_singular_values(1.0, 0.5, 1.5, 2, 6),
                          gaussian_cross_singular_values(0.5, 1.0, 1.5, 2, 6))


def test_svd_step_restatement_is_the_autograd_gradient():
    """tests/_pair_oracle.py:svd_step's gradients against torch autograd on its own loss, float64"""
    g = torch.Generator().manual_seed(3)
    f, Tg, gg, Ta = (torch.randn(17, 5, generator=g, dtype=torch.float64) for _ in range(4))
    v = torch.tensor([1.0, 1.0, 0.5, 0.5, 0.25], dtype=torch.float64)
    M = torch.minimum(v[:, None], v[None, :])
    f.requires_grad_(True)
    gg.requires_grad_(True)
    loss, df, dg = P.svd_step(f, Tg, gg, Ta, v, M)
    loss.backward()
    assert torch.allclose(f.grad, df.detach(), rtol=1e-12, atol=1e-14)
    # (autograd sees no path from the loss to g through Tadjf: the Function's d loss / d g carries the operator term of
    # the symmetric form, which equals d/dg of -2 mean f . (K g) when Tadjf = K^T f / B1)
    K = torch.randn(17, 17, generator=g, dtype=torch.float64)
    f2, g2 = f.detach().clone().requires_grad_(True), gg.detach().clone().requires_grad_(True)
    loss2, df2, dg2 = P.svd_step(f2, K @ g2 / 17, g2, (K.T @ f2 / 17).detach(), v, M)
    loss2.backward()
    _, _, dg_fn = P.svd_step(f2.detach(), (K @ g2 / 17).detach(), g2.detach(), (K.T @ f2 / 17).detach(), v, M)
    assert torch.allclose(g2.grad, dg_fn, rtol=1e-12, atol=1e-14)


def test_workspace_and_partition_queries():
    from neural_svd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.nsvd_abi_version() == 6
    q, part = lib.nsvd_rbf_apply_pair_workspace_bytes, lib.nsvd_rbf_apply_pair_partition
    rg, cs = ctypes.c_int(-5), ctypes.c_int(-5)
    for bad in ((0, 8, 2, 2), (8, 0, 2, 2), (8, 8, 0, 2), (8, 8, 65, 2), (8, 8, 2, 0), (-1, 8, 2, 2)):
        assert q(*bad) == 0, bad
        assert part(*bad, ctypes.byref(rg), ctypes.byref(cs)) != 0 and (rg.value, cs.value) == (-5, -5), bad
    assert part(8, 8, 65, 2, ctypes.byref(rg), ctypes.byref(cs)) == _lib.EUNSUPPORTED
    assert part(8, 8, 2, 2, None, ctypes.byref(cs)) == _lib.EINVAL and part(8, 8, 2, 2, ctypes.byref(rg), None) == _lib.EINVAL
    for shape in ((1, 1, 1, 1), (65, 200, 3, 5), (65, 257, 3, 5), (130, 1030, 64, 130), (8192, 8192, 16, 64)):
        assert q(*shape) == P.pair_workspace_bytes(*shape) and q(*shape) % 256 == 0, shape
        assert part(*shape, ctypes.byref(rg), ctypes.byref(cs)) == 0
        assert (rg.value, cs.value) == P.pair_split(shape[0], shape[1], shape[3]), shape
    assert [P.pair_split(65, 200, 5), P.pair_split(65, 257, 5), P.pair_split(130, 1030, 65),
            P.pair_split(8192, 8192, 64)] == [(2, 1), (2, 2), (2, 4), (32, 16)]


def test_workspace_is_monotone_and_the_copies_are_capped():
    """more rows never need less workspace; never more than 32 partial copies of either output, up to 65 536 rows"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd import _lib
    q = _lib.load().nsvd_rbf_apply_pair_workspace_bytes
    sizes = (1, 63, 64, 65, 130, 257, 1030, 4096, 8192, 8193, 16384, 40000, 65536)
    for D, L in ((1, 1), (3, 5), (16, 64), (64, 130)):
        for fixed in (1, 200, 8192):
            a = [q(B, fixed, D, L) for B in sizes]
            b = [q(fixed, B, D, L) for B in sizes]
            assert a == sorted(a) and b == sorted(b), (D, L, fixed)
        for B1 in sizes:
            for B2 in sizes:
                rg, cs = H.rbf_apply_pair_partition(B1, B2, D, L)
                assert 1 <= rg <= min(32, (B1 + 63) // 64) and 1 <= cs <= min(32, (B2 + 255) // 256), (B1, B2, D, L)


def test_python_refusals_without_a_gpu():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator, kernel_singular_values
    from neural_svd_amd.kernel_svd import KernelSvdTrainer, PairedFunctions
    from neural_svd_amd.nested_lowrank import NestedLoRA
    x, y, g, f = torch.zeros(8, 2), torch.zeros(9, 2), torch.zeros(9, 3), torch.zeros(8, 3)
    with pytest.raises(NsvdError, match="GPU"):
        H.rbf_apply_pair(x, y, g, f, H.RBF_GAUSSIAN, 1.0, 1.0, 1.0)
    with pytest.raises(NsvdError):
        H.rbf_apply_pair(x, y, g, f[:, :2], H.RBF_GAUSSIAN, 1.0, 1.0, 1.0)
    with pytest.raises(NsvdError, match="unsupported"):
        H.rbf_apply_pair_workspace(8, 8, 65, 3, "cpu")
    with pytest.raises(NsvdError, match="unsupported"):
        H.rbf_apply_pair_partition(8, 8, 65, 3)
    with pytest.raises(NsvdError, match="invalid"):
        H.rbf_apply_pair_partition(0, 8, 2, 3)
    with pytest.raises(NsvdError, match="GPU"):
        RadialKernelOperator(H.RBF_GAUSSIAN, 1.0, 2, 1.0, "cpu")
    with pytest.raises(NsvdError, match="GPU"):
        kernel_singular_values(None, None, None, x, y)
    pair = PairedFunctions(torch.nn.Linear(2, 3), torch.nn.Linear(2, 3))
    assert isinstance(pair.f, torch.nn.Linear) and len(list(pair.parameters())) == 4
    method = NestedLoRA(pair, 3)
    with pytest.raises(NsvdError, match="B1 == B2"):
        method.compute_loss_kernel_svd(lambda *a, **k: None, x, y)
    with pytest.raises(NsvdError, match="PairedFunctions"):
        NestedLoRA(torch.nn.Linear(2, 3), 3).compute_loss_kernel_svd(lambda *a, **k: None, x, x)
    with pytest.raises(NsvdError, match="callable"):
        method.compute_loss_kernel_svd(None, x, x)
    with pytest.raises(NotImplementedError):
        KernelSvdTrainer(object(), L=3, m=64)
