"""CPU tests of the deep ReLU kinds' float64 restatement (tests/_relu_kernel_oracle.py) and of the Python surface that
needs no GPU: the recursion against the order-1 arc-cosine oracle, against its own Gram-matrix form, against the
closed-form diagonal, positive semi-definiteness, one level against a Monte-Carlo estimate of the two Gaussian
expectations, the refusals and the zero-row convention."""
import math

import numpy as np
import pytest
import torch

from tests import _dot_oracle as DO
from tests import _relu_kernel_oracle as R

KINDS = {"nngp": R.RELU_NNGP, "ntk": R.RELU_NTK}
DEPTHS = (1, 2, 3, 8)
PARAMS = ((1.0, 0.0), (2.0, 0.1), (0.5, 1.0))  # (gamma, coef0)


@pytest.fixture(scope="module")
def points():
    return torch.randn(40, 3, generator=torch.Generator().manual_seed(11), dtype=torch.float64)


def test_depth_one_is_the_arc_cosine_kernel(points):
    want = DO.dot_kernel_matrix(points, points, DO.ARCCOS1)
    got = R.relu_kernel_matrix(points, points, R.RELU_NNGP, 1.0, 0.0, 1)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-15
    y = points[:7] * 1.5 + 0.25
    want = DO.dot_kernel_matrix(points, y, DO.ARCCOS1)
    got = R.relu_kernel_matrix(points, y, R.RELU_NNGP, 1.0, 0.0, 1)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-15


@pytest.mark.parametrize("gamma,coef0", PARAMS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_recursion_equals_the_gram_matrix_form(points, kind, depth, gamma, coef0):
    """closed-form diagonals q_l against each level's diagonal read off its own Gram: NNGP to 1e-14 relative; NTK to
    1e-6, the float64 image of A0's slope at c = 1 (the diagonal's c is 1 - O(1e-16) in the Gram form: sqrt(2e-16) / pi
    per level; 2e-8 seen)"""
    a = R.relu_kernel_matrix(points, points, KINDS[kind], gamma, coef0, depth)
    b = R.relu_gram_form(points, KINDS[kind], gamma, coef0, depth)
    e = float((a - b).abs().max() / a.abs().max())
    print(f"{kind} depth {depth} gamma {gamma} coef0 {coef0}: recursion against Gram form {e:.2e}")
    assert e <= (1e-14 if kind == "nngp" else 1e-6)


@pytest.mark.parametrize("gamma,coef0", PARAMS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_diagonal_and_positive_semi_definiteness(points, kind, depth, gamma, coef0):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import relu_kernel_diagonal
    assert (H.DOT_RELU_NNGP, H.DOT_RELU_NTK) == (R.RELU_NNGP, R.RELU_NTK)
    K = R.relu_kernel_matrix(points, points, KINDS[kind], gamma, coef0, depth)
    r2 = (points * points).sum(1).numpy()
    want = relu_kernel_diagonal(KINDS[kind], r2, gamma, coef0, depth)
    assert want.dtype == np.float64 and want.shape == r2.shape
    # the matrix's diagonal has c = 1 to rounding: exact for A1 (stationary), sqrt(2 * 1e-16) / pi per level for A0
    d = float(np.abs(K.diagonal().numpy() - want).max() / np.abs(want).max())
    assert d <= (1e-14 if kind == "nngp" else 1e-6), d
    assert float((K - K.T).abs().max()) <= 1e-14 * float(K.abs().max())
    ev = np.linalg.eigvalsh(((K + K.T) / 2).numpy())
    assert ev[0] >= -1e-12 * ev[-1], (ev[0], ev[-1])


def test_diagonal_closed_forms():
    """q_depth and sum_l gamma^(depth - l) q_l written out"""
    from neural_svd_amd.kernel_ops import relu_kernel_diagonal
    r2 = np.array([0.0, 0.3, 2.0])
    g, b = 2.0, 0.1
    q = [r2, g * r2 + b, g * (g * r2 + b) + b, g * (g * (g * r2 + b) + b) + b]
    np.testing.assert_allclose(relu_kernel_diagonal(R.RELU_NNGP, r2, g, b, 3), q[3], rtol=1e-15)
    np.testing.assert_allclose(relu_kernel_diagonal(R.RELU_NTK, r2, g, b, 3), q[3] + g * q[2] + g * g * q[1] + g ** 3 * q[0],
                               rtol=1e-15)
    np.testing.assert_allclose(relu_kernel_diagonal(R.RELU_NNGP, r2, 1.0, 0.0, 1), r2, rtol=0)
    for bad in (dict(kind=1), dict(depth=0), dict(depth=9), dict(depth=2.5)):
        kw = dict(dict(kind=R.RELU_NNGP, r2=r2, gamma=1.0, coef0=0.0, depth=1), **bad)
        with pytest.raises(ValueError):
            relu_kernel_diagonal(**kw)


@pytest.mark.parametrize("c", (-0.6, 0.3, 0.9))
def test_one_level_against_monte_carlo(c):
    """A1 = 2 E[relu u relu v] and A0 = 2 E[1{u>0} 1{v>0}] for unit Gaussians of correlation c: 4e6 seeded samples,
    within 5 standard errors computed from the sample"""
    n = 4_000_000
    rng = np.random.default_rng(1234)
    u = rng.standard_normal(n)
    v = c * u + math.sqrt(1.0 - c * c) * rng.standard_normal(n)
    A1, A0 = (float(t) for t in R.a1_a0(torch.tensor([c], dtype=torch.float64)))
    for want, sample in ((A1, 2.0 * np.maximum(u, 0.0) * np.maximum(v, 0.0)), (A0, 2.0 * ((u > 0) & (v > 0)))):
        mean, se = float(sample.mean()), float(sample.std(ddof=1)) / math.sqrt(n)
        print(f"c = {c}: exact {want:.6f} Monte Carlo {mean:.6f} +- {se:.1e}")
        assert abs(mean - want) <= 5.0 * se
    # and the level itself is these two: unit rows, gamma = 1, coef0 = 0
    x = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    y = torch.tensor([[c, math.sqrt(1.0 - c * c)]], dtype=torch.float64)
    assert abs(float(R.relu_kernel_matrix(x, y, R.RELU_NNGP, 1.0, 0.0, 1)) - A1) <= 1e-15
    assert abs(float(R.relu_kernel_matrix(x, y, R.RELU_NTK, 1.0, 0.0, 1)) - (A1 + c * A0)) <= 1e-15


def test_python_surface_refusals_without_a_gpu():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import DotKernelOperator
    for kind in (H.DOT_RELU_NNGP, H.DOT_RELU_NTK):
        for kw in (dict(depth=0), dict(depth=9), dict(depth=2.5), dict(gamma=0.0), dict(gamma=float("nan")),
                   dict(gamma=float("inf")), dict(coef0=-0.5), dict(coef0=float("nan"))):
            with pytest.raises(ValueError):
                DotKernelOperator(kind, 3, **kw)
        # valid parameters reach the device check; degree is ignored on the way
        with pytest.raises(NsvdError, match="GPU"):
            DotKernelOperator(kind, 3, gamma=2.0, coef0=0.0, depth=8, degree=0, device="cpu")
    with pytest.raises(ValueError):
        DotKernelOperator(2, 3, depth=1)
    x, y, f = torch.zeros(4, 3), torch.zeros(5, 3), torch.zeros(5, 2)
    with pytest.raises(NsvdError, match="GPU"):
        H.dot_apply(x, y, f, H.DOT_RELU_NTK, 1.0, 0.0, 3, 1.0)
    with pytest.raises(NsvdError, match="GPU"):
        H.dot_apply_pair(x, y, f, torch.zeros(4, 2), H.DOT_RELU_NNGP, 1.0, 0.0, 3, 1.0, 1.0)


@pytest.mark.parametrize("kind", list(KINDS))
def test_zero_row_gives_coef0_only_values(points, kind):
    """p = 0 takes both A terms as 0: level 1 of a zero row is coef0 whatever the other row; deeper levels then run on
    q_1 = coef0. With coef0 = 0 the row stays exactly 0 at every depth. Never a NaN."""
    x = points[:6].clone()
    x[2] = 0.0
    for depth in DEPTHS:
        for gamma, coef0 in PARAMS:
            K = R.relu_kernel_matrix(x, points, KINDS[kind], gamma, coef0, depth)
            assert bool(torch.isfinite(K).all())
            if coef0 == 0.0:
                assert bool((K[2] == 0).all())
            if depth == 1:
                assert bool((K[2] == coef0).all())
            # the zero row's values depend on the other row through coef0-derived quantities only: the same recursion
            # started from S_1 = T_1 = coef0, q_1(x) = coef0, q_1(y) = gamma |y|^2 + coef0
            S = torch.full((points.shape[0],), coef0, dtype=torch.float64)
            T = S.clone()
            qx, qy = torch.tensor(coef0, dtype=torch.float64), gamma * (points * points).sum(1) + coef0
            for _ in range(depth - 1):
                S, T = R._level(S, T, torch.sqrt(qx * qy), gamma, coef0)
                qx, qy = gamma * qx + coef0, gamma * qy + coef0
            want = S if kind == "nngp" else T
            assert float((K[2] - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))
    Kz = R.relu_kernel_matrix(x, x, KINDS[kind], 2.0, 0.1, 3)
    assert bool(torch.isfinite(Kz).all()) and float(Kz[2].min()) >= 0.0 and float(Kz[:, 2].min()) >= 0.0
