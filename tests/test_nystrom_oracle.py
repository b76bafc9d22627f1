"""CPU checks of the Nystrom baseline's ground truth (tests/_nystrom_oracle.py): the float64 definition (a) against the
golden captured from the reference's own Nystrom (tests/golden/nystrom.npz, make_golden_nystrom.py), the recurrence (b)
the device solver runs against (a) at the shapes of tests/test_nystrom_gpu.py, and the host side of the new entry points."""
import os

import numpy as np
import pytest
import torch

from tests import _nystrom_oracle as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nystrom.npz")
KINDS = {"gaussian": N.GAUSSIAN, "exponential": N.EXPONENTIAL}


@pytest.mark.parametrize("kind", list(KINDS))
def test_definition_against_the_reference(kind):
    """Eigenvalues within 1e-6 of the largest; projections per column, up to sign, within 2e-6 of that column's max.
    The reference's float32 eigh is 1e-8 / 3e-8 from float64 on the eigenvalues and <= 4.7e-7 on the projections of
    this fixture, whose relative gaps are >= 0.007."""
    z = np.load(GOLDEN)
    xs, xnew, dim, ell = torch.tensor(z["xs"]), torch.tensor(z["xnew"]), int(z["dim"]), float(z[f"ell_{kind}"])
    w, U, w_all = N.definition(xs, KINDS[kind], ell, dim)
    assert N.eigen_gaps(w_all, dim).min() >= 0.007
    ev = np.abs(z[f"eigvals_{kind}"] - w).max() / w[0]
    print(f"{kind}: eigenvalues {ev:.1e} of the largest")
    assert ev <= 1e-6
    assert np.abs(np.abs(np.sum(z[f"eigvecs_{kind}"] * U, axis=0)) - 1.0).max() <= 1e-5
    want = N.project(xnew, xs, KINDS[kind], ell, w, U)
    got = z[f"proj_{kind}"].astype(np.float64)
    assert got.shape == want.shape == (40, dim)
    sign = np.sign(np.sum(got * want, axis=0))
    err = np.abs(got * sign - want).max(axis=0) / np.abs(want).max(axis=0)
    print(f"{kind}: projections " + " ".join(f"{e:.1e}" for e in err))
    assert err.max() <= 2e-6


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_recurrence_against_definition(case):
    """Recurrence (b) with float32 blocks (what the device stores) converges to tol = 1e-5 within 27 iterations
    (Gaussian kind) resp. 29 (the exponential case) and lands on the TOP eigenpairs of (a): every relative
    gap among the first L + 1 eigenvalues is >= 1e-4, eigenvalues within 2 tol lambda_0, true residuals within 2 tol.
    Measured iterations, in the order of CASES: 2 7 6 7 27 5 3 3 1 9 4."""
    n, D, L, kind, ell, shift = case
    s = N.solved(case)
    rec, w, G = s["rec"], s["w"], s["G"]
    gaps = N.eigen_gaps(w, L)
    print(f"{N.case_id(case)}: {rec['iterations']} iterations, min gap {gaps.min():.1e}, worst residual "
          f"{rec['residuals'].max():.1e}")
    assert gaps.min() >= N.MIN_GAP
    assert rec["converged"]
    assert rec["iterations"] <= (N.MAX_ITERS_GAUSSIAN if kind == N.GAUSSIAN else N.MAX_ITERS_EXPONENTIAL)
    assert np.abs(rec["eigvals"] - w[:L]).max() <= 2e-5 * w[0]
    true_res = np.linalg.norm(G @ rec["eigvecs"] - rec["eigvecs"] * rec["eigvals"], axis=0)
    assert true_res.max() <= 2e-5 * w[0]


def test_identity_gram_floors_the_residual_without_the_basis_gram():
    """Why step 3 takes C = V^T V: on an exact eigenpair whose vector is stored in float32, sqrt(M_kk - theta_k^2)
    reads ~theta sqrt(|1 - |v|^2|) (1e-5 .. 1e-4 theta), the corrected formula ~1e-8 theta or less."""
    xs, _ = N.case_points(N.CASES[0])
    G = N.gram(xs, N.GAUSSIAN, 1.5)
    w, U, _ = N.definition(xs, N.GAUSSIAN, 1.5, 6)
    V = U.astype(np.float32).astype(np.float64)
    W = G @ V
    plain = N.ritz_step(W.T @ W, V.T @ W)[1]
    fixed = N.ritz_step(W.T @ W, V.T @ W, V.T @ V)[1]
    print("plain", plain / w[0], "with C", fixed / w[0])
    assert fixed.max() <= 1e-7 * w[0]
    assert plain.max() >= 10.0 * max(fixed.max(), 1e-9 * w[0])


def test_flat_spectrum_is_reported_not_hidden():
    """exponential kind, n = 70, L = 64 (m = 70 = n would be exact: oversample 2 keeps m = 66 < n): the rate
    lambda_(m+1) / lambda_L is close to 1 and 40 iterations do not reach 1e-5"""
    g = torch.Generator().manual_seed(3)
    xs = torch.randn(70, 3, generator=g)
    rec = N.subspace_iteration(N.gram(xs, N.EXPONENTIAL, 2.0), 64, oversample=2, max_iters=40)
    assert not rec["converged"] and rec["iterations"] == 40
    assert np.isfinite(rec["residuals"]).all() and rec["residuals"].max() > 1e-5


def test_ritz_step_restatement():
    rng = np.random.default_rng(0)
    V, _ = np.linalg.qr(rng.standard_normal((50, 7)))
    X = rng.standard_normal((50, 50))
    G = X @ X.T / 50
    W = G @ V
    theta, resid, Q, T = N.ritz_step(W.T @ W, V.T @ W)
    assert np.all(np.diff(theta) <= 0)
    assert np.abs(Q.T @ Q - np.eye(7)).max() < 1e-13
    assert np.abs(T.T @ (W.T @ W) @ T - np.eye(7)).max() < 1e-10
    direct = np.linalg.norm(W @ Q - (V @ Q) * theta, axis=0)
    assert np.abs(resid - direct).max() < 1e-10 * theta[0]
    _, _, Q0, T0 = N.ritz_step(W.T @ W, None)
    assert np.array_equal(Q0, np.eye(7)) and np.abs(np.tril(T0, -1)).max() == 0.0
    assert np.abs(T0.T @ (W.T @ W) @ T0 - np.eye(7)).max() < 1e-10


def test_abi_version_workspace_and_refusals():
    """host side only: the entry points refuse out-of-range shapes before anything is launched"""
    from neural_svd_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 6 and lib.nsvd_abi_version() == 6
    q = lib.nsvd_tsgram_f64_workspace_bytes
    for bad in ((0, 8), (8, 0), (8, 81), (-1, 8), (8, -1)):
        assert q(*bad) == 0, bad
    for shape in ((1, 1), (63, 13), (64, 64), (65, 80), (1030, 13), (4100, 80), (8192, 18), (65536, 72), (10 ** 6, 80)):
        assert q(*shape) == N.tsgram_workspace_bytes(*shape) and q(*shape) % 256 == 0, shape
    assert [N.tsgram_slices(n) for n in (1, 64, 65, 8192, 8193, 10 ** 6)] == [1, 1, 2, 128, 128, 128]
    p = 4096  # a non-null, 256-byte aligned stand-in: nothing dereferences it before the refusal
    big = 1 << 30
    for n, m, want in ((8, 0, _lib.EINVAL), (8, 81, _lib.EUNSUPPORTED), (0, 8, _lib.EINVAL)):
        assert lib.nsvd_tsgram_f64(p, max(m, 1), p, max(m, 1), n, m, p, p, p, big, None) == want, (n, m)
        assert lib.nsvd_ts_rotate(p, max(m, 1), n, m, p, max(m, 1), max(min(m, 1), 1), p, max(m, 1), None) == want, (n, m)
        if n:
            assert lib.nsvd_ritz_step_f64(p, p, None, m, p, p, p, p, p, None) == want, m
    E = _lib.EINVAL
    assert lib.nsvd_tsgram_f64(p, 8, p, 8, 16, 8, None, None, p, big, None) == E      # nothing to compute
    assert lib.nsvd_tsgram_f64(p, 8, None, 0, 16, 8, p, p, p, big, None) == E         # XtY without Y
    assert lib.nsvd_tsgram_f64(p, 7, None, 0, 16, 8, p, None, p, big, None) == E      # ldx < m
    assert lib.nsvd_tsgram_f64(p, 8, None, 0, 16, 8, p, None, p, 256, None) == E      # workspace too small
    assert lib.nsvd_tsgram_f64(p, 8, None, 0, 16, 8, p, None, p + 8, big, None) == E  # workspace misaligned
    assert lib.nsvd_ts_rotate(p, 8, 16, 8, p, 8, 9, p, 9, None) == E                  # k > m
    assert lib.nsvd_ts_rotate(p, 8, 16, 8, p, 8, 0, p, 8, None) == E                  # k = 0
    assert lib.nsvd_ritz_step_f64(None, p, None, 8, p, p, p, p, p, None) == E
    assert lib.nsvd_ritz_step_f64(p, p, None, 8, p, p, p, p, None, None) == E         # no status word


def test_nystrom_refuses_cpu_tensors_and_bad_dims():
    from neural_svd_amd import Nystrom
    from neural_svd_amd._lib import NsvdError

    def k(a, b):
        return torch.exp(-torch.cdist(a, b) ** 2)
    with pytest.raises(NsvdError, match="GPU"):
        Nystrom(k, torch.zeros(20, 2), 3)
