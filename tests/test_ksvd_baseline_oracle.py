"""CPU checks of the truncated-SVD baseline's recurrence (tests/_ksvd_oracle.py): the two-sided block iteration (b) with
float32 products and stored bases against the float64 definition (a), the residual identity it stops on, and the reason
the short residual form is not used. No GPU."""
import numpy as np
import pytest
import torch

from tests import _ksvd_oracle as K

TOL = 1e-5


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_recurrence_against_definition(case):
    kind, nx, ny, D, dim, over = case
    s = K.solved(case)
    C, rec = s["C"], s["rec"]
    s0 = s["s"][0]
    assert rec["converged"] and rec["iterations"] <= 40
    assert np.abs(rec["svals"] - s["s"]).max() <= 2 * TOL * s0
    # the claimed residuals are the residuals of the Ritz triplets under the float32 operator the iteration applied, to
    # two digits (the claim is relative to the step's own sigma_0)
    C32 = C.astype(np.float32).astype(np.float64)
    U, V, sv = rec["left64"], rec["right64"], rec["svals"]
    claimed = np.maximum(np.linalg.norm(C32 @ V - U * sv, axis=0), np.linalg.norm(C32.T @ U - V * sv, axis=0)) / sv[0]
    # (plus the rounding of the float32 products P and R themselves, which the claim sees and C32 @ V in float64 does
    # not: |P - C32 V| <= ~eps32 sigma_0 a column, on either side)
    assert np.all(np.abs(rec["residuals"] - claimed) <= 0.01 * claimed + 2 * np.finfo(np.float32).eps), \
        (rec["residuals"], claimed)
    # and the returned (float32) triplets under the exact C
    U, V = rec["left"], rec["right"]
    true = np.maximum(np.linalg.norm(C @ V - U * sv, axis=0), np.linalg.norm(C.T @ U - V * sv, axis=0)) / s0
    print(f"{K.case_id(case)}: iterations {rec['iterations']}, claimed {rec['residuals'].max():.1e}, true {true.max():.1e},"
          f" sigma {np.abs(rec['svals'] - s['s']).max() / s0:.1e}")
    assert true.max() <= 2 * TOL
    assert np.abs(U.T @ U - np.eye(dim)).max() <= 2e-6 and np.abs(V.T @ V - np.eye(dim)).max() <= 2e-6


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_half_the_columns_are_separated(case):
    """the vector checks on the GPU skip a column only below a relative gap of 0.005: at least half stay"""
    kind, nx, ny, D, dim, over = case
    gaps = K.relative_gaps(K.solved(case)["s_all"], dim)
    assert 2 * int((gaps >= K.MIN_GAP).sum()) >= dim, gaps


def test_short_residual_form_stalls():
    """Mp_kk - sigma_k^2 in place of the three-term form: the claimed residual sits on a floor above tol = 1e-5 for 200
    iterations on at least one case, while the true residual of the same iterates is far below it"""
    stalled = []
    for case in K.CASES[:4]:
        kind, nx, ny, D, dim, over = case
        C = K.solved(case)["C"]
        rec = K.two_sided_iteration(C, dim, over, tol=TOL, max_iters=200, short_residual=True)
        U, V, sv = rec["left"], rec["right"], rec["svals"]
        true = np.maximum(np.linalg.norm(C @ V - U * sv, axis=0), np.linalg.norm(C.T @ U - V * sv, axis=0)) / sv[0]
        print(f"{K.case_id(case)}: short form claimed {rec['residuals'].max():.1e} after {rec['iterations']} iterations, "
              f"true {true.max():.1e}")
        if not rec["converged"]:
            assert true.max() <= TOL  # the iterates themselves had converged: only the claim had not
            stalled.append(K.case_id(case))
    assert stalled


def test_svd_ritz_step_identities():
    """the small step on a real iteration state: the three-term residuals equal the direct norms for bases that are NOT
    orthonormal, and P Tu, R Tv are orthonormal with the Ritz directions leading"""
    case = K.CASES[1]
    kind, nx, ny, D, dim, over = case
    C = K.solved(case)["C"]
    rng = np.random.default_rng(3)
    m = 13
    U, V = rng.standard_normal((nx, m)) / np.sqrt(nx), rng.standard_normal((ny, m)) / np.sqrt(ny)
    Pm, Rm = C @ V, C.T @ U
    sigma, rl, rr, A, B, Tu, Tv = K.svd_ritz_step(Pm.T @ U, Rm.T @ V, Pm.T @ Pm, Rm.T @ Rm, U.T @ U, V.T @ V)
    dl = np.linalg.norm(Pm @ B - (U @ A) * sigma, axis=0)
    dr = np.linalg.norm(Rm @ A - (V @ B) * sigma, axis=0)
    assert np.abs(rl - dl).max() <= 1e-9 * sigma[0] and np.abs(rr - dr).max() <= 1e-9 * sigma[0]
    I = np.eye(m)
    assert np.abs((Pm @ Tu).T @ (Pm @ Tu) - I).max() <= 1e-8 and np.abs((Rm @ Tv).T @ (Rm @ Tv) - I).max() <= 1e-8
    assert np.abs(np.tril(B.T @ Tu, -1)).max() <= 1e-10 * np.abs(B.T @ Tu).max()
    assert np.abs(np.tril(A.T @ Tv, -1)).max() <= 1e-10 * np.abs(A.T @ Tv).max()


def test_workspace_formula_matches_the_library():
    from neural_svd_amd import _lib
    lib = _lib.load()
    for n in (1, 63, 64, 65, 1030, 4100, 8192, 100000):
        for m in (1, 13, 64, 80):
            assert lib.nsvd_tsgram3_f64_workspace_bytes(n, m) == K.tsgram3_workspace_bytes(n, m)
    assert lib.nsvd_tsgram3_f64_workspace_bytes(0, 4) == 0 and lib.nsvd_tsgram3_f64_workspace_bytes(4, 81) == 0
    assert lib.nsvd_tsgram3_f64_workspace_bytes(4, 0) == 0


def test_refuses_cpu_tensors():
    from neural_svd_amd import NystromSVD
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    xs, ys = torch.randn(20, 2), torch.randn(15, 2)
    with pytest.raises(NsvdError, match="GPU"):
        NystromSVD(lambda a, b: a @ b.T, xs, ys, 3)
    with pytest.raises(NsvdError):
        H.tsgram3_f64(torch.zeros(8, 2), torch.zeros(8, 2))
    z = torch.zeros(2, 2, dtype=torch.float64)
    with pytest.raises(NsvdError):
        H.svd_ritz_step_f64(z, z, z, z, torch.zeros(1, dtype=torch.int32))
