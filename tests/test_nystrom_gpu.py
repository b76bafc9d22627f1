"""GPU tests of the Nystrom baseline on HIP: the three kernels of csrc/nystrom.hip alone (nsvd_tsgram_f64,
nsvd_ritz_step_f64, nsvd_ts_rotate) against float64, and neural_svd_amd.Nystrom against the float64 definition and the
recurrence of tests/_nystrom_oracle.py.

Bounds of the solver tests follow the repository's convention max(floor, 4 x yardstick): the yardstick is the same
quantity from the reference's op sequence on the same GPU (a float32 Gram by torch ops, copied to the host, float32
np.linalg.eigh) against the same float64 oracle. Both are printed by every test.

Measured on an MI355X: the tables in the docstrings of the tests (the whole file: 77 tests in 3.5 s).
"""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import _nystrom_oracle as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
NS, MS = (1, 63, 64, 65, 1030, 4100), (1, 13, 64, 80)
# the Gram kernels' slice count stops at 128 from n = 8192 on: 8200 rows go to 128 slices of 64 or 65 rows
GRAM_SHAPES = [(n, m) for n in NS for m in MS] + [(8200, 13), (8200, 80)]


def _rel(got, want):
    want = want.double()
    return float((got.double() - want).abs().max() / want.abs().max())


def _block(n, m, seed, ld=None):
    g = torch.Generator().manual_seed(seed + 100 * n + m)
    full = torch.randn(n, ld or m, generator=g).to(DEV)
    return full[:, :m] if ld else full


# ---- nsvd_tsgram_f64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", GRAM_SHAPES)
def test_tsgram_against_float64(n, m):
    """X^T X and X^T Y against float64 torch on the same float32 inputs, rel <= 1e-13; Y strided (ld = m + 7); two calls
    give the same bits. Measured: worst rel 1.8e-14 (n = 8200, m = 80: the slice cap); 6.6e-15 at n = 4100, 2.6e-15 at
    n = 1030."""
    from neural_svd_amd import hip_ops as H
    X, Y = _block(n, m, 1), _block(n, m, 2, ld=m + 7)
    assert Y.stride(0) == m + 7
    xx, xy = H.tsgram_f64(X, Y)
    wxx, wxy = X.double().T @ X.double(), X.double().T @ Y.double()
    e = max(_rel(xx, wxx), _rel(xy, wxy))
    print(f"tsgram n={n} m={m}: rel {e:.1e}")
    assert xx.dtype == torch.float64 and tuple(xy.shape) == (m, m)
    assert e <= 1e-13
    xx2, xy2 = H.tsgram_f64(X, Y)
    assert torch.equal(xx, xx2) and torch.equal(xy, xy2)
    # one output at a time: the same bits
    assert torch.equal(H.tsgram_f64(X)[0], xx) and torch.equal(H.tsgram_f64(X, Y, xtx=False)[1], xy)


def test_tsgram_strided_x_and_y_is_x():
    from neural_svd_amd import hip_ops as H
    n, m = 1030, 13
    Xs = _block(n, m, 3, ld=m + 3)
    Xc = Xs.contiguous()
    xx, xy = H.tsgram_f64(Xs, Xs)
    assert torch.equal(xx, xy)                      # Y == X: the two products are the same sums
    assert torch.equal(xx, H.tsgram_f64(Xc)[0])     # the stride changes nothing
    assert torch.equal(xx, xx.T)                    # bitwise symmetric
    assert _rel(xx, Xc.double().T @ Xc.double()) <= 1e-13
    ws = H.tsgram_workspace(n, m, DEV)
    out = torch.empty((m, m), dtype=torch.float64, device=DEV)
    assert H.tsgram_f64(Xc, ws=ws, out_xtx=out)[0] is out and torch.equal(out, xx)


# ---- nsvd_ritz_step_f64 -----------------------------------------------------------------------------------------------
def _ritz_inputs(m, store32=False):
    """S = W^T W, A = V^T W of a random orthonormal V (200, m) and W = G V, G the Gaussian Gram of 200 points in 3-D
    with ell = 0.5 (float64, formed on the host): cond(S) = 3.4e3 at m = 80, so that 1e-10 on T^T S T is a statement
    about the kernel and not about the data (numpy's own Cholesky gives 1.5e-14 there)."""
    xs = torch.randn(200, 3, generator=torch.Generator().manual_seed(11)).float()
    G = N.gram(xs, N.GAUSSIAN, 0.5)
    V, _ = np.linalg.qr(np.random.default_rng(5 + m).standard_normal((200, m)))
    if store32:
        V = V.astype(np.float32).astype(np.float64)
    W = G @ V
    return V, W, W.T @ W, V.T @ W


def _run_ritz(S, A, C=None):
    from neural_svd_amd import hip_ops as H
    def dev(a):
        return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    theta, resid, Q, T = H.ritz_step_f64(dev(S), dev(A), status, C=dev(C))
    return theta.cpu().numpy(), resid.cpu().numpy(), Q.cpu().numpy(), T.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("m", (1, 2, 13, 16, 17, 33, 64, 80))
def test_ritz_step_against_numpy(m):
    """theta to 1e-12 of theta_0; |Q^T Q - I| and |T^T S T - I| <= 1e-10; resid to 1e-9 of theta_0. m = 16 is the
    last width whose m^2 elements take one pass of the 256 threads, 17 the first that takes two; 17 and 33 are odd (a
    bye in every round of the tournament).
    Measured (theta / Q^T Q / T^T S T / resid; status 0 everywhere):
        m = 2    1.6e-16 / 2.2e-16 / 1.9e-16 / 6.3e-16
        m = 13   3.5e-15 / 4.0e-15 / 5.6e-16 / 1.2e-15
        m = 16   2.3e-15 / 3.6e-15 / 6.7e-16 / 1.1e-15
        m = 17   2.0e-15 / 2.9e-15 / 1.0e-15 / 7.4e-16
        m = 33   5.1e-15 / 7.8e-15 / 3.1e-15 / 1.6e-15
        m = 64   1.4e-14 / 1.5e-14 / 7.9e-15 / 7.7e-15
        m = 80   1.5e-14 / 1.9e-14 / 2.3e-14 / 8.7e-15"""
    V, W, S, A = _ritz_inputs(m)
    theta, resid, Q, T, status = _run_ritz(S, A)
    want = np.linalg.eigvalsh(0.5 * (A + A.T))[::-1]
    I = np.eye(m)
    e_th = np.abs(theta - want).max() / want[0]
    e_q, e_t = np.abs(Q.T @ Q - I).max(), np.abs(T.T @ S @ T - I).max()
    direct = np.linalg.norm(W @ Q - (V @ Q) * theta, axis=0)  # |G v - theta v| of the Ritz pairs, as numpy has it
    e_r = np.abs(resid - direct).max() / want[0]
    e_a = np.abs(0.5 * (A + A.T) @ Q - Q * theta).max() / want[0]
    print(f"ritz m={m}: theta {e_th:.1e} QtQ {e_q:.1e} TtST {e_t:.1e} resid {e_r:.1e} AQ-Qtheta {e_a:.1e}")
    assert status == 0
    assert np.all(np.diff(theta) <= 0)
    assert e_th <= 1e-12 and e_q <= 1e-10 and e_t <= 1e-10 and e_r <= 1e-9 and e_a <= 1e-10
    # W T spans W with the Ritz directions leading: T = Q R^-1 with R upper triangular
    Rinv = Q.T @ T
    assert np.abs(np.tril(Rinv, -1)).max() <= 1e-10 * np.abs(Rinv).max()


def test_ritz_step_with_the_gram_of_a_float32_basis():
    """C = V^T V of a V rounded to float32: the residuals are |W q - theta V q| of THAT basis (1e-9 of theta_0); without
    C they would sit on a floor of theta sqrt(|q^T (C - I) q|)"""
    m = 13
    V, W, S, A = _ritz_inputs(m, store32=True)
    theta, resid, Q, T, status = _run_ritz(S, A, V.T @ V)
    direct = np.linalg.norm(W @ Q - (V @ Q) * theta, axis=0)
    assert status == 0 and np.abs(resid - direct).max() <= 1e-9 * theta[0]


def test_ritz_step_degenerate_null_and_singular():
    m = 13
    I = np.eye(m)
    theta, resid, Q, T, status = _run_ritz(I, I)          # every eigenvalue 1: finishes at once, ties by index
    assert status == 0 and np.array_equal(theta, np.ones(m)) and np.array_equal(Q, I) and np.array_equal(T, I)
    assert np.array_equal(resid, np.zeros(m))
    _, _, S, A = _ritz_inputs(m)
    theta, resid, Q, T, status = _run_ritz(S, None)        # A == NULL: orthonormalisation only
    assert status == 0 and np.array_equal(Q, I) and np.array_equal(theta, np.zeros(m))
    assert np.abs(np.tril(T, -1)).max() == 0.0 and np.abs(T.T @ S @ T - I).max() <= 1e-10
    theta, resid, Q, T, status = _run_ritz(np.zeros((m, m)), A)   # S = 0: an error return, not a fault
    from neural_svd_amd import hip_ops as H
    assert status & H.RITZ_BAD_PIVOT
    for a in (theta, resid, Q, T):
        assert np.isfinite(a).all()
    assert np.array_equal(T, np.zeros((m, m)))
    # a rank-deficient S: the columns before the bad pivot are kept, the rest are zero
    S2 = S.copy()
    S2[:, 7:] = 0.0
    S2[7:, :] = 0.0
    _, _, _, T2, status2 = _run_ritz(S2, None)
    assert status2 & H.RITZ_BAD_PIVOT and np.isfinite(T2).all() and np.array_equal(T2[:, 7:], np.zeros((m, m - 7)))
    assert np.abs(T2[:7, :7].T @ S[:7, :7] @ T2[:7, :7] - np.eye(7)).max() <= 1e-10


# ---- nsvd_ts_rotate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_ts_rotate_against_float64(n, m):
    """out = X T[:, :k], k in {1, m}, against float64, rel <= 2e-7 (one rounding to float32: 6e-8). Measured: worst 5.4e-8."""
    from neural_svd_amd import hip_ops as H
    X = _block(n, m, 4, ld=m + 5)
    T = torch.randn(m, m, generator=torch.Generator().manual_seed(m), dtype=torch.float64).to(DEV)
    for k in sorted({1, m}):
        got = H.ts_rotate(X, T, k)
        e = _rel(got, X.double() @ T[:, :k])
        print(f"ts_rotate n={n} m={m} k={k}: rel {e:.1e}")
        assert tuple(got.shape) == (n, k) and got.dtype == torch.float32
        assert e <= 2e-7
    with pytest.raises(H.NsvdError, match="alias"):
        H.ts_rotate(X, T, m, out=X)


# ---- the solver, matrix-free ------------------------------------------------------------------------------------------
def _kernel32(kind, ell):
    """the float32 torch composition of the kernel matrix (direct differences): the reference's op sequence"""
    def k(a, b):
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        return torch.exp(-d2 / (2.0 * ell ** 2)) if kind == N.GAUSSIAN else torch.exp(-d2.sqrt() / ell)
    return k


def _align(U, Uref):
    return U * np.sign(np.sum(U * Uref, axis=0))


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_solver_matrix_free(case):
    """tol = 1e-5, check_every = 1, against the float64 definition. Measured on an MI355X - iterations (recurrence (b)),
    worst true residual / lambda_0, eigenvalue error / lambda_0, |U^T U - I| (yardstick), worst eigenvector column
    err (yardstick; Davis-Kahan term), worst projection column rel (yardstick):

        n200-D1-L6    2 (2)   9.6e-8  6.5e-8  2.3e-8 (1.1e-8)  3.3e-6 (1.8e-7; 3.4e-5)  1.3e-5 (9.4e-6)
        n64-D3-L5     7 (7)   2.4e-6  3.2e-8  1.3e-8 (2.2e-8)  2.3e-8 (8.4e-9; 1.9e-7)  2.4e-7 (1.4e-7)
        n65-D3-L5     7 (6)   1.6e-6  4.2e-8  1.6e-8 (9.9e-9)  1.6e-8 (8.2e-9; 2.0e-7)  2.7e-7 (2.2e-7)
        n1030-D3-L5   7 (7)   3.4e-6  7.5e-8  5.7e-9 (5.4e-9)  1.1e-8 (1.9e-9; 2.9e-7)  1.4e-7 (3.4e-7)
        n200-D64-L5  27 (27)  8.5e-6  2.2e-8  7.0e-9 (1.6e-8)  1.5e-8 (3.9e-9; 1.7e-7)  6.9e-7 (3.6e-7)
        n200-D3-L1    5 (5)   1.1e-6  1.9e-8  1.5e-9 (5.8e-10) 2.4e-7 (4.0e-9; 2.7e-6)  1.7e-7 (2.2e-7)
        n200-D3-L56   3 (3)   3.8e-6  7.6e-7  4.2e-8 (3.3e-8)  1.7e-8 (4.2e-9; 1.9e-7)  1.4e-6 (6.4e-7)
        n200-D3-L64   3 (3)   3.7e-6  6.0e-7  3.2e-8 (1.8e-8)  1.9e-8 (4.1e-9; 2.2e-7)  9.3e-6 (5.0e-6)
        n10-D2-L4     1 (1)   4.4e-8  5.1e-9  5.6e-8 (1.5e-8)  8.1e-8 (4.5e-8; 3.7e-7)  2.1e-7 (1.5e-7)
        n333-D3-L10  10 (9)   6.1e-6  3.3e-8  1.1e-8 (6.6e-9)  1.8e-8 (3.8e-9; 2.2e-7)  4.1e-7 (3.4e-7)
        n200-D2-L6s   4 (4)   9.5e-7  6.1e-8  6.4e-9 (4.2e-9)  1.7e-8 (3.7e-9; 2.8e-7)  2.4e-7 (1.9e-7)

    (the eigenvector and projection columns name the column closest to its bound, not the largest error; the solver's
    own residual claim agreed with the recomputed one to two digits at every case; every column of every case had a
    relative gap >= 0.005 and was checked)"""
    from neural_svd_amd import Nystrom
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    n, D, L, kind, ell, shift = case
    xs, xnew = N.case_points(case)
    s = N.solved(case)
    G, w, Ustar, rec = s["G"], s["w"], s["U"][:, :L], s["rec"]
    assert N.eigen_gaps(w, L).min() >= N.MIN_GAP
    xd = xs.to(DEV)
    op = RadialKernelOperator(kind, ell, D, device=DEV)
    ny = Nystrom(op, xd, L, tol=TOL, check_every=1)
    theta = ny.eigvals.double().cpu().numpy()
    U = ny.eigvecs.double().cpu().numpy()
    assert ny.eigvals.dtype == torch.float32 and tuple(ny.eigvals.shape) == (L,) and tuple(ny.eigvecs.shape) == (n, L)
    assert ny.eigvals.device == xd.device and ny.training_time > 0
    # the reference's op sequence on the same GPU: float32 Gram by torch ops, float32 eigh on the host
    k32 = _kernel32(kind, ell)
    w32, U32 = np.linalg.eigh(k32(xd, xd).cpu().numpy())
    U32 = U32[:, ::-1][:, :L].astype(np.float64)
    I = np.eye(L)
    # residuals recomputed here in float64 from the returned pairs and the exact Gram
    r = np.linalg.norm(G @ U - U * theta, axis=0)
    orth, orth_y = np.abs(U.T @ U - I).max(), np.abs(U32.T @ U32 - I).max()
    print(f"{N.case_id(case)}: iterations {ny.iterations} (recurrence {rec['iterations']}), worst r / theta_0 "
          f"{r.max() / w[0]:.1e} (claimed {float(ny.residuals.max()):.1e}), eigenvalues "
          f"{np.abs(np.sort(theta)[::-1] - w[:L]).max() / w[0]:.1e}, UtU {orth:.1e} yardstick {orth_y:.1e}")
    assert ny.converged and len(ny.residuals) == L
    assert ny.iterations <= 2 * rec["iterations"]
    assert r.max() <= 2 * TOL * w[0]
    assert np.abs(np.sort(theta)[::-1] - w[:L]).max() <= 2 * TOL * w[0]
    assert orth <= max(2e-6, 4 * orth_y)
    # eigenvectors of the columns with a relative gap >= 0.005, up to sign: float32 (4 x yardstick) or Davis-Kahan
    assert n > L
    gap = np.minimum(w[:L] - w[1:L + 1], np.append(np.inf, w[:L - 1] - w[1:L]))  # to the nearer neighbour, absolute
    Ua, Uy = _align(U, Ustar), _align(U32, Ustar)
    err, yard = np.abs(Ua - Ustar).max(axis=0), np.abs(Uy - Ustar).max(axis=0)
    checked = 0
    for k in range(L):
        if gap[k] / w[k] >= 0.005:
            bound = max(4 * yard[k], 2 * r[k] / gap[k])
            assert err[k] <= bound, (k, err[k], yard[k], r[k], gap[k])
            checked += 1
    worst = int(np.argmax(err / np.maximum(4 * yard, 2 * r / gap)))
    print(f"    eigenvectors: {checked} of {L} columns checked; column {worst}: err {err[worst]:.1e} yardstick "
          f"{yard[worst]:.1e} Davis-Kahan {2 * r[worst] / gap[worst]:.1e}")
    assert checked >= 1
    # Nystrom(xnew) against the definition's formula evaluated with the object's OWN eigenpairs
    xn = xnew.to(DEV)
    got = ny(xn).double().cpu().numpy()
    want = N.project(xnew, xs, kind, ell, theta, U)
    ref32 = (k32(xn, xd) @ ny.eigvecs / ny.eigvals / np.sqrt(n)).double().cpu().numpy()
    cmax = np.abs(want).max(axis=0)
    e, ey = np.abs(got - want).max(axis=0) / cmax, np.abs(ref32 - want).max(axis=0) / cmax
    worst = int(np.argmax(e / np.maximum(2e-6, 4 * ey)))
    print(f"    projection: worst column {worst}: rel {e[worst]:.1e} yardstick {ey[worst]:.1e}")
    assert got.shape == (40, L) and np.isfinite(got).all()
    assert np.all(e <= np.maximum(2e-6, 4 * ey)), (e, ey)


# ---- further cases ----------------------------------------------------------------------------------------------------
SHIFTED = N.CASES[-1]
EXPONENTIAL = N.CASES[-2]


def test_emp_kernel_path_against_matrix_free():
    from neural_svd_amd import Nystrom
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    n, D, L, kind, ell, _ = SHIFTED
    xs, xnew = N.case_points((n, D, L, kind, ell, 0.0))
    xd = xs.to(DEV)
    free = Nystrom(RadialKernelOperator(kind, ell, D, device=DEV), xd, L, tol=TOL, check_every=1)
    k32 = _kernel32(kind, ell)
    dense = Nystrom(k32, xd, L, tol=TOL, check_every=1)
    given = Nystrom(None, xd, L, emp_kernel=k32(xd, xd), tol=TOL, check_every=1)
    lam0 = float(free.eigvals[0])
    d = float((free.eigvals - dense.eigvals).abs().max())
    print(f"emp_kernel path against matrix-free: eigenvalues {d / lam0:.1e} of the largest")
    assert dense.converged and given.converged and d <= 2 * TOL * lam0
    assert torch.equal(dense.eigvals, given.eigvals) and torch.equal(dense.eigvecs, given.eigvecs)
    assert tuple(dense(xnew.to(DEV)).shape) == (40, L)


def test_same_seed_same_bits():
    from neural_svd_amd import Nystrom
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    n, D, L, kind, ell, _ = EXPONENTIAL
    xd = N.case_points(EXPONENTIAL)[0].to(DEV)
    op = RadialKernelOperator(kind, ell, D, device=DEV)
    a, b = Nystrom(op, xd, L, seed=3), Nystrom(op, xd, L, seed=3)
    assert torch.equal(a.eigvals, b.eigvals) and torch.equal(a.eigvecs, b.eigvecs) and a.iterations == b.iterations
    assert a.iterations % 4 == 0  # (the default check_every)


def test_not_converged_is_reported():
    from neural_svd_amd import Nystrom
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    n, D, L, kind, ell, _ = EXPONENTIAL
    xd = N.case_points(EXPONENTIAL)[0].to(DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ny = Nystrom(RadialKernelOperator(kind, ell, D, device=DEV), xd, L, tol=TOL, max_iters=2)
    assert len(caught) == 1 and "not converged" in str(caught[0].message)
    assert f"{float(ny.residuals.max()):.3e}" in str(caught[0].message)  # names the worst residual
    assert ny.converged is False and ny.iterations == 2
    assert bool(torch.isfinite(ny.residuals).all()) and float(ny.residuals.max()) > TOL
    assert bool(torch.isfinite(ny.eigvecs).all()) and bool(torch.isfinite(ny.eigvals).all())


def test_refusals():
    from neural_svd_amd import Nystrom
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    op = RadialKernelOperator(N.GAUSSIAN, 1.5, 2, device=DEV)
    xs = torch.randn(100, 2, generator=torch.Generator().manual_seed(0))
    with pytest.raises(NsvdError, match="GPU"):
        Nystrom(op, xs, 4)
    with pytest.raises(NsvdError, match="dim"):
        Nystrom(op, xs.to(DEV), 65)
    with pytest.raises(NsvdError, match="exceeds the number of points"):
        Nystrom(op, xs[:3].to(DEV), 4)
    with pytest.raises(NsvdError):
        Nystrom(op, torch.zeros(100, 3, device=DEV), 4)   # not the operator's input dimension
    with pytest.raises(NsvdError, match="block limit"):
        Nystrom(op, xs.to(DEV), 64, oversample=17)


def test_run_nystrom_writes_the_references_keys(tmp_path):
    from neural_svd_amd import Nystrom, run_nystrom
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    n, D, L, kind, ell, _ = SHIFTED
    xs, xnew = N.case_points(SHIFTED)
    op = RadialKernelOperator(kind, ell, D, device=DEV)
    eigvals, eigfuncs, t = run_nystrom(op, L, xs.to(DEV), xnew.to(DEV), str(tmp_path))
    z = np.load(os.path.join(str(tmp_path), "eigvals.npz"))
    assert sorted(z.files) == ["eigfuncs", "eigvals"]
    assert z["eigvals"].shape == (L,) and z["eigfuncs"].shape == (40, L) and z["eigvals"].dtype == np.float32
    assert np.array_equal(z["eigvals"], eigvals) and np.array_equal(z["eigfuncs"], eigfuncs) and t > 0
    ev, evec, _ = Nystrom.evd(xs.to(DEV), op, L)
    assert isinstance(ev, np.ndarray) and ev.shape == (L,) and evec.shape == (n, L)
    assert np.array_equal(ev, eigvals)
