"""GPU tests of the truncated-SVD baseline of the kernel SVD operators: the two kernels of csrc/nystrom_svd.hip alone
(nsvd_tsgram3_f64, nsvd_svd_ritz_step_f64) against float64, and neural_svd_amd.NystromSVD against the float64 definition
and the recurrence of tests/_ksvd_oracle.py.

Bounds of the solver tests follow the repository's convention max(floor, 4 x yardstick): the yardstick is the same
quantity from a float32 cross Gram by torch ops on the same GPU, copied to the host, with float32 np.linalg.svd, against
the same float64 oracle. Both are printed by every test.

Measured on an MI355X: the tables in the docstrings of the tests (the whole file: 58 tests in 6.9 s).
"""
import math
import warnings

import numpy as np
import pytest
import torch

from tests import _ksvd_oracle as K

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


# ---- nsvd_tsgram3_f64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", GRAM_SHAPES)
def test_tsgram3_against_float64(n, m):
    """X^T X, X^T Y and Y^T Y against float64 torch on the same float32 inputs, rel <= 1e-13 (the bound
    test_tsgram_against_float64 holds the same arithmetic to); Y strided (ld = m + 7); two calls give the same bits, and
    the bits of nsvd_tsgram_f64 (the same products summed in the same order).
    Measured: worst rel 1.8e-14 (n = 8200, m = 80: the slice cap); 6.8e-15 at n = 4100, 2.9e-15 at n = 1030."""
    from neural_svd_amd import hip_ops as H
    X, Y = _block(n, m, 1), _block(n, m, 2, ld=m + 7)
    assert Y.stride(0) == m + 7
    xx, xy, yy = H.tsgram3_f64(X, Y)
    Xd, Yd = X.double(), Y.double()
    e = max(_rel(xx, Xd.T @ Xd), _rel(xy, Xd.T @ Yd), _rel(yy, Yd.T @ Yd))
    print(f"tsgram3 n={n} m={m}: rel {e:.1e}")
    for o in (xx, xy, yy):
        assert o.dtype == torch.float64 and tuple(o.shape) == (m, m)
    assert e <= 1e-13
    xx2, xy2, yy2 = H.tsgram3_f64(X, Y)
    assert torch.equal(xx, xx2) and torch.equal(xy, xy2) and torch.equal(yy, yy2)
    wxx, wxy = H.tsgram_f64(X, Y)
    assert torch.equal(xx, wxx) and torch.equal(xy, wxy) and torch.equal(yy, H.tsgram_f64(Y)[0])


def test_tsgram3_x_is_y_and_given_buffers():
    from neural_svd_amd import hip_ops as H
    n, m = 1030, 13
    Xs = _block(n, m, 3, ld=m + 3)
    xx, xy, yy = H.tsgram3_f64(Xs, Xs)
    assert torch.equal(xx, xy) and torch.equal(xx, yy)   # Y == X: the three products are the same sums
    assert torch.equal(xx, xx.T)                          # bitwise symmetric
    assert _rel(xx, Xs.double().T @ Xs.double()) <= 1e-13
    ws = H.tsgram3_workspace(n, m, DEV)
    assert ws.numel() == K.tsgram3_workspace_bytes(n, m)
    outs = [torch.empty((m, m), dtype=torch.float64, device=DEV) for _ in range(3)]
    got = H.tsgram3_f64(Xs.contiguous(), Xs, ws=ws, out_xtx=outs[0], out_xty=outs[1], out_yty=outs[2])
    assert all(g is o for g, o in zip(got, outs)) and all(torch.equal(o, xx) for o in outs)


def test_tsgram3_refusals():
    from neural_svd_amd import _lib
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    n, m = 65, 13
    X, Y = _block(n, m, 1), _block(n, m, 2)
    lib = _lib.load()
    out = [torch.full((m, m), 7.0, dtype=torch.float64, device=DEV) for _ in range(3)]
    ws = H.tsgram3_workspace(n, m, DEV)
    big = torch.empty(ws.numel() + 256, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(xtx, xty, yty, w, nbytes, mm=m, ld=m):
        return lib.nsvd_tsgram3_f64(X.data_ptr(), ld, Y.data_ptr(), ld, n, mm, xtx, xty, yty, w, nbytes, st)
    p = [o.data_ptr() for o in out]
    assert call(p[0], p[1], None, ws.data_ptr(), ws.numel()) == _lib.EINVAL          # a NULL output
    assert call(None, p[1], p[2], ws.data_ptr(), ws.numel()) == _lib.EINVAL
    assert call(p[0], p[1], p[2], ws.data_ptr(), ws.numel() - 1) == _lib.EINVAL      # short workspace
    assert call(p[0], p[1], p[2], big.data_ptr() + 8, ws.numel()) == _lib.EINVAL     # misaligned workspace
    assert call(p[0], p[1], p[2], big.data_ptr(), big.numel(), mm=81, ld=81) == _lib.EUNSUPPORTED
    assert lib.nsvd_tsgram3_f64_workspace_bytes(n, 81) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in out)                                       # a refused call writes nothing
    with pytest.raises(NsvdError):
        H.tsgram3_f64(X, Y[:, :5])
    with pytest.raises(NsvdError):
        H.tsgram3_f64(X.cpu(), Y.cpu())


# ---- nsvd_svd_ritz_step_f64 -------------------------------------------------------------------------------------------
def _state(m):
    """A real iteration state in float64 on the host: C the Gaussian cross Gram of 200 x 150 points in 3-D with ell = 0.5
    (both samples N(0, I): cond(P^T P) = 2e4 at m = 80, so that 1e-10 on T^T S T is a statement about the kernel and not
    about the data), random orthonormal U, V ROUNDED to float32 (Cu, Cv are not the identity) and P = C V, R = C^T U
    rounded to float32 (Hl != Hr)."""
    xs = torch.randn(200, 3, generator=torch.Generator().manual_seed(11)).float()
    ys = torch.randn(150, 3, generator=torch.Generator().manual_seed(12)).float()
    C = K.P.R.radial_kernel_matrix(xs, ys, K.P.GAUSSIAN, 0.5).numpy() / math.sqrt(200 * 150)
    rng = np.random.default_rng(5 + m)

    def r32(a):
        return a.astype(np.float32).astype(np.float64)
    U, V = r32(np.linalg.qr(rng.standard_normal((200, m)))[0]), r32(np.linalg.qr(rng.standard_normal((150, m)))[0])
    Pm, Rm = r32(C @ V), r32(C.T @ U)
    return dict(U=U, V=V, P=Pm, R=Rm, PtU=Pm.T @ U, RtV=Rm.T @ V, Sp=Pm.T @ Pm, Sr=Rm.T @ Rm, Cu=U.T @ U, Cv=V.T @ V)


def _run_step(PtU, RtV, Sp, Sr, Cu=None, Cv=None):
    from neural_svd_amd import hip_ops as H

    def dev(a):
        return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = H.svd_ritz_step_f64(dev(PtU), dev(RtV), dev(Sp), dev(Sr), status, dev(Cu), dev(Cv))
    return tuple(o.cpu().numpy() for o in out) + (int(status.item()),)


@pytest.mark.parametrize("m", (1, 2, 13, 64, 80))
def test_svd_ritz_step_against_numpy(m):
    """sigma to 1e-12 of sigma_0; |A^T A - I|, |B^T B - I|, |Tu^T Sp Tu - I|, |Tv^T Sr Tv - I| <= 1e-10;
    |A diag(sigma) B^T - H| <= 1e-10 sigma_0; both residuals to 1e-9 of sigma_0 of the direct norms; B^T Tu and A^T Tv
    upper triangular to 1e-10 (the bounds of test_ritz_step_against_numpy for the same class of arithmetic).
    Measured (sigma / A^T A / B^T B / A sigma B^T - H / Tu^T Sp Tu / Tv^T Sr Tv / resid_l / resid_r; status 0 everywhere;
    the residuals of this unconverged state are of order sigma_0):
        m = 1    0       / 0       / 0       / 0       / 0       / 0       / 0       / 2.5e-15
        m = 2    1.1e-17 / 9.5e-17 / 1.2e-17 / 8.8e-17 / 1.1e-16 / 2.2e-16 / 1.4e-15 / 2.1e-15
        m = 13   1.1e-15 / 8.4e-16 / 4.0e-15 / 7.8e-16 / 5.7e-16 / 5.8e-16 / 9.4e-16 / 6.3e-16
        m = 64   1.3e-14 / 9.8e-16 / 2.5e-14 / 3.1e-15 / 4.7e-14 / 5.0e-14 / 9.5e-16 / 5.6e-16
        m = 80   1.2e-14 / 1.0e-15 / 3.0e-14 / 2.9e-15 / 8.4e-14 / 1.7e-13 / 9.6e-16 / 1.2e-15"""
    s = _state(m)
    sigma, rl, rr, A, B, Tu, Tv, status = _run_step(s["PtU"], s["RtV"], s["Sp"], s["Sr"], s["Cu"], s["Cv"])
    Hm = 0.5 * (s["PtU"].T + s["RtV"])
    want = np.linalg.svd(Hm, compute_uv=False)
    I = np.eye(m)
    e_s = np.abs(sigma - want).max() / want[0]
    e_a, e_b = np.abs(A.T @ A - I).max(), np.abs(B.T @ B - I).max()
    e_h = np.abs((A * sigma) @ B.T - Hm).max() / want[0]
    e_tu, e_tv = np.abs(Tu.T @ s["Sp"] @ Tu - I).max(), np.abs(Tv.T @ s["Sr"] @ Tv - I).max()
    dl = np.linalg.norm(s["P"] @ B - (s["U"] @ A) * sigma, axis=0)
    dr = np.linalg.norm(s["R"] @ A - (s["V"] @ B) * sigma, axis=0)
    e_rl, e_rr = np.abs(rl - dl).max() / want[0], np.abs(rr - dr).max() / want[0]
    print(f"svd ritz m={m}: sigma {e_s:.1e} AtA {e_a:.1e} BtB {e_b:.1e} H {e_h:.1e} TuSpTu {e_tu:.1e} TvSrTv {e_tv:.1e} "
          f"resid_l {e_rl:.1e} resid_r {e_rr:.1e} (residuals up to {max(dl.max(), dr.max()) / want[0]:.1e})")
    assert status == 0
    assert np.all(np.diff(sigma) <= 0) and np.all(sigma >= 0)
    assert e_s <= 1e-12 and e_a <= 1e-10 and e_b <= 1e-10 and e_h <= 1e-10
    assert e_tu <= 1e-10 and e_tv <= 1e-10
    assert e_rl <= 1e-9 and e_rr <= 1e-9
    Ru, Rv = B.T @ Tu, A.T @ Tv
    assert np.abs(np.tril(Ru, -1)).max() <= 1e-10 * np.abs(Ru).max()
    assert np.abs(np.tril(Rv, -1)).max() <= 1e-10 * np.abs(Rv).max()
    # the oracle's restatement of the step: the same values up to the signs of the vector pairs
    o_sigma, o_rl, o_rr = K.svd_ritz_step(s["PtU"], s["RtV"], s["Sp"], s["Sr"], s["Cu"], s["Cv"])[:3]
    assert np.abs(sigma - o_sigma).max() <= 1e-12 * want[0]
    assert np.abs(rl - o_rl).max() <= 1e-9 * want[0] and np.abs(rr - o_rr).max() <= 1e-9 * want[0]


@pytest.mark.parametrize("m", (32, 33))
def test_svd_ritz_step_at_the_workgroup_size_threshold(m):
    """m = 32 is the last width of the 256-thread instance of the kernel, m = 33 the first of the 512-thread one: the
    same checks and bounds"""
    test_svd_ritz_step_against_numpy(m)


def test_svd_ritz_step_null_grams_are_the_identity():
    m = 13
    s = _state(m)
    I = np.eye(m)
    a = _run_step(s["PtU"], s["RtV"], s["Sp"], s["Sr"])
    b = _run_step(s["PtU"], s["RtV"], s["Sp"], s["Sr"], I, I)
    assert a[-1] == 0 and b[-1] == 0
    for x, y in zip(a[:-1], b[:-1]):
        assert np.array_equal(x, y)


def test_svd_ritz_step_degenerate():
    from neural_svd_amd import hip_ops as H
    m = 13
    I, Z = np.eye(m), np.zeros((m, m))
    # H = I with unit Grams: every singular value 1, no rotation, ties by index, zero residuals
    sigma, rl, rr, A, B, Tu, Tv, status = _run_step(I, I, I, I)
    assert status == 0 and np.array_equal(sigma, np.ones(m)) and np.array_equal(A, I) and np.array_equal(B, I)
    assert np.array_equal(Tu, I) and np.array_equal(Tv, I)
    assert np.array_equal(rl, np.zeros(m)) and np.array_equal(rr, np.zeros(m))
    s = _state(m)
    # Sp = 0: an error return, not a fault
    out = _run_step(s["PtU"], s["RtV"], Z, s["Sr"], s["Cu"], s["Cv"])
    assert out[-1] & H.RITZ_BAD_PIVOT and np.array_equal(out[5], Z)
    assert all(np.isfinite(o).all() for o in out[:-1])
    assert np.abs(out[6].T @ s["Sr"] @ out[6] - I).max() <= 1e-10     # the other side is untouched by it
    # Sr rank deficient from column 7 on (H = I, so A = I and Mr = Sr): the columns before the bad pivot are kept
    Sr = s["Sr"].copy()
    Sr[:, 7:] = 0.0
    Sr[7:, :] = 0.0
    out = _run_step(I, I, s["Sp"], Sr)
    assert out[-1] & H.RITZ_BAD_PIVOT and all(np.isfinite(o).all() for o in out[:-1])
    Tv = out[6]
    assert np.array_equal(Tv[:, 7:], np.zeros((m, m - 7)))
    assert np.abs(Tv[:7, :7].T @ Sr[:7, :7] @ Tv[:7, :7] - np.eye(7)).max() <= 1e-10
    assert np.abs(out[5].T @ s["Sp"] @ out[5] - I).max() <= 1e-10
    # H = 0: sigma = 0, zero columns of A (never a division), a bad pivot of Mr
    out = _run_step(Z, Z, s["Sp"], s["Sr"], s["Cu"], s["Cv"])
    assert out[-1] & H.RITZ_BAD_PIVOT and all(np.isfinite(o).all() for o in out[:-1])
    assert np.array_equal(out[0], np.zeros(m)) and np.array_equal(out[3], Z) and np.array_equal(out[6], Z)


def test_svd_ritz_step_refusals():
    from neural_svd_amd import _lib
    lib = _lib.load()
    m = 4
    t = [torch.full((m, m), 7.0, dtype=torch.float64, device=DEV) for _ in range(6)]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = [x.data_ptr() for x in t]
    st = torch.cuda.current_stream().cuda_stream

    def call(PtU, RtV, Sp, Sr, Tu, Tv, stat, mm=m):
        return lib.nsvd_svd_ritz_step_f64(PtU, RtV, Sp, Sr, None, None, mm, None, None, None, None, None, Tu, Tv, stat, st)
    assert call(None, p[1], p[2], p[3], p[4], p[5], status.data_ptr()) == _lib.EINVAL
    assert call(p[0], p[1], p[2], p[3], None, p[5], status.data_ptr()) == _lib.EINVAL
    assert call(p[0], p[1], p[2], p[3], p[4], None, status.data_ptr()) == _lib.EINVAL
    assert call(p[0], p[1], p[2], p[3], p[4], p[5], None) == _lib.EINVAL
    assert call(p[0], p[1], p[2], p[3], p[4], p[5], status.data_ptr(), mm=0) == _lib.EINVAL
    assert call(p[0], p[1], p[2], p[3], p[4], p[5], status.data_ptr(), mm=81) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in t) and int(status.item()) == 0   # a refused call writes nothing


# ---- the solver, matrix-free ------------------------------------------------------------------------------------------
def _kernel32(kind):
    """the float32 torch composition of the kernel matrix: the library route"""
    def k(a, b):
        if kind in (K.GAUSSIAN, K.EXPONENTIAL):
            d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
            return torch.exp(-d2 / (2.0 * K.ELL ** 2)) if kind == K.GAUSSIAN else torch.exp(-d2.sqrt() / K.ELL)
        s = a @ b.T
        if kind == K.POLYNOMIAL:
            gamma, coef0, degree = K.POLY
            return (gamma * s + coef0) ** degree
        p = a.norm(dim=1)[:, None] * b.norm(dim=1)[None, :]
        c = (s / p).clamp(-1.0, 1.0)
        return p / math.pi * (torch.sqrt((1.0 - c) * (1.0 + c)) + torch.acos(-c) * c)
    return k


def _operator(kind, D):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import DotKernelOperator, RadialKernelOperator
    if kind in (K.GAUSSIAN, K.EXPONENTIAL):
        return RadialKernelOperator(H.RBF_GAUSSIAN if kind == K.GAUSSIAN else H.RBF_EXPONENTIAL, K.ELL, D, device=DEV)
    if kind == K.POLYNOMIAL:
        gamma, coef0, degree = K.POLY
        return DotKernelOperator(H.DOT_POLYNOMIAL, D, gamma=gamma, coef0=coef0, degree=degree, device=DEV)
    return DotKernelOperator(H.DOT_ARCCOS1, D, device=DEV)


def _align_pair(U, V, Uref, Vref):
    """a singular pair is defined up to a COMMON sign"""
    s = np.sign(np.sum(U * Uref, axis=0) + np.sum(V * Vref, axis=0))
    return U * s, V * s


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_solver_matrix_free(case):
    """tol = 1e-5, check_every = 1, against the float64 definition; every figure is printed with its yardstick.
    Measured on an MI355X - iterations (recurrence (b)), worst true residual / sigma_0, singular value error / sigma_0,
    orthonormality of left and right (yardstick), worst left_functions / right_functions column rel (yardsticks):

        gauss 64 x 50 D3 L5       4 (4)   4.3e-6  1.8e-8  2.7e-8 (1.7e-8)  3.8e-7 / 4.0e-7 (4.2e-7 / 2.1e-7)
        gauss 257 x 130 D3 L5     5 (5)   7.7e-6  3.7e-8  1.2e-8 (1.4e-8)  3.8e-7 / 2.8e-7 (4.0e-7 / 2.7e-7)
        exp 257 x 130 D3 L5       8 (8)   2.9e-6  2.5e-8  1.7e-8 (1.2e-8)  1.5e-7 / 3.3e-7 (1.1e-7 / 4.4e-7)
        arccos 257 x 130 D3 L5    4 (4)   9.6e-7  4.3e-8  3.0e-8 (1.4e-8)  3.0e-7 / 3.5e-7 (3.2e-7 / 2.0e-7)
        gauss 1030 x 515 D3 L5    6 (6)   1.3e-6  5.1e-8  6.3e-9 (3.7e-9)  3.1e-7 / 2.2e-7 (3.1e-7 / 3.0e-7)
        exp 130 x 257 D2 L10      8 (9)   6.2e-6  1.2e-8  1.9e-8 (1.0e-8)  6.4e-7 / 6.2e-7 (3.9e-7 / 7.0e-7)
        gauss 300 x 300 D16 L10  13 (13)  3.8e-6  1.2e-8  1.9e-8 (1.5e-8)  2.8e-7 / 3.4e-7 (1.4e-7 / 1.1e-7)
        poly 200 x 150 D3 L4     15 (14)  8.7e-6  1.4e-8  3.0e-8 (1.1e-8)  1.9e-7 / 1.5e-7 (1.1e-7 / 1.3e-7)
        gauss 10 x 7 D2 L4        2 (2)   5.4e-8  9.3e-9  2.8e-8 (6.0e-8)  1.3e-6 / 3.3e-7 (1.1e-6 / 4.8e-7)
        gauss 200 x 200 D3 L1     4 (4)   2.0e-6  6.9e-8  8.3e-9 (4.7e-9)  1.3e-7 / 1.9e-7 (4.5e-7 / 4.7e-7)
        gauss 200 x 120 D3 L56    2 (2)   1.0e-6  1.8e-7  2.6e-8 (3.1e-8)  2.8e-5 / 1.7e-5 (1.3e-5 / 6.4e-6)
        gauss 200 x 120 D3 L64    2 (2)   1.7e-7  6.8e-8  2.6e-8 (2.8e-8)  4.6e-4 / 6.0e-5 (1.8e-4 / 2.8e-5)

    (the function columns name the column closest to its bound; the solver's own residual claim agreed with the recomputed
    one to two digits at every case; every column of every case had a relative gap >= 0.005 and was checked, the worst
    vector error 4.9e-7 against a Wedin term of 4.9e-6. The last two rows' function errors are relative errors of
    columns whose singular value is 1e-5 .. 1e-6 sigma_0: the float32 product divided by it, in the yardstick alike.)"""
    from neural_svd_amd import NystromSVD
    kind, nx, ny, D, dim, over = case
    xs, ys, xnew, ynew = K.case_points(case)
    s = K.solved(case)
    C, sv, Ustar, Vstar, s_all, rec = s["C"], s["s"], s["U"], s["V"], s["s_all"], s["rec"]
    xd, yd = xs.to(DEV), ys.to(DEV)
    op = _operator(kind, D)
    sol = NystromSVD(op, xd, yd, dim, oversample=over, tol=TOL, check_every=1)
    for t, shape in ((sol.svals, (dim,)), (sol.left, (nx, dim)), (sol.right, (ny, dim))):
        assert t.dtype == torch.float32 and tuple(t.shape) == shape and t.device == xd.device
    assert tuple(sol.residuals.shape) == (dim,) and sol.training_time > 0 and isinstance(sol.iterations, int)
    sg = sol.svals.double().cpu().numpy()
    U, V = sol.left.double().cpu().numpy(), sol.right.double().cpu().numpy()
    # the library route on the same GPU: float32 cross Gram by torch ops, float32 svd on the host
    k32 = _kernel32(kind)
    U32, s32, Vt32 = np.linalg.svd(k32(xd, yd).cpu().numpy() / np.float32(math.sqrt(nx * ny)), full_matrices=False)
    U32, V32 = U32[:, :dim].astype(np.float64), Vt32[:dim].T.astype(np.float64)
    I = np.eye(dim)
    # residuals recomputed here in float64 from the returned triplets and the exact C
    rl, rr = np.linalg.norm(C @ V - U * sg, axis=0), np.linalg.norm(C.T @ U - V * sg, axis=0)
    r = np.maximum(rl, rr)
    orth = max(np.abs(U.T @ U - I).max(), np.abs(V.T @ V - I).max())
    orth_y = max(np.abs(U32.T @ U32 - I).max(), np.abs(V32.T @ V32 - I).max())
    e_s = np.abs(sg - sv).max() / sv[0]
    print(f"{K.case_id(case)}: iterations {sol.iterations} (recurrence {rec['iterations']}), worst r / sigma_0 "
          f"{r.max() / sv[0]:.1e} (claimed {float(sol.residuals.max()):.1e}), singular values {e_s:.1e} "
          f"(yardstick {np.abs(s32[:dim] - sv).max() / sv[0]:.1e}), orthonormality {orth:.1e} yardstick {orth_y:.1e}")
    assert sol.converged
    assert sol.iterations <= 2 * rec["iterations"]
    assert r.max() <= 2 * TOL * sv[0]
    assert e_s <= 2 * TOL
    assert orth <= max(2e-6, 4 * orth_y)
    # singular vectors of the columns with a relative gap >= 0.005, up to a common sign of the pair: float32
    # (4 x yardstick) or Wedin's bound
    rgap = K.relative_gaps(s_all, dim)
    gap = rgap * sv
    Ua, Va = _align_pair(U, V, Ustar, Vstar)
    Uy, Vy = _align_pair(U32, V32, Ustar, Vstar)
    err = np.maximum(np.abs(Ua - Ustar).max(axis=0), np.abs(Va - Vstar).max(axis=0))
    yard = np.maximum(np.abs(Uy - Ustar).max(axis=0), np.abs(Vy - Vstar).max(axis=0))
    bound = np.maximum(4 * yard, 2 * r / np.maximum(gap, 1e-300))
    checked = 0
    for k in range(dim):
        if rgap[k] >= K.MIN_GAP:
            assert err[k] <= bound[k], (k, err[k], yard[k], r[k], gap[k])
            checked += 1
    worst = int(np.argmax(np.where(rgap >= K.MIN_GAP, err / bound, 0.0)))
    print(f"    vectors: {checked} of {dim} columns checked; column {worst}: err {err[worst]:.1e} yardstick "
          f"{yard[worst]:.1e} Wedin {2 * r[worst] / gap[worst]:.1e}")
    assert 2 * checked >= dim
    # the singular functions on fresh points against the definition's formula with the object's OWN triplets
    xn, yn = xnew.to(DEV), ynew.to(DEV)
    for name, got, want, ref32 in (
            ("left", sol.left_functions(xn), K.left_functions(kind, xnew, ys, sg, V),
             k32(xn, yd) @ sol.right / sol.svals / math.sqrt(ny)),
            ("right", sol.right_functions(yn), K.right_functions(kind, ynew, xs, sg, U),
             k32(yn, xd) @ sol.left / sol.svals / math.sqrt(nx))):
        got, ref32 = got.double().cpu().numpy(), ref32.double().cpu().numpy()
        cmax = np.abs(want).max(axis=0)
        e, ey = np.abs(got - want).max(axis=0) / cmax, np.abs(ref32 - want).max(axis=0) / cmax
        worst = int(np.argmax(e / np.maximum(2e-6, 4 * ey)))
        print(f"    {name}_functions: worst column {worst}: rel {e[worst]:.1e} yardstick {ey[worst]:.1e}")
        assert got.shape == (40, dim) and np.isfinite(got).all()
        assert np.all(e <= np.maximum(2e-6, 4 * ey)), (name, e, ey)


# ---- further cases ----------------------------------------------------------------------------------------------------
RADIAL = K.CASES[2]    # exponential 257 x 130
DOT = K.CASES[3]       # arc-cosine 257 x 130


def test_singular_functions_on_the_sample():
    """on the sample itself the functions are sqrt(n) x the stored vectors, up to the residual: |.| <= 2 tol sigma_0 /
    sigma_k a column (C v_k / sigma_k - u_k = resid_l_k / sigma_k)"""
    from neural_svd_amd import NystromSVD
    kind, nx, ny, D, dim, over = RADIAL
    xs, ys, _, _ = K.case_points(RADIAL)
    xd, yd = xs.to(DEV), ys.to(DEV)
    sol = NystromSVD(_operator(kind, D), xd, yd, dim, tol=TOL, check_every=1)
    ratio = float(sol.svals[0]) / sol.svals.double().cpu().numpy()
    dl = (sol.left_functions(xd) / math.sqrt(nx) - sol.left).double().norm(dim=0).cpu().numpy()
    dr = (sol.right_functions(yd) / math.sqrt(ny) - sol.right).double().norm(dim=0).cpu().numpy()
    print(f"functions on the sample: left {dl.max():.1e} right {dr.max():.1e}")
    # (2e-6 sigma_0: the float32 product that evaluates them, the floor of the other function checks)
    assert np.all(dl <= (2 * TOL + 2e-6) * ratio) and np.all(dr <= (2 * TOL + 2e-6) * ratio)


def test_emp_kernel_and_callable_routes_against_matrix_free():
    from neural_svd_amd import NystromSVD
    kind, nx, ny, D, dim, over = RADIAL
    xs, ys, xnew, _ = K.case_points(RADIAL)
    xd, yd = xs.to(DEV), ys.to(DEV)
    free = NystromSVD(_operator(kind, D), xd, yd, dim, tol=TOL, check_every=1)
    k32 = _kernel32(kind)
    dense = NystromSVD(k32, xd, yd, dim, tol=TOL, check_every=1)
    given = NystromSVD(None, xd, yd, dim, emp_kernel=k32(xd, yd), tol=TOL, check_every=1)
    s0 = float(free.svals[0])
    d = float((free.svals - dense.svals).abs().max())
    print(f"emp_kernel route against matrix-free: singular values {d / s0:.1e} of the largest")
    assert dense.converged and given.converged and d <= 2 * TOL * s0
    assert torch.equal(dense.svals, given.svals) and torch.equal(dense.left, given.left)
    assert torch.equal(dense.right, given.right)
    assert tuple(dense.left_functions(xnew.to(DEV)).shape) == (40, dim)


@pytest.mark.parametrize("case", (RADIAL, DOT), ids=K.case_id)
def test_two_call_operator_against_the_fused_pair(case):
    """the base class's two-sided product (two apply_raw calls with swapped arguments) in place of the one-call pair"""
    from neural_svd_amd import NystromSVD
    from neural_svd_amd.kernel_ops import MatrixFreeKernelOperator
    kind, nx, ny, D, dim, over = case
    xs, ys, _, _ = K.case_points(case)
    xd, yd = xs.to(DEV), ys.to(DEV)
    op = _operator(kind, D)
    two = type("TwoCall" + type(op).__name__, (type(op),),
               dict(workspace_pair=MatrixFreeKernelOperator.workspace_pair,
                    apply_pair_raw=MatrixFreeKernelOperator.apply_pair_raw))
    op2 = _operator(kind, D)
    op2.__class__ = two
    a = NystromSVD(op, xd, yd, dim, tol=TOL, check_every=1)
    b = NystromSVD(op2, xd, yd, dim, tol=TOL, check_every=1)
    s0 = float(a.svals[0])
    d = float((a.svals - b.svals).abs().max())
    print(f"two-call operator against the fused pair ({kind}): singular values {d / s0:.1e} of the largest")
    assert a.converged and b.converged and d <= 2 * TOL * s0


def test_symmetric_case_against_nystrom():
    """xs == ys, Gaussian: C = k(xs, xs) / n is PSD and symmetric, its singular values are Nystrom's eigenvalues"""
    from neural_svd_amd import Nystrom, NystromSVD
    case = K.CASES[1]
    kind, nx, ny, D, dim, over = case
    xd = K.case_points(case)[0].to(DEV)
    op = _operator(kind, D)
    sv = NystromSVD(op, xd, xd, dim, tol=TOL, check_every=1)
    ev = Nystrom(op, xd, dim, tol=TOL, check_every=1)
    lam0 = float(ev.eigvals[0])
    d = float((sv.svals - ev.eigvals).abs().max())
    print(f"NystromSVD(xs, xs) against Nystrom: {d / lam0:.1e} of the largest")
    assert sv.converged and ev.converged and d <= 2 * TOL * lam0


def test_same_seed_same_bits():
    from neural_svd_amd import NystromSVD
    kind, nx, ny, D, dim, over = DOT
    xs, ys, _, _ = K.case_points(DOT)
    xd, yd = xs.to(DEV), ys.to(DEV)
    op = _operator(kind, D)
    a, b = NystromSVD(op, xd, yd, dim, seed=3), NystromSVD(op, xd, yd, dim, seed=3)
    assert torch.equal(a.svals, b.svals) and torch.equal(a.left, b.left) and torch.equal(a.right, b.right)
    assert a.iterations == b.iterations and a.iterations % 4 == 0  # (the default check_every)


def test_not_converged_is_reported():
    from neural_svd_amd import NystromSVD
    kind, nx, ny, D, dim, over = K.SLOWEST
    xs, ys, _, _ = K.case_points(K.SLOWEST)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sol = NystromSVD(_operator(kind, D), xs.to(DEV), ys.to(DEV), dim, tol=TOL, max_iters=2)
    assert len(caught) == 1 and "not converged" in str(caught[0].message)
    assert issubclass(caught[0].category, RuntimeWarning)
    assert f"{float(sol.residuals.max()):.3e}" in str(caught[0].message)  # names the worst residual
    assert sol.converged is False and sol.iterations == 2
    assert bool(torch.isfinite(sol.residuals).all()) and float(sol.residuals.max()) > TOL
    for t in (sol.svals, sol.left, sol.right):
        assert bool(torch.isfinite(t).all())


def test_refusals():
    from neural_svd_amd import NystromSVD
    from neural_svd_amd._lib import NsvdError
    op = _operator(K.GAUSSIAN, 2)
    g = torch.Generator().manual_seed(0)
    xs, ys = torch.randn(100, 2, generator=g), torch.randn(90, 2, generator=g)
    xd, yd = xs.to(DEV), ys.to(DEV)
    with pytest.raises(NsvdError, match="GPU"):
        NystromSVD(op, xs, yd, 4)
    with pytest.raises(NsvdError, match="GPU"):
        NystromSVD(op, xd, ys, 4)
    with pytest.raises(NsvdError):
        NystromSVD(op, xd[0], yd, 4)                      # wrong rank
    with pytest.raises(NsvdError, match="dim"):
        NystromSVD(op, xd, yd, 65)
    with pytest.raises(NsvdError, match="dim"):
        NystromSVD(op, xd, yd, 0)
    with pytest.raises(NsvdError, match="exceeds the number of points"):
        NystromSVD(op, xd, yd[:3], 4)
    with pytest.raises(NsvdError):
        NystromSVD(op, torch.zeros(100, 3, device=DEV), torch.zeros(90, 3, device=DEV), 4)   # not the operator's dimension
    with pytest.raises(NsvdError, match="block limit"):
        NystromSVD(op, xd, yd, 64, oversample=17)
    with pytest.raises(NsvdError):
        NystromSVD(None, xd, yd, 4, emp_kernel=torch.zeros(100, 90))                        # a CPU matrix
    sol = NystromSVD(op, xd, yd, 4)
    with pytest.raises(NsvdError, match="GPU"):
        sol.left_functions(xs)
