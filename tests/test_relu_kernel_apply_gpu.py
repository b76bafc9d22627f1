"""GPU tests of the deep ReLU kinds of the matrix-free dot-product kernel operator (nsvd_dot_apply with
NSVD_DOT_RELU_NNGP / NSVD_DOT_RELU_NTK, hip_ops.dot_apply) against their float64 restatement
(tests/_relu_kernel_oracle.py). rel = max |got - want| / max |want|; the bound is the project's own,
max(2e-6, 4 * yardstick), the yardstick being the rel of the same quantity composed in float32 from library calls on the
same GPU (x @ y.T, the recursion in torch ops, @ f: _relu_kernel_oracle.relu_kernel_matrix32) against the same oracle.
gamma and coef0 are float32 values, so that the oracle sees the inputs the kernel sees."""
import math

import numpy as np
import pytest
import torch

from tests import _dot_oracle as DO
from tests import _relu_kernel_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {"nngp": R.RELU_NNGP, "ntk": R.RELU_NTK}
BASE = (65, 200, 3, 5)  # B1, B2, D, L
DEPTH, GAMMA, COEF0 = 3, 2.0, float(np.float32(0.1))
B2_FIRST_SPLIT, B2_SPLIT = 961, 1030  # 16 and 17 chunks of 64 reference rows: two slices (asserted below)


def rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _shapes():
    b1, b2, d, l = BASE
    s = [(v, b2, d, l) for v in (1, 64, 65, 130)]
    s += [(b1, v, d, l) for v in (1, 63, 64, 65, B2_FIRST_SPLIT, B2_SPLIT)]
    s += [(b1, b2, v, l) for v in (2, 3, 8, 9, 64)]
    s += [(b1, b2, d, v) for v in (1, 64, 65, 130)]
    s += [(130, B2_SPLIT, 64, 130)]
    return sorted(set(s))


def _inputs(B1, B2, D, L):
    g = torch.Generator().manual_seed(1000 * B1 + 100 * B2 + 10 * D + L)
    x = torch.randn(B1, D, generator=g).float()
    y = torch.randn(B2, D, generator=g).float()
    f = torch.randn(B2, L, generator=g)
    return x, y, f


def _check(x, y, f, kind, gamma, coef0, depth, what):
    """got and the float32 yardstick against the oracle on the SAME float32 inputs; returns (got, rel, bound)"""
    from neural_svd_amd import hip_ops as H
    scale = 1.0 / y.shape[0]
    want = R.relu_kernel_apply(x, y, f, kind, gamma, coef0, depth, scale)
    xd, yd, fd = x.to(DEV), y.to(DEV), f.to(DEV)
    got = H.dot_apply(xd, yd, fd, kind, gamma, coef0, depth, scale)
    yard = scale * (R.relu_kernel_matrix32(xd, yd, kind, gamma, coef0, depth) @ fd)
    e, ey = rel(got, want), rel(yard, want)
    bound = max(2e-6, 4.0 * ey)
    print(f"relu dot_apply {what}: rel {e:.2e} yardstick {ey:.2e} bound {bound:.2e}")
    assert bool(torch.isfinite(got).all())
    assert e < bound, (what, e, ey, bound)
    return got, e, bound


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B1,B2,D,L", _shapes())
def test_against_float64(B1, B2, D, L, kind):
    """depth 3, (gamma, coef0) = (2, 0.1), one axis at a time around (65, 200, 3, 5) plus the corner; B2 = 961 and 1030
    take two slices of the reference rows. Measured on an MI355X over the 38 cases: worst rel 6.3e-7 (NTK, D = 2;
    yardstick 4.5e-7), the largest bound any case was given 3.8e-6; the depth / variance cases below: worst 1.1e-6 (NTK,
    depth 8, gamma 1, coef0 0; yardstick 1.0e-6)."""
    assert DO.split_slices(BASE[0], BASE[1], BASE[3]) == 1 and DO.split_slices(BASE[0], B2_SPLIT, BASE[3]) == 2
    assert DO.split_slices(BASE[0], B2_FIRST_SPLIT - 1, BASE[3]) == 1 and DO.split_slices(BASE[0], B2_FIRST_SPLIT, BASE[3]) == 2
    x, y, f = _inputs(B1, B2, D, L)
    _check(x, y, f, KINDS[kind], GAMMA, COEF0, DEPTH, f"{kind} B1={B1} B2={B2} D={D} L={L}")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("gamma,coef0", ((1.0, 0.0), (0.5, 1.0)))
@pytest.mark.parametrize("depth", (1, 2, 8))
def test_depths_and_variances(depth, gamma, coef0, kind):
    x, y, f = _inputs(*BASE)
    _check(x, y, f, KINDS[kind], gamma, coef0, depth, f"{kind} depth={depth} gamma={gamma} coef0={coef0}")


def test_depth_one_is_the_arc_cosine_kind():
    """gamma = 1, coef0 = 0, depth = 1: the NNGP kind against H.dot_apply(..., DOT_ARCCOS1, ...) within the bound"""
    from neural_svd_amd import hip_ops as H
    x, y, f = _inputs(*BASE)
    got, _, bound = _check(x, y, f, R.RELU_NNGP, 1.0, 0.0, 1, "nngp as arccos1")
    ref = H.dot_apply(x.to(DEV), y.to(DEV), f.to(DEV), H.DOT_ARCCOS1, 1.0, 1.0, 2, 1.0 / y.shape[0])
    e = rel(got, ref)
    print(f"nngp depth 1 against DOT_ARCCOS1: {e:.2e} bound {bound:.2e}")
    assert e < bound


def _c_rounding(D, depth):
    """delta: how far the float32 c of a pair whose exact c is +-1 may sit from it, in units u = 2^-24, at the deepest
    level. Level 1: x.y is a sum of D products (D u relative for a sum of same-signed terms, which |c| = 1 makes it),
    each |.|^2 likewise and p = sqrt(. .) takes half of both and of their product's rounding plus its own
    (under D u + 2 u), the quotient at most 2 u (1 ulp): under (2 D + 6) u. Every further level adds the
    rounding of S_l = gamma p A1 + coef0 (A1's slope in c is A0 <= 1, so delta goes through once; the two FMAs of q_l,
    two roots, the products: under 2 u + 6 u), again of that size or less: delta <= depth (2 D + 8) u, a few times the
    (2 D + 4) u of one level."""
    return depth * (2 * D + 8) * 2.0 ** -24


def _ntk_edge_bound(D, depth):
    """A0 = acos(-c) / pi at c = +-(1 - delta) is off by acos(1 - delta) / pi = sqrt(2 delta) / pi (1 + O(delta)).
    T_l = S_l + gamma T_{l-1} A0, and |T_{l-1}| <= max diag T_{l-1} <= max diag T_l / gamma (positive semi-definite;
    the diagonal grows by at least the factor gamma), so relative to max |T_depth| each level adds at most its own
    sqrt(2 delta) / pi, and S's own error (the usual 2e-6) on top: depth sqrt(2 delta) / pi + 2e-6."""
    return depth * math.sqrt(2.0 * _c_rounding(D, depth)) / math.pi + 2e-6


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_matrix_itself(kind):
    """x is y (the same tensor) and f = B I: the output is the kernel matrix, B = 65, D = 3, depth 3, (2, 0.1). Off the
    diagonal the usual bound against the float32 composition. NNGP diagonal: relu_kernel_diagonal to depth * 1e-6
    relative (the bracket is stationary at t = 0). NTK diagonal: c = 1 in exact arithmetic, and the rounding of c
    reaches the value through A0's slope: the bound is _ntk_edge_bound's, derived there from the rounding of c alone
    (2.1e-3 at D = 3, depth 3; one level with c = 1 - 2^-23 costs 1.6e-4 of it). Measured on an MI355X: off the
    diagonal 1.4e-7 (NNGP) / 4.5e-7 (NTK), the NNGP diagonal 2.0e-7, the NTK diagonal 2.8e-4; the NTK at D = 1 (below)
    2.4e-5 against 1.8e-3."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import relu_kernel_diagonal
    B, D = 65, 3
    x, _, _ = _inputs(B, B, D, B)
    xd = x.to(DEV)
    got = H.dot_apply(xd, xd, (float(B) * torch.eye(B)).to(DEV), KINDS[kind], GAMMA, COEF0, DEPTH, 1.0 / B).cpu().double()
    want = R.relu_kernel_matrix(x, x, KINDS[kind], GAMMA, COEF0, DEPTH)
    yard = R.relu_kernel_matrix32(xd, xd, KINDS[kind], GAMMA, COEF0, DEPTH).cpu().double()
    off = ~torch.eye(B, dtype=torch.bool)
    scale = float(want[off].abs().max())
    e, ey = float((got - want)[off].abs().max()) / scale, float((yard - want)[off].abs().max()) / scale
    print(f"{kind} kernel matrix off the diagonal: rel {e:.2e} yardstick {ey:.2e}")
    assert bool(torch.isfinite(got).all())
    assert e < max(2e-6, 4.0 * ey)
    diag = torch.from_numpy(relu_kernel_diagonal(KINDS[kind], (x.double() ** 2).sum(1).numpy(), GAMMA, COEF0, DEPTH))
    d = float(((got.diagonal() - diag).abs() / diag).max())
    bound = DEPTH * 1e-6 if kind == "nngp" else _ntk_edge_bound(D, DEPTH)
    print(f"{kind} diagonal against the closed form: {d:.2e} bound {bound:.2e}")
    assert d <= bound


def test_ntk_at_one_dimension():
    """D = 1: every pair has c = +-1, so every value carries A0's edge error; the whole matrix against float64 under
    _ntk_edge_bound (relative to the largest value)"""
    from neural_svd_amd import hip_ops as H
    B = 65
    x, _, _ = _inputs(B, B, 1, B)
    xd = x.to(DEV)
    got = H.dot_apply(xd, xd, (float(B) * torch.eye(B)).to(DEV), R.RELU_NTK, GAMMA, COEF0, DEPTH, 1.0 / B)
    e = rel(got, R.relu_kernel_matrix(x, x, R.RELU_NTK, GAMMA, COEF0, DEPTH))
    bound = _ntk_edge_bound(1, DEPTH)
    print(f"ntk at D = 1: rel {e:.2e} bound {bound:.2e}")
    assert bool(torch.isfinite(got).all())
    assert e <= bound


@pytest.mark.parametrize("kind", list(KINDS))
def test_zero_rows_and_antiparallel_pair(kind):
    """a zero row on either side (x row 0, y row 3) and an antiparallel pair (y_2 = -1.7 x_1): finite, >= 0 there, the
    oracle's values; the zero rows are coef0-only at depth 1 and exactly 0 at coef0 = 0"""
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(8, 3, generator=g), torch.randn(8, 3, generator=g)
    x[0] = 0.0
    y[3] = 0.0
    y[2] = -1.7 * x[1]
    xd, yd = x.to(DEV), y.to(DEV)
    eye = (8.0 * torch.eye(8)).to(DEV)  # with scale = 1 / 8: the kernel matrix, exactly
    for depth, gamma, coef0 in ((DEPTH, GAMMA, COEF0), (1, GAMMA, COEF0), (DEPTH, 1.0, 0.0)):
        got = H.dot_apply(xd, yd, eye, KINDS[kind], gamma, coef0, depth, 0.125).cpu()
        want = R.relu_kernel_matrix(x, y, KINDS[kind], gamma, coef0, depth)
        assert bool(torch.isfinite(got).all())
        assert float(got[0].min()) >= 0.0 and float(got[:, 3].min()) >= 0.0 and float(got[1, 2]) >= 0.0
        # the antiparallel pair has c = -1: the NTK kind's edge error there, the usual bound elsewhere
        e = float((got.double() - want).abs().max() / want.abs().max())
        ey = rel(R.relu_kernel_matrix32(xd, yd, KINDS[kind], gamma, coef0, depth), want)
        bound = max(2e-6, 4.0 * ey) if kind == "nngp" else _ntk_edge_bound(3, depth)
        print(f"{kind} edge rows depth {depth} gamma {gamma} coef0 {coef0}: rel {e:.2e} bound {bound:.2e}")
        assert e <= bound
        if depth == 1:
            assert bool((got[0] == coef0).all()) and bool((got[:, 3] == coef0).all())
        if coef0 == 0.0:
            assert bool((got[0] == 0).all()) and bool((got[:, 3] == 0).all())


@pytest.mark.parametrize("kind", list(KINDS))
def test_padded_reference_rows_are_not_seen(kind):
    """B2 = 65 leaves 63 padded (zero) reference rows in the second chunk, whose kernel values are coef0-derived, not 0.
    The workspace is filled with ones first, so that f^T's padding is the call's own; the result equals the call on
    the first 64 rows plus the 65th row's term, and the oracle."""
    from neural_svd_amd import hip_ops as H
    B1, B2, D, L = 65, 65, 3, 5
    x, y, f = _inputs(B1, B2, D, L)
    coef0 = 1.0
    _check(x, y, f, KINDS[kind], GAMMA, coef0, DEPTH, f"{kind} padded rows")
    xd, yd, fd = x.to(DEV), y.to(DEV), f.to(DEV)
    ws = H.dot_apply_workspace(B1, B2, D, L, DEV)
    ws.fill_(0x3F)
    a = H.dot_apply(xd, yd, fd, KINDS[kind], GAMMA, coef0, DEPTH, 1.0, ws=ws)
    ws.fill_(0xFF)
    b = H.dot_apply(xd, yd, fd, KINDS[kind], GAMMA, coef0, DEPTH, 1.0, ws=ws)
    assert torch.equal(a, b)
    # with f = ones a seen padded row would add its coef0-derived value (of the size of every other) to every sum
    _check(x, y, torch.ones(B2, L), KINDS[kind], GAMMA, coef0, DEPTH, f"{kind} padded rows, f = ones")


def test_two_calls_give_the_same_bits():
    from neural_svd_amd import hip_ops as H
    x, y, f = (t.to(DEV) for t in _inputs(130, B2_SPLIT, 16, 65))
    for kind in KINDS.values():
        a = H.dot_apply(x, y, f, kind, GAMMA, COEF0, DEPTH, 1.0 / B2_SPLIT)
        b = H.dot_apply(x, y, f, kind, GAMMA, COEF0, DEPTH, 1.0 / B2_SPLIT)
        assert torch.equal(a, b)
        ws = H.dot_apply_workspace(130, B2_SPLIT, 16, 65, DEV)
        out = torch.empty_like(a)
        assert H.dot_apply(x, y, f, kind, GAMMA, COEF0, DEPTH, 1.0 / B2_SPLIT, ws=ws, out=out) is out
        assert torch.equal(out, a)


def test_refusals_leave_out_untouched():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    B1, B2, D, L = BASE
    x, y, f = (t.to(DEV) for t in _inputs(B1, B2, D, L))
    out = torch.full((B1, L), 7.0, device=DEV)
    nan, inf = float("nan"), float("inf")
    for kind in KINDS.values():
        for gamma, coef0, depth in ((1.0, 0.0, 0), (1.0, 0.0, 9), (1.0, 0.0, -1), (0.0, 0.0, 3), (-1.0, 0.0, 3),
                                    (nan, 0.0, 3), (inf, 0.0, 3), (1.0, -0.5, 3), (1.0, nan, 3), (1.0, inf, 3)):
            with pytest.raises(NsvdError, match="invalid"):
                H.dot_apply(x, y, f, kind, gamma, coef0, depth, 1.0, out=out)
    with pytest.raises(NsvdError, match="invalid"):  # 2 stays unassigned
        H.dot_apply(x, y, f, 2, 1.0, 0.0, 3, 1.0, out=out)
    with pytest.raises(NsvdError, match="invalid"):
        H.dot_apply(x, y, f, 5, 1.0, 0.0, 3, 1.0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for kind in KINDS.values():
        out.fill_(7.0)
        H.dot_apply(x, y, f, kind, 1.0, 0.0, 8, 1.0, out=out)
        assert not bool((out == 7.0).any()) and bool(torch.isfinite(out).all())
