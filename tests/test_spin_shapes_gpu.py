"""SpIN's two kernels (csrc/spin.hip) at the tile, block and input branches tests/test_spin_gpu.py does not reach, against
the float64 restatement (tests/_spin_oracle.py):

  1. nsvd_spin_jac_step at every edge of its one kernel instance (SP_TM = 32 rows x SP_TN = 128 columns per tile, SP_KB =
     32 samples per chunk, blocks of at most SP_AB = 8 a's balanced by spin_carve): more than one column tile, dead and
     partly live waves, unbalanced and short blocks of a, ragged row tiles, B1 from 2 to 1024, one to eight layers. J,
     every gradient tensor and the workspace are views inside larger buffers whose margins must keep their bits, and the
     workspace is filled with NaN bit patterns before a call: its pad columns are documented as never read unmasked.
  2. nsvd_spin_solve at odd and in-between L, rank-deficient sigma, decay = 0, three distinct scales, non-finite moments
     and an accumulating status word.

Bounds (none is taken from what the code under test gives):
- nsvd_spin_jac_step, per tensor relative Frobenius error AND, per tensor, per (a, c) slice of J and per head c of the
  gradients, ||got - want||_F / ||A||_F over the slice, A = the same contraction with |phi| |delta| |a_{i-1}|
  (S.jacobian_contraction_abs; for the gradients sum_a |gsigma[a, c]| A[a, c]) - the sum of the absolute terms, which a
  rounding error of the element is relative to: test_spin_gpu's derivation (1.8e-6 per softplus layer, through at most
  three hidden layers into both operands: 1.1e-5) plus the fp32 MFMA sum over B1 <= 1024 terms (sqrt(1024) 6e-8 = 1.9e-6):
  1.3e-5, bound 2e-5. Eight layers: 2 x 7 x 1.8e-6 = 2.5e-5, with the same factor of about two: 5e-5.
- nsvd_spin_solve: test_spin_gpu's, for cond(sigma_avg + 1e-3 I) < 2e4 (asserted on the float64 side): 1e-9 on the
  float64 outputs, 1e-6 on sigma_avg and chol.

Measured on an MI355X, the worst over the two calls and the tensors of a shape (per-tensor relative error of J / of the
gradients, then the worst (a, c) slice of J / head of the gradients against A):

    (L, m, hidden, B1, D)              J        gradients  (a, c) slice  head     bound
    (10, 64, (128, 128), 130, 2)       2.0e-7   2.6e-7     2.9e-7        2.4e-7   2e-5
    (9, 8, (260,), 33, 3)              1.2e-7   1.3e-7     1.3e-7        8.9e-8   2e-5
    (17, 72, (33, 33), 97, 5)          1.9e-7   2.4e-7     3.0e-7        1.1e-7   2e-5
    (63, 8, (16,), 34, 4)              1.1e-7   1.4e-7     2.6e-7        5.2e-8   2e-5
    (64, 8, (136,), 40, 64)            1.3e-7   1.5e-7     3.0e-7        5.2e-8   2e-5
    (10, 96, (136, 40), 128, 2)        1.8e-7   2.1e-7     2.8e-7        1.6e-7   2e-5
    (2, 130, (8,), 2, 1)               1.2e-7   1.4e-7     2.0e-7        1.5e-7   2e-5
    (3, 8, (16,) * 7, 25, 2)           1.7e-7   2.9e-7     1.9e-7        2.0e-7   5e-5
    (4, 8, (16, 16), 1024, 2)          4.7e-7   4.2e-7     9.0e-7        3.4e-7   2e-5
    (5, 8, (), 31, 2)                  1.3e-7   1.3e-7     7.0e-8        7.1e-8   2e-5

(for scale, a separate run on the CPU of S.jacobian_contraction_einsum in float32 with torch, the same inputs and metric,
worst (a, c) slice per shape in the table's order: 2.9e-7 1.5e-7 2.6e-7 2.5e-7 2.9e-7 2.8e-7 2.1e-7 1.8e-7 1.9e-7 7.0e-8 -
the kernel's errors are those of any float32 evaluation of these sums; no bound is taken from either column.)
No slice needed the float32 yardstick; the poisoned and the zero-filled workspace gave equal bits and every margin kept
its sentinel at every shape. nsvd_spin_solve, the worst per group (cond <= 8.8, rank-deficient sigma: <= 6.3e2):

    group                    sigma_avg  chol     loss     eigvals  gsigma   gpi
    more L                   3.8e-8     4.0e-8   1.3e-14  6.2e-16  8.0e-16  4.6e-16
    rank-deficient sigma     2.6e-8     3.1e-8   7.8e-14  2.4e-14  3.0e-14  1.8e-14
    decay = 0                0 (bits)   3.6e-8   1.2e-15  5.7e-16  6.9e-16  4.3e-16
    three scales             3.0e-8     2.9e-8   4.4e-15  4.8e-16  7.2e-16  3.0e-16
    after a failed solve     2.5e-8     2.2e-8   6.0e-15  4.3e-16  7.4e-16  4.4e-16
"""
import pytest
import torch

from tests import _spin_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64

# =============================================================================================== guarded buffers
GUARD = 256               # 4-byte words of margin on either side of a view
# 1.236 as a float32, one ulp = 1.2e-7: a store, J's `x = (1 - decay) x + ..` and the gradients' `x += s` (the only write
# spin_reduce_kernel makes, |s| ~ 1e-3 .. 1 here) all change its bits; a large pattern would round such a sum back to itself
SENTINEL = 0x3F9E3779


class Guarded:
    """`words` 4-byte words with GUARD sentinel words before and after them"""

    def __init__(self, words):
        self.words = int(words)
        self.buf = torch.full((self.words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)

    def floats(self, *shape):
        return self.buf[GUARD:GUARD + self.words].view(torch.float32).view(*shape)

    def bytes(self):
        return self.buf[GUARD:GUARD + self.words].view(torch.uint8)

    def intact(self):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.words:]
        return hi.numel() == GUARD and bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())


def _guarded_like(tensors, fill):
    guards = [Guarded(t.numel()) for t in tensors]
    views = [g.floats(*t.shape).fill_(fill) for g, t in zip(guards, tensors)]
    return guards, views


# =============================================================================================== 1. Jacobian contraction
# (L, m, hidden, B1, D); F = 2 m inputs of layer 0; nrt = ceil(h / 32) row tiles, nkt = ceil(kin / 128) column tiles
JAC_SHAPES = [
    # the scripts' default L: two blocks with AB = 5 (< SP_AB with nblocks > 1); five chunks, the last with 2 samples
    pytest.param(10, 64, (128, 128), 130, 2, id="L10_blocks5+5_B130_chunks5"),
    # blocks 5 + 4 (na < AB); h = 260: nine row tiles, the last with 4 rows; last layer kin = 260: three column tiles, the
    # last 4 columns wide (wave 0 alone live, 4 lanes of it)
    pytest.param(9, 8, (260,), 33, 3, id="L9_blocks5+4_h260_nrt9_nkt3"),
    # blocks 6 + 6 + 5; F = 144: second column tile 16 wide; h = 33: second row tile with one row; odd kin and odd B1: the
    # scalar GEMM instance for the activations and the deltas
    pytest.param(17, 72, (33, 33), 97, 5, id="L17_blocks6+6+5_F144_h33_scalar_gemm"),
    # eight blocks: seven of 8 and the last of 7
    pytest.param(63, 8, (16,), 34, 4, id="L63_blocks7x8+7"),
    # the largest L and D; last layer kin = 136: second column tile 8 wide; J is 40 MB
    pytest.param(64, 8, (136,), 40, 64, id="L64_D64_kin136"),
    # F = 192: second column tile 64 wide, waves 2 and 3 off; h = 136 ragged over five row tiles; B1 a multiple of 4 with
    # no tail: the vectorised GEMM instance
    pytest.param(10, 96, (136, 40), 128, 2, id="L10_F192_waves_off_h136_vector_gemm"),
    # the smallest B1; F = 260: three column tiles in layer 0, the bias from kt == 0 alone
    pytest.param(2, 130, (8,), 2, 1, id="B2_F260_nkt3_bias_kt0"),
    # NSVD_MAX_LAYERS = 8 layers
    pytest.param(3, 8, (16,) * 7, 25, 2, id="layers8"),
    # 32 chunks
    pytest.param(4, 8, (16, 16), 1024, 2, id="B1024_chunks32"),
    # one layer: no hidden layer, no activation buffer, the delta is the constant
    pytest.param(5, 8, (), 31, 2, id="layers1"),
]


def jac_bound(hidden):
    return 5e-5 if len(hidden) > 3 else 2e-5


def _slice_errors(got, want, scale, lead):
    """got, want, scale: float64 with `lead` leading slice axes. Returns (||got - want|| / ||want||, ||got - want|| /
    ||scale||, max over the slices of ||got - want||_slice / ||scale||_slice)."""
    shape = tuple(want.shape[:lead]) + (-1,)
    d = (got.reshape(want.shape) - want).reshape(shape)
    sc = scale.reshape(shape).norm(dim=-1)
    assert bool((sc > 0).all())
    return (float(d.norm() / want.norm()), float(d.norm() / scale.norm()), float((d.norm(dim=-1) / sc).max()))


@pytest.mark.parametrize("L,m,hidden,B1,D", JAC_SHAPES)
def test_spin_jac_step_shapes(L, m, hidden, B1, D):
    """test_spin_jac_step_matches_the_oracle's body (two calls, the float64 einsum oracle, the bit-equal re-run, `adds to
    the gradient buffers`) with the per-slice metric, guarded buffers and the poisoned workspace. What a wrong line of
    spin_jac_kernel would do here:
    - `col` without k0: every column tile would write tile 0's columns - the slices of W_i with kin > 128 lose their
      columns 128.. (error ~ 1 against A in every (a, c) slice of that tensor, all shapes with nkt > 1);
    - a0 = ab * SP_AB instead of ab * A.AB: at L = 10 block 1 would start at a = 8 - a = 5, 6, 7 are never written (J
      stays at its previous state: slice error ~ 1) and the gradients lose their terms;
    - kt > 0 tiles writing the bias: (1 - decay) would be applied nkt times to J's bias slices and the partial sums of
      the later tiles would overwrite part[offb ..]: bias slices of J and the bias gradients off by ~ 1, and no two
      runs need agree on which tile wrote last."""
    from neural_svd_amd import hip_ops as H
    torch.manual_seed(11 * L + B1)
    fB, ws, bs = S.init_params(L, D, m, hidden, seed=500 + L)
    bs = [0.1 * torch.randn_like(b) for b in bs]
    shape = H.ModelShape(L=L, D=D, m=m, hidden=hidden)
    c, decay, bound = 0.7, 0.3, jac_bound(hidden)
    dev_t = [t.to(DEV).contiguous() for t in ws + bs]
    params = S.pack_tensors(H, shape, dev_t, fB.to(DEV).contiguous())
    P = H.spin_state_floats(shape)
    assert P == sum(t.numel() for t in ws + bs)

    ws_probe = H.spin_jac_workspace(shape, B1, DEV)
    assert ws_probe.numel() % 4 == 0
    wsg = Guarded(ws_probe.numel() // 4)
    work = wsg.bytes().zero_()
    assert work.numel() == ws_probe.numel() and work.data_ptr() % 256 == 0
    del ws_probe
    Jg = Guarded(L * P)
    J = Jg.floats(L, P).zero_()
    guards = [wsg, Jg]

    J64 = [torch.zeros((L,) + tuple(t.shape), dtype=F64) for t in ws + bs]
    A64 = [torch.zeros_like(j) for j in J64]
    ws64, bs64 = [w.double() for w in ws], [b.double() for b in bs]
    snapshot, worst = None, [0.0] * 4
    for call in range(2):  # the second call's moving average meets non-zero state
        x = (1.5 / (1 + D) ** 0.5) * torch.randn(B1, D)
        gsigma = torch.randn(L, L, dtype=F64)
        phi64 = S.model_forward(x.double(), fB.double(), ws64, bs64, c)
        phi = phi64.float().contiguous()
        j_new = S.jacobian_contraction_einsum(x.double(), phi.double(), fB.double(), ws64, bs64, c)
        a_new = S.jacobian_contraction_abs(x.double(), phi.double(), fB.double(), ws64, bs64, c)
        J64 = [(1.0 - decay) * jo + decay * jn for jo, jn in zip(J64, j_new)]
        A64 = [(1.0 - decay) * ao + decay * an for ao, an in zip(A64, a_new)]
        want_g = [torch.einsum("ac,ac...->c...", gsigma, j) for j in J64]
        scale_g = [torch.einsum("ac,ac...->c...", gsigma.abs(), a) for a in A64]
        gg, grads = _guarded_like(dev_t, 0.0)
        guards += gg
        args = (shape, params, x.to(DEV), phi.to(DEV), c, gsigma.to(DEV), decay)
        if call == 1:
            snapshot = J.clone()
        H.spin_jac_step(*args, J, S.pack_tensors(H, shape, grads), work)
        Jc = J.cpu().double()
        off = 0
        for i, (j64, a64, g64, s64, g) in enumerate(zip(J64, A64, want_g, scale_g, grads)):
            nel = j64[0].numel()
            assert bool((j64.abs() <= a64 * (1 + 1e-12)).all())
            ej, ej_abs, ej_slice = _slice_errors(Jc[:, off:off + nel], j64, a64, 2)
            eg, eg_abs, eg_slice = _slice_errors(g.cpu().double(), g64, s64, 1)
            print(f"spin_jac_step {(L, m, hidden, B1, D)} call={call} tensor={i} J={ej:.2e} grad={eg:.2e} against A: "
                  f"J={ej_abs:.2e} worst (a, c)={ej_slice:.2e} grad={eg_abs:.2e} worst head={eg_slice:.2e}")
            assert ej <= bound and eg <= bound, (call, i, ej, eg)
            assert ej_abs <= bound and eg_abs <= bound, (call, i, ej_abs, eg_abs)
            assert ej_slice <= bound and eg_slice <= bound, (call, i, ej_slice, eg_slice)
            worst = [max(a, b) for a, b in zip(worst, (ej, eg, ej_slice, eg_slice))]
            off += nel
        assert off == P
    print(f"spin_jac_step {(L, m, hidden, B1, D)} worst: J={worst[0]:.2e} grad={worst[1]:.2e} (a, c) slice={worst[2]:.2e} "
          f"head={worst[3]:.2e} bound={bound:.0e}")

    def rerun(fill):
        jg = Guarded(L * P)
        j2 = jg.floats(L, P).copy_(snapshot)
        gg2, g2 = _guarded_like(dev_t, fill)
        guards.extend([jg] + gg2)
        H.spin_jac_step(*args, j2, S.pack_tensors(H, shape, g2), work)
        return j2, g2

    # the same call from the same state (the workspace as the calls before left it): equal bits (no atomics)
    J2, grads2 = rerun(0.0)
    assert torch.equal(J2, J)
    for a, b in zip(grads, grads2):
        assert torch.equal(a, b)
    # the workspace full of NaN bit patterns, then zero-filled: nothing of what it held reaches a result
    work.fill_(0xFF)
    assert bool(torch.isnan(work.view(torch.float32)).all())
    Jp, gradsp = rerun(0.0)
    work.zero_()
    Jz, gradsz = rerun(0.0)
    for t in [Jp, Jz] + gradsp + gradsz:
        assert bool(torch.isfinite(t).all())
    assert torch.equal(Jp, Jz) and torch.equal(Jp, J)
    for a, p, z in zip(grads, gradsp, gradsz):
        assert torch.equal(p, z) and torch.equal(a, p)
    # the step ADDS to what the gradient buffers hold
    _, grads3 = rerun(0.25)
    for a, b in zip(grads, grads3):
        assert torch.equal(0.25 + a, b)
    # nothing was written outside J, the gradient tensors and the workspace
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), [i for i, g in enumerate(guards) if not g.intact()]


# =============================================================================================== 2. the small solve
class Solve:
    """the buffers of nsvd_spin_solve; the outputs start as NaN so that every call has to write them"""

    def __init__(self, L, state=None, status=0):
        nan = float("nan")
        self.L = L
        self.state = torch.zeros((L, L), dtype=torch.float32, device=DEV) if state is None else state.float().to(DEV)
        self.chol = torch.full((L, L), nan, dtype=torch.float32, device=DEV)
        self.le = torch.full((L + 1,), nan, dtype=F64, device=DEV)
        self.gs = torch.full((L, L), nan, dtype=F64, device=DEV)
        self.gp = torch.full((L, L), nan, dtype=F64, device=DEV)
        self.status = torch.full((1,), status, dtype=torch.int32, device=DEV)

    def __call__(self, S_raw, sscale, Pi_raw, pscale, decay, gscale):
        from neural_svd_amd import hip_ops as H
        H.spin_solve(S_raw.to(DEV), sscale, Pi_raw.to(DEV), pscale, decay, gscale, self.state, self.chol, self.le, self.gs,
                     self.gp, self.status)

    def outputs(self):
        return self.chol, self.le, self.gs, self.gp

    def errors(self, new, want, gscale):
        return dict(sigma_avg=S.rel_err(self.state.cpu(), new), chol=S.rel_err(self.chol.cpu(), want["chol"]),
                    loss=S.rel_err(self.le[:1].cpu(), want["loss"]), eigvals=S.rel_err(self.le[1:].cpu(), want["eigvals"]),
                    gsigma=S.rel_err(self.gs.cpu(), want["gsigma"]), gpi=S.rel_err(self.gp.cpu(), gscale * want["gpi"]))

    def check(self, what, ref_state, sigma, pi, decay, gscale):
        """every output against the oracle on the float64 moving average of ref_state; returns the new reference state"""
        new, want = S.solve_ref(ref_state, sigma, pi, decay)
        cond = float(torch.linalg.cond(new + 1e-3 * torch.eye(self.L, dtype=F64)))
        assert cond < 2e4, cond
        errs = self.errors(new, want, gscale)
        print(f"spin_solve {what} L={self.L} decay={decay} cond={cond:.2e} " +
              " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        assert errs["sigma_avg"] <= 1e-6 and errs["chol"] <= 1e-6, errs
        assert max(errs["loss"], errs["eigvals"], errs["gsigma"], errs["gpi"]) <= 1e-9, errs
        assert not bool(torch.triu(self.chol, 1).count_nonzero())
        return self.state.cpu().double()  # the state is float32: the next step starts from its rounded value


def _moments(g, L, rows=None, row_scale=1.0):
    """test_spin_solve_matches_float64's recipe: sigma_raw = X^T X of n rows, pi_raw = Y^T Z of B1 rows"""
    n, B1 = (4 * L + 3 if rows is None else rows), 2 * L + 1
    X = torch.randn(n, L, generator=g, dtype=F64) * row_scale
    Y = torch.randn(B1, L, generator=g, dtype=F64)
    Z = torch.randn(B1, L, generator=g, dtype=F64)
    return X.T @ X, n, Y.T @ Z, B1


@pytest.mark.parametrize("decay", [0.01, 1.0])
@pytest.mark.parametrize("L", [3, 9, 10, 17, 33, 63])
def test_spin_solve_more_L(L, decay):
    """odd L (ld = L | 1 = L: no padding column) and L between the tested powers of two, two calls each"""
    g = torch.Generator().manual_seed(100 + L)
    sv = Solve(L)
    ref = torch.zeros((L, L), dtype=F64)
    for call in range(2):  # the second call meets non-zero state
        S_raw, n, Pi_raw, B1 = _moments(g, L, row_scale=0.3 if decay == 1.0 else 1.0)
        sv(S_raw, 1.0 / n, Pi_raw, 1.0 / B1, decay, 1.0 / B1)
        assert int(sv.status.item()) == 0
        ref = sv.check(f"call={call}", ref, S_raw / n, Pi_raw / B1, decay, 1.0 / B1)


@pytest.mark.parametrize("L", [3, 10, 17, 33, 64])
def test_spin_solve_rank_deficient_sigma(L):
    """sigma of rank max(1, L // 2) factored itself (decay = 1): the 1e-3 I term alone holds the other pivots up"""
    g = torch.Generator().manual_seed(200 + L)
    sv = Solve(L)
    ref = torch.zeros((L, L), dtype=F64)
    rows = max(1, L // 2)
    for call in range(2):
        S_raw, n, Pi_raw, B1 = _moments(g, L, rows=rows, row_scale=0.3)
        assert int(torch.linalg.matrix_rank(S_raw)) == rows < L
        sv(S_raw, 1.0 / n, Pi_raw, 1.0 / B1, 1.0, 1.0 / B1)
        assert int(sv.status.item()) == 0
        ref = sv.check(f"rank={rows} call={call}", ref, S_raw / n, Pi_raw / B1, 1.0, 1.0 / B1)


@pytest.mark.parametrize("L", [3, 10, 64])
def test_spin_solve_decay_zero_keeps_the_state(L):
    """decay = 0 on a non-zero state: sigma_avg keeps its bits and every output is the oracle's on that state, whatever
    sigma_raw holds"""
    g = torch.Generator().manual_seed(300 + L)
    S0, n, Pi0, B1 = _moments(g, L)
    sv = Solve(L)
    sv(S0, 1.0 / n, Pi0, 1.0 / B1, 1.0, 1.0 / B1)
    before = sv.state.clone()
    assert bool(before.count_nonzero())
    S_raw, n, Pi_raw, B1 = _moments(g, L)
    sv(S_raw, 1.0 / n, Pi_raw, 1.0 / B1, 0.0, 1.0 / B1)
    assert int(sv.status.item()) == 0
    assert torch.equal(sv.state, before)
    sv.check("decay=0", before.cpu().double(), S_raw / n, Pi_raw / B1, 0.0, 1.0 / B1)


@pytest.mark.parametrize("L", [5, 10, 33])
def test_spin_solve_three_distinct_scales(L):
    """sigma_scale, pi_scale and gpi_scale all different: gpi_scaled = 0.37 x the oracle's gpi"""
    g = torch.Generator().manual_seed(400 + L)
    sv = Solve(L)
    ref = torch.zeros((L, L), dtype=F64)
    for call in range(2):
        S_raw, n, Pi_raw, B1 = _moments(g, L)
        sv(S_raw, 1.0 / n, Pi_raw, 1.0 / B1, 0.25, 0.37)
        assert int(sv.status.item()) == 0
        ref = sv.check(f"scales call={call}", ref, S_raw / n, Pi_raw / B1, 0.25, 0.37)


@pytest.mark.parametrize("bad", ["sigma_nan", "sigma_inf", "pi_nan"])
@pytest.mark.parametrize("L", [3, 10, 64])
def test_spin_solve_non_finite_moments(L, bad):
    """one non-finite element among the moments: RITZ_BAD_PIVOT, every output exactly zero, nothing non-finite stored.
    sigma_raw: the element of sigma_avg the value would go to keeps its previous value, every other element holds the
    moving average. pi_raw: sigma_avg is fully updated."""
    from neural_svd_amd import hip_ops as H
    g = torch.Generator().manual_seed(500 + L)
    S0, n, Pi0, B1 = _moments(g, L)
    sv = Solve(L)
    sv(S0, 1.0 / n, Pi0, 1.0 / B1, 1.0, 1.0 / B1)  # a non-zero state, and outputs that are not zero
    assert int(sv.status.item()) == 0
    assert all(bool(t.count_nonzero()) for t in sv.outputs())
    before = sv.state.cpu().double()
    S_raw, n, Pi_raw, B1 = _moments(g, L)
    i, j = L - 1, L // 2
    value = float("inf") if bad == "sigma_inf" else float("nan")
    (Pi_raw if bad == "pi_nan" else S_raw)[i, j] = value
    decay = 0.25
    sv(S_raw, 1.0 / n, Pi_raw, 1.0 / B1, decay, 1.0 / B1)
    assert int(sv.status.item()) == H.RITZ_BAD_PIVOT
    for t in (sv.state,) + sv.outputs():
        assert bool(torch.isfinite(t).all())
    for t in sv.outputs():
        assert not bool(t.count_nonzero())
    want = (1.0 - decay) * before + decay * S_raw / n
    got = sv.state.cpu().double()
    if bad != "pi_nan":
        assert float(got[i, j]) == float(before[i, j])
        want[i, j] = before[i, j]
    assert bool(torch.isfinite(want).all())
    assert S.rel_err(got, want) <= 1e-6
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("L", [3, 10, 64])
def test_spin_solve_status_accumulates(L):
    """status is OR-ed into, never cleared (SpinKernelTrainer.check() reads it once after many steps): a bit somebody
    else set survives a failing and a good solve, the failing solve adds RITZ_BAD_PIVOT, the good solve after it changes
    nothing in status and still delivers its outputs"""
    from neural_svd_amd import hip_ops as H
    other = H.RITZ_SWEEP_CAP
    assert other != H.RITZ_BAD_PIVOT and other & H.RITZ_BAD_PIVOT == 0
    g = torch.Generator().manual_seed(600 + L)
    sv = Solve(L, state=-torch.eye(L), status=other)
    S_raw, n, Pi_raw, B1 = _moments(g, L)
    sv(S_raw, 1.0 / n, Pi_raw, 1.0 / B1, 0.01, 1.0 / B1)  # 0.99 (-I) + 0.01 sigma: an indefinite matrix
    assert int(sv.status.item()) == other | H.RITZ_BAD_PIVOT
    assert not any(bool(t.count_nonzero()) for t in sv.outputs())
    S_raw, n, Pi_raw, B1 = _moments(g, L)
    sv(S_raw, 1.0 / n, Pi_raw, 1.0 / B1, 1.0, 1.0 / B1)  # decay 1: the state is replaced by a definite matrix
    assert int(sv.status.item()) == other | H.RITZ_BAD_PIVOT
    assert all(bool(t.count_nonzero()) for t in sv.outputs())
    sv.check("after a failed solve", torch.zeros((L, L), dtype=F64), S_raw / n, Pi_raw / B1, 1.0, 1.0 / B1)
