"""evd_loss.hip at every dispatch branch, against float64 on the same float32 inputs.

Reference (float64 torch on the CPU): f1, f2 = chunk(f, 2) (the first half gets the ceiling), lam_h = f_h^T f_h / B_h,
the operator moment mean_b sum_l v_l f Tf, loss and d loss / d f from O.evd_loss_forward / O.evd_loss_backward; masks
from O.sequential_nesting_masks / O.joint_nesting_masks(L, 1); "custom" is the joint masks at step 2, by pointer.

Which shape reaches which branch is DERIVED from the dispatch code (evd_loss.hip: fused_ok, evd_partial_cuts,
chunk_gram, evd_reduce_kernel's sum_chunks, the 48 KiB test of nsvd_evd_loss_grad and launch_fused, the `parts` loop and
the (n & 3) staging test of evd_fused_kernel) - restated below in `dispatch` and asserted per shape, not observed in a
run. fused_ok is B * L <= 16384 and L <= 64 and B >= 2: no pipeline shape satisfies it, every fused shape does.

Pipeline (evd_partial_kernel -> evd_reduce_kernel -> evd_loss_grad_kernel); chunks are 64 rows, per half:
  (B, L, mask)          chunks   cuts  NQ  JC   what it is here for
  (130, 65, custom)     2 + 2    1     16  no   L > 64 at a tiny batch; second chunk of each half holds 1 row
  (3301, 5, seq)        26 + 26  1     2   no   odd B (1651 + 1650); the reduce sums 3 eights + 2
  (1100, 16, joint)     9 + 9    1     2   yes  one eight + 1 in the reduce
  (771, 23, custom)     7 + 7    1     4   no   fewer than 8 chunks: the reduce's scalar tail alone; last chunks 2 / 1 rows
  (600, 32, seq)        5 + 5    1     4   yes
  (300, 64, joint)      3 + 3    4     4   yes  span 1024 per workgroup
  (16400, 64, seq)      129+129  2     16  yes  258 chunks
  (32770, 64, joint)    257+257  1     16  yes  514 chunks: no cut at L = 64, NQ 16 over the whole block
  (400, 96, custom)     4 + 4    4     16  no   span 2304; loss/grad LDS 61,440 bytes (hipFuncSetAttribute branch)
  (1031, 128, joint)    9 + 9    8     16  yes  MAXL; loss/grad LDS 98,304 bytes
  (257, 64, seq)        3 + 2    4     4   yes  first B past FUSED_MAX at L = 64 (B * L = 16448); a chunk of one row
  (4097, 4, joint)      33 + 32  1     2   no   first B past FUSED_MAX at L = 4 (B * L = 16388); a chunk of one row
  (1, 3, seq)           1 + 0    1     2   no   B2 == 0: lam_f2 all NaN like the reference; lam_f1 and the operator
                                                moment right; loss[1] right, loss[0], loss[2] and df NaN like the reference

Fused (evd_fused_kernel<1> for the moments, <3> for the one-call entry point), each with all three mask kinds:
  (B, L)       parts  staging  what it is here for
  (3, 2)       16     scalar   B2 == 1
  (37, 8)      8      vector
  (50, 10)     4      vector   L % 4 != 0: the mask index wraps inside a float4
  (51, 11)     4      scalar
  (1024, 16)   2      vector   exactly FUSED_MAX; 67,712 bytes of LDS (the last three: hipFuncSetAttribute branch)
  (963, 17)    1      scalar
  (481, 34)    1      scalar   L not a power of two

Every output is pre-filled with NaN (777 at B = 1, where NaN is the right answer for some): an element no kernel
stores fails its comparison.

Bars (the project's own): moments 2e-6 in relative L2 AND as the largest entry error over the largest |lam| entry;
df 5e-6 in relative L2 AND per row (each row's error over that row's norm, the maximum over rows); loss
2e-5 * max(1, |loss|); loss[1] + loss[2] == loss[0] to 1e-4. The operator moment is a sum of B L products of either
sign: it is held to 2e-6 of mean_b sum_l |v_l f Tf|, the scale its float32 rounding errors are relative to (each
thread's chain is at most 32 fused multiply-adds, then a wave sum, then up to 514 chunk sums in order:
sqrt(514) * 2^-24 = 1.4e-6 of the RUNNING sum, which is some 100 x smaller than that scale).

Measured on MI355X (worst over all cases): moments 3.40e-7 in L2 and 6.40e-7 in max norm (both (963, 17), fused; the
pipeline's worst is (32770, 64): 2.31e-7 / 5.34e-7), operator moment 1.7e-8, df 1.22e-7 in L2 and 1.35e-6 per row (the
row of (4097, 4) whose gradient nearly cancels: float32 numpy gives 1.55e-6 on the same row; every other shape is
below 3.6e-7), loss 5.5e-7.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = None
CH, MAXL, FUSED_MAX, FUSED_THREADS = 64, 128, 16384, 1024

# (B, L, mask): chunks of the halves, cuts, NQ, JC, bytes of dynamic LDS of the loss / gradient kernel
PIPELINE = {
    (130, 65, "custom"): ((2, 2), 1, 16, False, 33540),
    (3301, 5, "seq"): ((26, 26), 1, 2, False, 1380),
    (1100, 16, "joint"): ((9, 9), 1, 2, True, 5120),
    (771, 23, "custom"): ((7, 7), 1, 4, False, 8004),
    (600, 32, "seq"): ((5, 5), 1, 4, True, 12288),
    (300, 64, "joint"): ((3, 3), 4, 4, True, 32768),
    (16400, 64, "seq"): ((129, 129), 2, 16, True, 32768),
    (32770, 64, "joint"): ((257, 257), 1, 16, True, 32768),
    (400, 96, "custom"): ((4, 4), 4, 16, False, 61440),
    (1031, 128, "joint"): ((9, 9), 8, 16, True, 98304),
    (257, 64, "seq"): ((3, 2), 4, 4, True, 32768),
    (4097, 4, "joint"): ((33, 32), 1, 2, False, 1088),
    (1, 3, "seq"): ((1, 0), 1, 2, False, 804),
}
# (B, L): parts, 16-byte staging
FUSED = {(3, 2): (16, False), (37, 8): (8, True), (50, 10): (4, True), (51, 11): (4, False), (1024, 16): (2, True),
         (963, 17): (1, False), (481, 34): (1, False)}
KINDS = ("seq", "joint", "custom")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import hip_ops
    H = hip_ops
    yield
    # (for the record in this file's docstring; shown with -s)
    print("\nevd shapes, worst over all cases: " + ", ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


def fused_ok(B, L):
    return B * L <= FUSED_MAX and L <= 64 and B >= 2


def dispatch(B, L):
    """evd_loss.hip's choices for the three-launch pipeline, restated"""
    B1 = (B + 1) // 2
    B2 = B - B1
    n1, n2 = -(-B1 // CH), -(-B2 // CH)
    LL = L * L
    cuts = 1
    while cuts < 8 and (n1 + n2) * cuts < 512 and LL % (256 * 2 * cuts) == 0 and LL // (2 * cuts) >= 1024:
        cuts *= 2
    span = LL // cuts
    assert cuts == 1 or span % 256 == 0
    nq = 2 if span <= 512 else 4 if span <= 1024 else 16
    jc = 256 % L == 0 and LL >= 256
    return (n1, n2), cuts, nq, jc, (LL + CH * L) * 4


def fused_dispatch(B, L):
    parts = 1
    while parts * 2 <= 16 and parts * 2 * 2 * L * L <= FUSED_THREADS:
        parts *= 2
    return parts, (B * L) % 4 == 0


def test_the_shapes_reach_the_branches_they_are_here_for():
    for (B, L, _), want in PIPELINE.items():
        assert not fused_ok(B, L) and L <= MAXL
        assert dispatch(B, L) == want, (B, L, dispatch(B, L))
    for (B, L), want in FUSED.items():
        assert fused_ok(B, L)
        assert fused_dispatch(B, L) == want, (B, L, fused_dispatch(B, L))
    got = {(nq, jc) for _, _, nq, jc, _ in PIPELINE.values()}
    assert got == {(nq, jc) for nq in (2, 4, 16) for jc in (False, True)}
    assert {c for _, c, _, _, _ in PIPELINE.values()} == {1, 2, 4, 8}
    assert {p for p, _ in FUSED.values()} == {1, 2, 4, 8, 16}
    assert fused_ok(256, 64) and fused_ok(4096, 4) and FUSED_MAX == 1024 * 16   # the last shapes inside the boundary
    # the 48 KiB branches: loss / gradient kernel at L = 96, 128 and not below; the fused kernel at (1024, 16)
    assert sorted(L for (_, L, _), w in PIPELINE.items() if w[4] > 48 * 1024) == [96, 128]
    fused_lds = {(B, L): (B * L + 2 * L * L + 32) * 4 for B, L in FUSED}
    assert fused_lds[(1024, 16)] == 67712 and fused_lds[(963, 17)] > 48 * 1024 and fused_lds[(481, 34)] > 48 * 1024
    assert all(fused_lds[s] < 48 * 1024 for s in ((3, 2), (37, 8), (50, 10), (51, 11)))


def masks(kind, L):
    if kind == "seq":
        return O.sequential_nesting_masks(L)
    return O.joint_nesting_masks(L, 1 if kind == "joint" else 2)


@functools.lru_cache(maxsize=None)
def case(B, L, kind):
    """inputs and the float64 reference, computed once per (B, L, mask) and shared; nothing writes to them"""
    g = torch.Generator().manual_seed(B * 131 + L)
    f = torch.randn(B, L, generator=g)
    Tf = 3.0 * torch.randn(B, L, generator=g)
    v, M = masks(kind, L)
    f64, T64, v64, M64 = f.double(), Tf.double(), v.double(), M.double()
    loss, lam1, lam2, lop, lmet = O.evd_loss_forward(f64, T64, v64, M64)
    if B > 1:
        df = O.evd_loss_backward(f64, T64, v64, M64, lam1, lam2)
    else:  # no second half (the oracle divides by its row count): the one row's gradient, through lam2 = 0 / 0
        df = -(4.0 / B) * T64 * v64.unsqueeze(0) + 2.0 * (f64 @ (M64 * lam2))
        assert torch.isnan(lam2).all() and torch.isnan(df).all()
    terms = f64 * T64 * v64.unsqueeze(0)
    return dict(f=f, Tf=Tf, v=v.float().contiguous(), M=M.float().contiguous(), lam1=lam1.numpy(), lam2=lam2.numpy(),
                opm=float(terms.sum(1).mean()), op_scale=float(terms.abs().sum(1).mean()),
                loss=np.array([float(loss), float(lop), float(lmet)]), df=df.numpy())


WORST = dict(mom_l2=0.0, mom_max=0.0, op=0.0, df_l2=0.0, df_row=0.0, loss=0.0)


def _note(key, val):
    WORST[key] = max(WORST[key], val)
    return val


def check_moments(lam1, lam2, opm, c, what):
    for h, (got, want) in enumerate(((lam1, c["lam1"]), (lam2, c["lam2"]))):
        got = np.asarray(got, dtype=np.float64).reshape(want.shape)
        if np.isnan(want).any():     # B2 == 0: 0 / 0 in every entry, like the reference
            assert np.isnan(want).all() and np.isnan(got).all(), what
            continue
        l2 = _note("mom_l2", float(np.linalg.norm(got - want) / np.linalg.norm(want)))
        mx = _note("mom_max", float(np.abs(got - want).max() / np.abs(want).max()))
        print(f"{what} lam{h + 1}: L2 {l2:.2e} max {mx:.2e}")
        assert l2 < 2e-6 and mx < 2e-6, (what, h, l2, mx)
    e = _note("op", abs(float(opm) - c["opm"]) / c["op_scale"])
    print(f"{what} operator moment: {e:.2e} of mean_b sum_l |v f Tf|")
    assert e < 2e-6, (what, e)


def check_loss(loss, c, what):
    got = loss.double().cpu().numpy()
    for i in range(3):
        want = c["loss"][i]
        if np.isnan(want):
            assert np.isnan(got[i]), (what, i)
            continue
        e = _note("loss", abs(got[i] - want) / max(1.0, abs(want)))
        assert e < 2e-5, (what, i, got[i], want)
    if not np.isnan(c["loss"][0]):
        assert abs(got[1] + got[2] - got[0]) < 1e-4 * max(1.0, abs(got[0])), what
    print(f"{what} loss: {got} want {c['loss']}")


def check_df(df, c, what):
    got, want = df.double().cpu().numpy(), c["df"]
    if np.isnan(want).any():         # B == 1: the other half's moments are 0 / 0, like the reference
        assert np.isnan(want).all() and np.isnan(got).all(), what
        return
    l2 = _note("df_l2", float(np.linalg.norm(got - want) / np.linalg.norm(want)))
    row = _note("df_row", float((np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)).max()))
    print(f"{what} df: L2 {l2:.2e} worst row {row:.2e}")
    assert l2 < 5e-6 and row < 5e-6, (what, l2, row)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_calls(B, L, kind, pipeline):
    c = case(B, L, kind)
    what = f"({B}, {L}, {kind})"
    fill = 777.0 if B == 1 else float("nan")
    mk = {"seq": H.MASK_SEQUENTIAL, "joint": H.MASK_JOINT, "custom": H.MASK_CUSTOM}[kind]
    f, Tf = c["f"].to(DEV), c["Tf"].to(DEV)
    v = c["v"].to(DEV) if kind == "custom" else None
    M = c["M"].to(DEV) if kind == "custom" else None
    LL = L * L

    def filled(*shape):
        return torch.full(shape, fill, dtype=torch.float32, device=DEV)

    def scratch():
        s = H.evd_scratch(B, L, DEV)
        s.view(torch.float32).fill_(fill)
        return s

    # the moments, then loss and gradient from them
    mom = H.evd_moments(f, Tf, mk, v, moments=filled(2 * LL + 1), scratch=scratch())
    m = mom.double().cpu().numpy()
    check_moments(m[:LL], m[LL:2 * LL], m[2 * LL], c, what + " evd_moments")
    loss, df = H.evd_loss_grad(f, Tf, mk, v, M, mom, loss=filled(3), df=filled(B, L))
    check_loss(loss, c, what + " evd_loss_grad")
    check_df(df, c, what + " evd_loss_grad")
    loss_only, none = H.evd_loss_grad(f, Tf, mk, v, M, mom, want_grad=False, loss=filled(3))
    assert none is None and bits_equal(loss_only, loss)
    # grad_scale: a power of two scales exactly
    _, df_q = H.evd_loss_grad(f, Tf, mk, v, M, mom, grad_scale=0.25, loss=filled(3), df=filled(B, L))
    assert bits_equal(df_q * 4, df), what
    # the one-call entry point, with the gradient and loss-only
    mom_f, loss_f, df_f = filled(2 * LL + 1), filled(3), filled(B, L)
    H.evd_loss_fused(f, Tf, mk, v, M, mom_f, loss_f, df_f, scratch())
    mf = mom_f.double().cpu().numpy()
    check_moments(mf[:LL], mf[LL:2 * LL], mf[2 * LL], c, what + " evd_loss_fused")
    check_loss(loss_f, c, what + " evd_loss_fused")
    check_df(df_f, c, what + " evd_loss_fused")
    mom_n, loss_n = filled(2 * LL + 1), filled(3)
    H.evd_loss_fused(f, Tf, mk, v, M, mom_n, loss_n, None, scratch())
    assert bits_equal(mom_n, mom_f) and bits_equal(loss_n, loss_f), what
    _, df_fq = filled(3), filled(B, L)
    H.evd_loss_fused(f, Tf, mk, v, M, filled(2 * LL + 1), filled(3), df_fq, scratch(), grad_scale=0.25)
    assert bits_equal(df_fq * 4, df_f), what
    if pipeline:
        # the one-call entry point falls back to the same launches: the same bits
        assert bits_equal(mom_f, mom) and bits_equal(loss_f, loss) and bits_equal(df_f, df), what
        # the partial sums by themselves (no reduce kernel): [n1 + n2][L * L] then [n1 + n2], summed here in float64
        (n1, n2), B1 = dispatch(B, L)[0], (B + 1) // 2
        s = scratch()
        H.evd_partial(f, Tf, mk, v, s)
        p = s.view(torch.float32)[:(n1 + n2) * (LL + 1)].double().cpu().numpy()
        part, part_op = p[:(n1 + n2) * LL].reshape(n1 + n2, LL), p[(n1 + n2) * LL:]
        lam1 = part[:n1].sum(0) / B1
        lam2 = part[n1:].sum(0) / (B - B1) if B > B1 else np.full(LL, np.nan)
        check_moments(lam1, lam2, part_op.sum() / B, c, what + " evd_partial")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,L,kind", list(PIPELINE))
def test_pipeline_shapes(B, L, kind):
    run_calls(B, L, kind, pipeline=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,L", list(FUSED))
def test_fused_shapes(B, L, kind):
    run_calls(B, L, kind, pipeline=False)


def test_refusals():
    """L = 129 is past MAXL: NSVD_EUNSUPPORTED from the three entry points, before any launch"""
    B, L = 8, 129
    f, Tf = torch.randn(B, L, device=DEV), torch.randn(B, L, device=DEV)
    mom = torch.zeros(2 * L * L + 1, device=DEV)
    s = H.evd_scratch(B, L, DEV)
    with pytest.raises(H.NsvdError, match="NSVD_EUNSUPPORTED"):
        H.evd_moments(f, Tf, H.MASK_SEQUENTIAL, None, moments=mom, scratch=s)
    with pytest.raises(H.NsvdError, match="NSVD_EUNSUPPORTED"):
        H.evd_partial(f, Tf, H.MASK_SEQUENTIAL, None, s)
    with pytest.raises(H.NsvdError, match="NSVD_EUNSUPPORTED"):
        H.evd_loss_grad(f, Tf, H.MASK_SEQUENTIAL, None, None, mom)
    torch.cuda.synchronize()
    assert float(mom.abs().sum()) == 0.0
