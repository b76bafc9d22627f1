"""eigfuncs.hip (nsvd_eigfunc_eval, nsvd_eigfunc_accumulate_f64) and the callers above it (FusedTrainer.
eigenfunction_accuracy, compute_spectrum_evd(ground_truth=...)) against the float64 restatement tests/_eigfunc_oracle.py,
itself held to the reference's values by tests/test_eigfunc_oracle.py.

Shapes, from the dispatch code (one workgroup per ER = 64 rows; LDS 64 x (Lg doubles + L floats); Lg <= 80, L <= 64):
B in {1, 63, 64, 65, 127, 128, 129, 300} - one row, the neighbours of one and of two row tiles, five workgroups with a
last one of 44 rows - times (L, Lg) in {(1, 1), (3, 4), (16, 16), (32, 36), (64, 66)}: one output, L*L and Lg*L below the
256 threads of the output loops, the headline size, Lg > L as oscillator.sh needs it, and the largest tile (56,576 bytes
of LDS). Both importance modes; every case makes two calls into accumulators that start non-zero.

nsvd_eigfunc_eval: deviation from the oracle relative to each function's maximum over the 300 points, planted rows
included (the origin, r = 1e-30, r = 70, the four axes, the well's wall and the float32 next to it outside). MEASURED on
an MI355X (worst over the functions): hydrogen Lg = 16 / 64 (Z = 2) 1.3e-15 / 5.0e-15, oscillator Lg = 36 / 66 (k = 4)
2.0e-15 / 4.0e-15, well Lg = 9 (lim = 5) 1.4e-16. EVAL_BOUND is ten times the worst of them and in no case above
1e-10: a float32 intermediate shows at 1e-7.

nsvd_eigfunc_accumulate_f64: 1e-12 of each matrix's largest entry (float64 sums, order not fixed). phi is float32
arithmetic on a float32 weight whose expf is the device's: the oracle is handed the device's weight, measured exactly
(`device_weights`), so that nothing float32 is left between the two sides.
"""
import numpy as np
import pytest
import torch

from tests import _eigfunc_oracle as EO
from tests import _golden as G
from tests import _stream_contract as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
EVAL_BOUND = 5e-14
ACC_BOUND = 1e-12
SIGMA, LIM = 4.0, 10.0
H = E = OPS = LIB = None


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H, E, OPS, LIB
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import _lib, eigfuncs, hip_ops, operators
    H, E, OPS, LIB = hip_ops, eigfuncs, operators, _lib
    yield


def table(name, Lg):
    """(kind, param, the first Lg quantum numbers) - Z = 2, k = 4, lim = 5; Lg need not end on a level here"""
    if name == "hyd":
        return LIB.GT_HYDROGEN2D, 2.0, [tuple(q) for q in OPS.Hydrogen2D().get_qnums(Lg)]
    if name == "osc":
        return LIB.GT_HARMONIC2D, 4.0, [tuple(int(v) for v in q) for q in OPS.HarmonicOscillator().get_qnums(Lg)]
    return LIB.GT_WELL2D, 5.0, OPS.InfiniteWell2D(10.0).get_qnums(Lg)


def points(name, B, seed):
    g = np.random.default_rng(seed)
    if name == "well":
        x = g.uniform(-6.0, 6.0, (B, 2))
    else:
        x = {"hyd": 6.0, "osc": 1.5}[name] * g.standard_normal((B, 2))
    x = x.astype(np.float32)
    if B >= 16:
        x[0] = 0.0                                              # the exact origin
        x[1] = (np.float32(1e-30), 0.0)                         # r = 1e-30
        x[2] = (-np.float32(6e-31), np.float32(8e-31))
        x[3] = (42.0, -56.0)                                    # r = 70
        x[4:8] = [(1.5, 0.0), (-1.5, 0.0), (0.0, 2.5), (0.0, -2.5)]
        x[8] = (5.0, 1.0)                                       # the well's wall ...
        x[9] = (np.nextafter(np.float32(5.0), np.float32(9.0)), 1.0)   # ... and the float32 next to it outside
        x[10] = (-2.0, -5.0)
        x[11] = (-2.0, np.nextafter(np.float32(-5.0), np.float32(-9.0)))
    return x


def worst(got, want):
    return float(np.max(np.max(np.abs(got - want), axis=0) / np.max(np.abs(want), axis=0)))


@pytest.mark.parametrize("name,Lg", [("hyd", 16), ("hyd", 64), ("osc", 36), ("osc", 66), ("well", 9)])
def test_eval_against_the_oracle(name, Lg):
    kind, param, q = table(name, Lg)
    x = points(name, 300, seed=Lg)
    want = EO.evaluate(kind, param, q, x)
    got = H.eigfunc_eval(kind, param, q, torch.tensor(x, device=DEV)).cpu().numpy()
    fig = worst(got, want)
    print(f"eigfunc_eval {name} Lg={Lg}: worst deviation / max {fig:.3e}")
    assert got.shape == (300, Lg) and np.isfinite(got).all()
    assert fig < EVAL_BOUND
    if name == "hyd":  # the limit at the origin: finite for l = 0, exactly 0 otherwise
        assert all((got[0, i] != 0.0) == (l == 0) for i, (_, l) in enumerate(q))
    if name == "well":
        assert not got[9].any() and not got[11].any() and np.max(np.abs(got[8])) < 1e-15


def device_weights(x, sigma, gaussian, lim):
    """w = sqrt(p_train) / sqrt(p_val) per row as the DEVICE forms it, float32, exactly: nsvd_spectrum_accumulate_f64 on
    f = the identity (64 rows at a time) leaves cov_ii = w_i^2, a float32 squared in float64 - exact, and so is its root"""
    w = np.empty(len(x), np.float32)
    eye = torch.eye(64, device=DEV)
    for i in range(0, len(x), 64):
        xb = x[i:i + 64]
        n = len(xb)
        cov, quad = (torch.zeros(n, n, dtype=F64, device=DEV) for _ in range(2))
        f = eye[:n, :n].contiguous()
        H.spectrum_accumulate(f, f, xb, sigma, gaussian, lim, cov, quad)
        w[i:i + n] = torch.diag(cov).sqrt().cpu().numpy()
    return w


def rel_max(got, want):
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))


CASES = [("hyd", 1, 1), ("well", 3, 4), ("hyd", 16, 16), ("osc", 32, 36), ("osc", 64, 66)]


@pytest.mark.parametrize("gaussian", [0, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 127, 128, 129, 300])
@pytest.mark.parametrize("name,L,Lg", CASES)
def test_accumulate_against_the_oracle(name, L, Lg, B, gaussian):
    kind, param, q = table(name, Lg)
    g = np.random.default_rng(1000 * B + 10 * L + gaussian)
    x = points(name, B, seed=B + Lg)
    fa, fb = (g.standard_normal((B, L)).astype(np.float32) for _ in range(2))
    xd = torch.tensor(x, device=DEV)
    w = device_weights(xd, SIGMA, bool(gaussian), LIM)
    w_np = EO.weights32(x, SIGMA, LIM, bool(gaussian))
    # the measurement itself, against numpy's float32 formula: equal without importance; with it the float32 rounding
    # of an exponent of up to 87 in magnitude moves exp by 87 * 6e-8 = 5e-6 relative, its square root by half of that
    big = w_np > 1e-30  # (below: the float32 exp has underflowed on both sides)
    assert np.max(np.abs(w[big] - w_np[big]) / w_np[big]) < (1e-5 if gaussian else 1e-30)
    want = [a + b for a, b in zip(EO.products(kind, param, q, fa, x, LIM, w), EO.products(kind, param, q, fb, x, LIM, w))]
    start = [0.25 * np.max(np.abs(m)) * g.uniform(-1, 1, m.shape) for m in want]
    gram, cross, cov = (torch.tensor(s, dtype=F64, device=DEV) for s in start)
    cov_s, quad_s = cov.clone(), torch.zeros_like(cov)
    for f in (fa, fb):
        fd = torch.tensor(f, device=DEV)
        H.eigfunc_accumulate(kind, param, q, fd, xd, SIGMA, bool(gaussian), LIM, gram, cross, cov)
        H.spectrum_accumulate(fd, fd, xd, SIGMA, bool(gaussian), LIM, cov_s, quad_s)
    got = [t.cpu().numpy() for t in (gram, cross, cov)]
    figs = [rel_max(a, s + b) for a, s, b in zip(got, start, want)]
    fig_s = rel_max(got[2], cov_s.cpu().numpy())
    print(f"eigfunc_accumulate {name} (L={L}, Lg={Lg}, B={B}, gauss={gaussian}): gram {figs[0]:.2e} cross {figs[1]:.2e} "
          f"cov {figs[2]:.2e}; cov against nsvd_spectrum_accumulate_f64 {fig_s:.2e}")
    assert all(np.isfinite(a).all() for a in got)
    assert max(figs) < ACC_BOUND, figs
    assert fig_s < ACC_BOUND, fig_s


def test_accumulate_without_cov_and_with_non_finite_f():
    """cov = NULL: gram and cross as with it. f with a planted NaN and +-inf follows nan_to_num (NaN -> 0, +-inf ->
    +-FLT_MAX, float32 semantics); no importance and lim = 0.5, so the weight is exactly 1 and FLT_MAX stays finite"""
    kind, param, q = table("hyd", 16)
    B, L = 129, 5
    g = np.random.default_rng(11)
    x = points("hyd", B, seed=3)
    f = g.standard_normal((B, L)).astype(np.float32)
    f[3, 1] = f[128, 4] = np.nan
    f[9, 0] = f[100, 2] = np.inf
    f[10, 0] = f[128, 2] = -np.inf
    xd, fd = torch.tensor(x, device=DEV), torch.tensor(f, device=DEV)
    w = EO.weights32(x, 1.0, 0.5, False)
    assert float(w[0]) == 1.0
    want = EO.products(kind, param, q, f, x, 0.5, w)
    assert all(np.isfinite(m).all() for m in want)
    gram, cross, cov = (torch.zeros(s, dtype=F64, device=DEV) for s in ((16, 16), (16, L), (L, L)))
    H.eigfunc_accumulate(kind, param, q, fd, xd, 1.0, False, 0.5, gram, cross, cov)
    gram2, cross2 = torch.zeros_like(gram), torch.zeros_like(cross)
    H.eigfunc_accumulate(kind, param, q, fd, xd, 1.0, False, 0.5, gram2, cross2, None)
    got = [t.cpu().numpy() for t in (gram, cross, cov, gram2, cross2)]
    assert all(np.isfinite(a).all() for a in got)
    figs = [rel_max(a, b) for a, b in zip(got, list(want) + list(want[:2]))]
    print("eigfunc_accumulate non-finite f / cov = NULL:", figs)
    assert max(figs) < ACC_BOUND, figs


def test_refusals_write_nothing():
    lib = LIB.load()
    stream = torch.cuda.current_stream().cuda_stream
    B, L, Lg = 8, 4, 4
    g = torch.Generator().manual_seed(0)
    f, x = torch.randn(B, 65, generator=g).to(DEV), torch.randn(B, 2, generator=g).to(DEV)
    sentinel = 7.0
    gram, cross, cov, psi = (torch.full((81 * 81,), sentinel, dtype=F64, device=DEV) for _ in range(4))
    ptr = {"f": f.data_ptr(), "x": x.data_ptr(), "gram": gram.data_ptr(), "cross": cross.data_ptr(),
           "cov": cov.data_ptr()}

    def acc(kind=LIB.GT_HYDROGEN2D, param=1.0, q=None, Lg=Lg, L=L, imp=LIB.IMP_GAUSSIAN, null=(), lim=LIM):
        q = OPS.Hydrogen2D().get_qnums(Lg) if q is None else q
        arr, _ = H._qnums_arg(q)
        p = {k: (None if k in null else v) for k, v in ptr.items()}
        return lib.nsvd_eigfunc_accumulate_f64(kind, param, None if "qnums" in null else arr, Lg, p["f"], L, p["x"], B,
                                               SIGMA, imp, lim, p["gram"], p["cross"], p["cov"], stream)

    def ev(kind=LIB.GT_HYDROGEN2D, param=1.0, q=None, Lg=Lg, null=()):
        q = OPS.Hydrogen2D().get_qnums(Lg) if q is None else q
        arr, _ = H._qnums_arg(q)
        return lib.nsvd_eigfunc_eval(kind, param, None if "qnums" in null else arr, Lg, None if "x" in null else ptr["x"],
                                     B, None if "psi" in null else psi.data_ptr(), stream)

    EINVAL, EUNSUP = LIB.EINVAL, LIB.EUNSUPPORTED
    assert acc(imp=LIB.IMP_UNIFORM) == EUNSUP
    assert [acc(imp=v) for v in (3, -1, 256)] == [EINVAL] * 3
    assert acc(kind=3) == EINVAL and acc(kind=-1) == EINVAL and ev(kind=3) == EINVAL
    assert acc(Lg=81) == EUNSUP and ev(Lg=81) == EUNSUP
    assert acc(L=65) == EUNSUP
    assert acc(Lg=0) == EINVAL and acc(L=0) == EINVAL and ev(Lg=0) == EINVAL
    assert acc(q=[(0, 0), (1, 2), (1, 0), (1, 1)]) == EINVAL and ev(q=[(0, 0), (1, -2), (1, 0), (1, 1)]) == EINVAL
    assert acc(kind=LIB.GT_WELL2D, param=5.0, q=[(1, 1), (0, 1), (1, 2), (2, 2)]) == EINVAL
    assert ev(kind=LIB.GT_WELL2D, param=5.0, q=[(1, 1), (2, 1), (1, 0), (2, 2)]) == EINVAL
    assert acc(kind=LIB.GT_HARMONIC2D, q=[(0, 0), (-1, 0), (0, 1), (1, 1)]) == EINVAL
    assert acc(param=0.0) == EINVAL and acc(param=float("nan")) == EINVAL and ev(param=-1.0) == EINVAL
    assert acc(lim=0.0) == EINVAL
    for name in ("qnums", "f", "x", "gram", "cross"):
        assert acc(null=(name,)) == EINVAL, name
    for name in ("qnums", "x", "psi"):
        assert ev(null=(name,)) == EINVAL, name
    torch.cuda.synchronize()
    for t in (gram, cross, cov, psi):
        assert bool((t == sentinel).all())
    # and the valid call behind all of them runs: cov may be NULL, the others are written
    assert acc(null=("cov",)) == 0 and ev() == 0
    torch.cuda.synchronize()
    assert bool((cov == sentinel).all())
    assert not bool((gram[:Lg * Lg] == sentinel).any()) and bool((gram[Lg * Lg:] == sentinel).all())
    assert not bool((cross[:Lg * L] == sentinel).any()) and bool((cross[Lg * L:] == sentinel).all())
    assert not bool((psi[:B * Lg] == sentinel).any()) and bool((psi[B * Lg:] == sentinel).all())


def _stream_calls():
    """the two entry points as tests/_stream_contract.py's Call: the evaluation (five workgroups), and the accumulation
    with its accumulators as STATE, carried over the calls as the chunk loop carries them. B = 60 there: one workgroup, so
    that each output is one atomic on top of the carried value and the bits do not depend on an arrival order."""
    kind, param, q = table("hyd", 16)
    mk = lambda B, L: tuple(dict(x=torch.tensor(points("hyd", B, seed=s), device=DEV),  # noqa: E731
                                 f=torch.randn(B, L, generator=torch.Generator().manual_seed(s)).to(DEV))
                            for s in (101, 202))
    A, B_ = mk(300, 16)

    def run_eval(i, w, o, s):
        H.eigfunc_eval(kind, param, q, i["x"], out=o["psi"])

    A2, B2 = mk(60, 16)

    def run_acc(i, w, o, s):
        H.eigfunc_accumulate(kind, param, q, i["f"], i["x"], SIGMA, True, LIM, s["gram"], s["cross"], s["cov"])

    zeros = lambda: {k: torch.zeros(16, 16, dtype=F64, device=DEV) for k in ("gram", "cross", "cov")}  # noqa: E731
    return {"eval": SC.Call(run_eval, A, B_, lambda: ([], dict(psi=torch.empty(300, 16, dtype=F64, device=DEV)), {})),
            "accumulate": SC.Call(run_acc, A2, B2, lambda: ([], {}, zeros()))}


@pytest.fixture(scope="module")
def chain():
    return SC.DelayChain()


@pytest.mark.parametrize("which", ["eval", "accumulate"])
def test_side_stream_and_graph_capture(which, chain):
    """no allocation, no copy, no synchronisation: the table travels in the launch arguments, so the call is legal on a
    side stream behind a pending producer and inside a capture, and gives the eager call's bits"""
    call = _stream_calls()[which]
    want = SC.eager(call, [call.A, call.B, call.B])
    SC.check_side_stream(call, want[0], chain)
    SC.check_capture(call, want)


def _grid(lim, val_eps):
    ax = torch.from_numpy(np.arange(-lim, lim, val_eps))
    return torch.stack([g.reshape(-1) for g in torch.meshgrid(ax, ax, indexing="xy")], dim=1).float().to(DEV)


@pytest.mark.parametrize("case", ["hyd_small", "osc_small"])
def test_end_to_end_on_golden_weights(case):
    """model_small's weights on the lim = 5, val_eps = 0.25 grid (1600 points, ragged against chunk = 512): the trainer's
    eigenfunction_accuracy and compute_spectrum_evd(ground_truth=...) against the oracle applied to operator_forward's f
    on the same grid; hyd_small has complete levels (L = 4), osc_small a partial last one (L = 5, Lg = 6)"""
    from neural_svd_amd.drop_in import _fused_loop_trainer
    from neural_svd_amd.spectrum import compute_spectrum_evd
    from tests.test_dropin_gpu import build
    z = G.load("model_small")
    cfg, args, operator, _, method, (_, _, _, imp_train, imp_val) = build(case, z)
    gt = OPS.ground_truth_of(args)
    lim, val_eps, chunk = 5.0, 0.25, 512
    tr = _fused_loop_trainer(args, method, operator, imp_train, DEV)
    assert tr is not None
    got = tr.eigenfunction_accuracy(gt, lim, val_eps, use_ema=False, chunk=chunk)
    # the oracle on the same f, chunk by chunk as the trainer forwards it
    grid = _grid(lim, val_eps)
    assert grid.shape == (1600, 2)
    t = E.ground_truth_table(gt, cfg["neigs"])
    psi, phi = [], []
    for i in range(0, len(grid), chunk):
        xb = grid[i:i + chunk]
        f, _ = H.operator_forward(tr.shape, tr._params, tr.problem, xb, H.new_workspace(tr.shape, len(xb), DEV), False,
                                  tr.path)
        a, b = EO.weighted(t.kind, t.param, t.qnums, f.cpu().numpy(), xb.cpu().numpy(), lim,
                           device_weights(xb, tr.problem.sigma, True, lim))
        psi.append(a)
        phi.append(b)
    psi, phi = np.concatenate(psi), np.concatenate(phi)
    n = len(grid)
    for k, m in (("gram", psi.T @ psi / n), ("cross", psi.T @ phi / n), ("cov", phi.T @ phi / n)):
        assert rel_max(got[k], m) < ACC_BOUND, k
    blocks = EO.metrics(psi, phi, list(t.degeneracy))
    same = compute_spectrum_evd(method, dataloader=((grid[i:i + chunk], 0.0) for i in range(0, len(grid), chunk)),
                                operator=operator, importance_train=imp_train,
                                importance_val=OPS.UniformBoxImportance(lim, 2), device=DEV, ground_truth=gt)
    plain = compute_spectrum_evd(method, dataloader=((grid[i:i + chunk], 0.0) for i in range(0, len(grid), chunk)),
                                 operator=operator, importance_train=imp_train,
                                 importance_val=OPS.UniformBoxImportance(lim, 2), device=DEV)
    assert sorted(plain) == ["cov", "eigfuncs", "eigvals", "norms", "quad"]
    assert sorted(same) == sorted(list(plain) + ["eigfunc_metrics"])
    for name, m in (("trainer", got), ("compute_spectrum_evd", same["eigfunc_metrics"])):
        assert m["levels"] == blocks["levels"]
        for k in ("subspace_distance", "angle", "procrustes_residual", "gram_defect"):
            got_k, want_k = np.asarray(m[k]), np.asarray(blocks[k])
            assert np.array_equal(np.isnan(got_k), np.isnan(want_k)), (name, k)
            d = np.nanmax(np.abs(got_k - want_k))
            print(f"{case} {name} {k}: {got_k} (off the oracle by {d:.2e})")
            assert d < 1e-9, (name, k, d)
        for Qa, Qb in zip(m["rotation"], blocks["rotation"]):
            assert (Qa is None) == (Qb is None)
            if Qa is not None:
                d = np.max(np.abs(Qa - Qb))
                print(f"{case} {name} rotation off the oracle by {d:.2e}")
                assert d < 1e-9, (name, d)


def test_drop_in_loop_adds_the_level_distances_only_when_asked():
    """train_operator with args.eigfunc_metrics: the evaluation also measures the functions and the log rows after it
    carry one distance per level; without the switch the rows have the reference's four keys and nothing else"""
    from neural_svd_amd.drop_in import train_operator
    from tests.test_dropin_gpu import build

    class Rows:
        def __init__(self):
            self.rows = []

        def writerow(self, row):
            self.rows.append(row)

    z = G.load("model_small")
    rows = {}
    for flag in (False, True):
        _, args, operator, gt, method, (make_batch, val_data, batch_ftn_val, imp_train, imp_val) = build("hyd_small", z)
        args.num_iters, args.print_freq, args.eval_freq = 4, 2, 2
        if flag:
            args.eigfunc_metrics = True
        w = Rows()
        train_operator(args, method, operator, make_batch, val_data, batch_ftn_val, w, None, DEV, imp_train, imp_val, gt)
        rows[flag] = w.rows
    four = {"iter", "train_loss", "avg_train_loss", "time"}
    assert [set(r) for r in rows[False]] == [four, four]
    assert set(rows[True][0]) == four  # printed at step 2, before the first evaluation
    extra = {k: v for k, v in rows[True][1].items() if k not in four}
    assert sorted(extra) == ["eigfunc_dist_level0", "eigfunc_dist_level1"]  # L = 4: the n = 0 and n = 1 levels
    assert all(0.0 <= v <= 1.0 + 1e-12 for v in extra.values())
