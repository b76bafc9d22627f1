"""The 3-D instances of eigfuncs.hip (nsvd_eigfunc3_eval, nsvd_eigfunc3_accumulate_f64: Hydrogen3D's states (n, l, m) at
x (B, 3)) and the callers above them (FusedTrainer.eigenfunction_accuracy, compute_spectrum_evd(ground_truth=...) with
operators.Hydrogen3D) against the float64 restatement tests/_eigfunc3d_oracle.py, itself held to the reference's values
by tests/test_eigfunc3d_oracle.py.

Shapes, from the dispatch code (one workgroup per ER = 64 rows; LDS 64 x (Lg doubles + L floats); Lg <= 80, L <= 64):
B in {1, 63, 64, 65, 127, 128, 129, 300} - one row, the neighbours of one and of two row tiles, five workgroups with a
last one of 44 rows - times (L, Lg) in {(1, 1), (3, 5), (14, 14), (16, 30), (64, 80)}: one output, L*L and Lg*L below the
256 threads of the output loops, three complete shells, Lg > L as L = 16 needs it (the n = 4 shell ends at 30), and the
largest tile (57,344 bytes of LDS, 80 functions: the n = 6 shell cut, which the entry point admits and the table builder
never asks for). Both importance modes; every case makes two calls into accumulators that start non-zero.

nsvd_eigfunc3_eval: deviation from the oracle relative to each function's maximum over the 300 points, planted rows
included (the origin, r = 1e-30 in three directions, both halves of the z axis, r = 120, the x and y axes). MEASURED on
an MI355X (worst over the functions, Z = 2): Lg = 14 7.2e-16, Lg = 55 1.8e-15. EVAL_BOUND is ten times the worst of them
(1.8e-14) and in no case above 1e-10: a float32 intermediate shows at 1e-7.

nsvd_eigfunc3_accumulate_f64: 1e-12 of each matrix's largest entry (float64 sums, order not fixed), the project's bound
for these sums (measured: 3.8e-15 at most over the 80 cases). phi is float32 arithmetic on a float32 weight whose expf
is the device's: the oracle is handed the device's weight, measured exactly (`device_weights`), so that nothing float32
is left between the two sides.
"""
import argparse

import numpy as np
import pytest
import torch

from tests import _eigfunc3d_oracle as EO3
from tests import _stream_contract as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
EVAL_BOUND = 1.8e-14
ACC_BOUND = 1e-12
SIGMA, LIM = 4.0, 10.0
Z = 2.0
H = E = OPS = LIB = KIND = None


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H, E, OPS, LIB, KIND
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import _lib, eigfuncs, hip_ops, operators
    H, E, OPS, LIB, KIND = hip_ops, eigfuncs, operators, _lib, _lib.GT_HYDROGEN3D
    yield


def points(B, seed):
    x = (4.0 * np.random.default_rng(seed).standard_normal((B, 3))).astype(np.float32)
    if B >= 16:
        tiny = np.float32(1e-30)
        x[0] = 0.0                                                   # the exact origin
        x[1] = (tiny, 0.0, 0.0)                                      # r = 1e-30: in the plane, on the axis, oblique
        x[2] = (0.0, 0.0, -tiny)
        x[3] = (-np.float32(6e-31), np.float32(8e-31), np.float32(1e-31))
        x[4:8] = [(0.0, 0.0, 0.5), (0.0, 0.0, 7.0), (0.0, 0.0, -0.5), (0.0, 0.0, -7.0)]   # both halves of the z axis
        x[8] = (0.0, 72.0, -96.0)                                    # r = 120
        x[9] = (120.0, 0.0, 0.0)
        x[10:14] = [(1.5, 0.0, 0.0), (-1.5, 0.0, 0.0), (0.0, 2.5, 0.0), (0.0, -2.5, 0.0)]  # the x and y axes
        x[14] = (1.0, -2.0, 0.0)                                     # the z = 0 plane
    return x


def worst(got, want):
    return float(np.max(np.max(np.abs(got - want), axis=0) / np.max(np.abs(want), axis=0)))


@pytest.mark.parametrize("Lg", [14, 55])
def test_eval_against_the_oracle(Lg):
    q = EO3.qnums(Lg)
    x = points(300, seed=Lg)
    want = EO3.evaluate(Z, q, x)
    got = H.eigfunc3_eval(KIND, Z, q, torch.tensor(x, device=DEV)).cpu().numpy()
    fig = worst(got, want)
    print(f"eigfunc3_eval Lg={Lg}: worst deviation / max {fig:.3e}")
    assert got.shape == (300, Lg) and np.isfinite(got).all()
    assert fig < EVAL_BOUND
    # the limit at the origin: finite for l = 0, exactly 0 otherwise; every m != 0 vanishes on the z axis
    assert all((got[0, i] != 0.0) == (l == 0) for i, (_, l, _) in enumerate(q))
    assert all(not got[4:8, i].any() for i, (_, _, m) in enumerate(q) if m != 0)
    assert all(got[4:8, i].all() for i, (n, l, m) in enumerate(q) if m == 0 and n == 1)


def device_weights(x, sigma, gaussian, lim):
    """w = sqrt(p_train) / sqrt(p_val) per row as the DEVICE forms it at D = 3, float32, exactly:
    nsvd_spectrum_accumulate_f64 on f = the identity (64 rows at a time) leaves cov_ii = w_i^2, a float32 squared in
    float64 - exact, and so is its root"""
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


CASES = [(1, 1), (3, 5), (14, 14), (16, 30), (64, 80)]


@pytest.mark.parametrize("gaussian", [0, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 127, 128, 129, 300])
@pytest.mark.parametrize("L,Lg", CASES)
def test_accumulate_against_the_oracle(L, Lg, B, gaussian):
    q = EO3.qnums(Lg)
    g = np.random.default_rng(1000 * B + 10 * L + gaussian)
    x = points(B, seed=B + Lg)
    fa, fb = (g.standard_normal((B, L)).astype(np.float32) for _ in range(2))
    xd = torch.tensor(x, device=DEV)
    w = device_weights(xd, SIGMA, bool(gaussian), LIM)
    w_np = EO3.weights32(x, SIGMA, LIM, bool(gaussian))
    # the measurement itself, against numpy's float32 formula: equal without importance; with it the float32 rounding
    # of an exponent of up to 87 in magnitude moves exp by 87 * 6e-8 = 5e-6 relative, its square root by half of that
    big = w_np > 1e-30  # (below: the float32 exp has underflowed on both sides)
    assert np.max(np.abs(w[big] - w_np[big]) / w_np[big]) < (1e-5 if gaussian else 1e-30)
    want = [a + b for a, b in zip(EO3.products(Z, q, fa, x, LIM, w), EO3.products(Z, q, fb, x, LIM, w))]
    start = [0.25 * np.max(np.abs(m)) * g.uniform(-1, 1, m.shape) for m in want]
    gram, cross, cov = (torch.tensor(s, dtype=F64, device=DEV) for s in start)
    cov_s, quad_s = cov.clone(), torch.zeros_like(cov)
    for f in (fa, fb):
        fd = torch.tensor(f, device=DEV)
        H.eigfunc3_accumulate(KIND, Z, q, fd, xd, SIGMA, bool(gaussian), LIM, gram, cross, cov)
        H.spectrum_accumulate(fd, fd, xd, SIGMA, bool(gaussian), LIM, cov_s, quad_s)
    got = [t.cpu().numpy() for t in (gram, cross, cov)]
    figs = [rel_max(a, s + b) for a, s, b in zip(got, start, want)]
    fig_s = rel_max(got[2], cov_s.cpu().numpy())
    print(f"eigfunc3_accumulate (L={L}, Lg={Lg}, B={B}, gauss={gaussian}): gram {figs[0]:.2e} cross {figs[1]:.2e} "
          f"cov {figs[2]:.2e}; cov against nsvd_spectrum_accumulate_f64 {fig_s:.2e}")
    assert all(np.isfinite(a).all() for a in got)
    assert max(figs) < ACC_BOUND, figs
    assert fig_s < ACC_BOUND, fig_s


def test_planted_rotation_and_planted_leak():
    """f = float32(psi_level @ Q) per level, L = 14 (three complete shells) on 300 points x = 4 N(0, I): every level's
    distance below 1e-9 (the float32 rounding of f, 6e-8, enters squared; the reference's functions give 2e-15 on the
    CPU). Column 4 replaced by the first state of the n = 3 shell: level 1 has lost one of its four directions to a
    function outside it - above 1e-2 (0.038 on the CPU on these points; not 1/4, the sample Gram is not the identity),
    while the other two levels stay put."""
    g = np.random.default_rng(5)
    x = (4 * g.standard_normal((300, 3))).astype(np.float32)
    t = E.ground_truth_table_3d(OPS.Hydrogen3D(1.0), 14)
    assert t.degeneracy == (0, 1, 5, 14)
    Psi = EO3.evaluate(1.0, t.qnums, x)
    Phi = np.empty_like(Psi)
    for lv, (s, e) in enumerate(zip(t.degeneracy[:-1], t.degeneracy[1:])):
        R, _ = np.linalg.qr(g.standard_normal((e - s, e - s)))
        Phi[:, s:e] = (0.5 + lv) * Psi[:, s:e] @ R
    leak = Phi.copy()
    leak[:, 4] = Psi[:, 5]
    xd = torch.tensor(x, device=DEV)
    dist = []
    for f in (Phi, leak):
        acc = E.Accumulator(t, 14, DEV)
        acc.add(torch.tensor(f.astype(np.float32), device=DEV), xd, 1.0, False, LIM)
        m = acc.metrics()
        assert m["levels"] == [(0, 1, 1), (1, 5, 4), (5, 14, 9)]
        dist.append(m["subspace_distance"])
    print("planted rotation:", dist[0], "planted leak:", dist[1])
    assert np.all(np.abs(dist[0]) < 1e-9)
    assert dist[1][1] > 1e-2 and abs(dist[1][0]) < 1e-9 and abs(dist[1][2]) < 1e-9


def test_refusals_write_nothing():
    lib = LIB.load()
    stream = torch.cuda.current_stream().cuda_stream
    B, L, Lg = 8, 4, 5
    g = torch.Generator().manual_seed(0)
    f, x = torch.randn(B, 65, generator=g).to(DEV), torch.randn(B, 3, generator=g).to(DEV)
    sentinel = 7.0
    gram, cross, cov, psi = (torch.full((81 * 81,), sentinel, dtype=F64, device=DEV) for _ in range(4))
    ptr = {"f": f.data_ptr(), "x": x.data_ptr(), "gram": gram.data_ptr(), "cross": cross.data_ptr(),
           "cov": cov.data_ptr()}

    def qarg(q, Lg):
        q = EO3.qnums(Lg) if q is None else q
        return H._qnums_arg(q, 3)[0]

    def acc(kind=None, param=1.0, q=None, Lg=Lg, L=L, imp=LIB.IMP_GAUSSIAN, null=(), lim=LIM):
        p = {k: (None if k in null else v) for k, v in ptr.items()}
        return lib.nsvd_eigfunc3_accumulate_f64(KIND if kind is None else kind, param,
                                                None if "qnums" in null else qarg(q, Lg), Lg, p["f"], L, p["x"], B,
                                                SIGMA, imp, lim, p["gram"], p["cross"], p["cov"], stream)

    def ev(kind=None, param=1.0, q=None, Lg=Lg, null=()):
        return lib.nsvd_eigfunc3_eval(KIND if kind is None else kind, param, None if "qnums" in null else qarg(q, Lg),
                                      Lg, None if "x" in null else ptr["x"], B,
                                      None if "psi" in null else psi.data_ptr(), stream)

    EINVAL, EUNSUP = LIB.EINVAL, LIB.EUNSUPPORTED
    assert acc(imp=LIB.IMP_UNIFORM) == EUNSUP
    assert [acc(imp=v) for v in (3, -1, 256)] == [EINVAL] * 3
    for kind in (LIB.GT_HYDROGEN2D, LIB.GT_HARMONIC2D, LIB.GT_WELL2D, 3, -1):  # the 2-D kinds and the unknown ones
        assert acc(kind=kind) == EINVAL and ev(kind=kind) == EINVAL, kind
    assert acc(Lg=81) == EUNSUP and ev(Lg=81) == EUNSUP
    assert acc(L=65) == EUNSUP
    assert acc(Lg=0) == EINVAL and acc(L=0) == EINVAL and ev(Lg=0) == EINVAL
    ok = [(1, 0, 0), (2, 0, 0), (2, 1, -1), (2, 1, 0)]
    for bad in ((0, 0, 0), (17, 0, 0), (2, 2, 0), (2, 1, 2), (2, 1, -2), (3, -1, 0)):
        assert acc(q=ok + [bad]) == EINVAL and ev(q=[bad] + ok) == EINVAL, bad
    assert acc(param=0.0) == EINVAL and acc(param=float("nan")) == EINVAL and ev(param=-1.0) == EINVAL
    assert acc(lim=0.0) == EINVAL
    for name in ("qnums", "f", "x", "gram", "cross"):
        assert acc(null=(name,)) == EINVAL, name
    for name in ("qnums", "x", "psi"):
        assert ev(null=(name,)) == EINVAL, name
    # and the 2-D entry points refuse the new kind
    pairs, _ = H._qnums_arg([(0, 0)] * Lg)
    assert lib.nsvd_eigfunc_eval(KIND, 1.0, pairs, Lg, ptr["x"], B, psi.data_ptr(), stream) == EINVAL
    assert lib.nsvd_eigfunc_accumulate_f64(KIND, 1.0, pairs, Lg, ptr["f"], L, ptr["x"], B, SIGMA, LIB.IMP_GAUSSIAN, LIM,
                                           ptr["gram"], ptr["cross"], ptr["cov"], stream) == EINVAL
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
    # the wrappers refuse a row width that does not belong to the entry point before anything is launched
    with pytest.raises(H.NsvdError):
        H.eigfunc3_eval(KIND, 1.0, EO3.qnums(5), x[:, :2].contiguous())
    with pytest.raises(H.NsvdError):
        H.eigfunc_eval(LIB.GT_HYDROGEN2D, 1.0, [(0, 0)], x)


def _stream_calls():
    """the two entry points as tests/_stream_contract.py's Call: the evaluation (five workgroups), and the accumulation
    with its accumulators as STATE, carried over the calls as the chunk loop carries them. B = 60 there: one workgroup, so
    that each output is one atomic on top of the carried value and the bits do not depend on an arrival order."""
    q = EO3.qnums(14)
    mk = lambda B, L: tuple(dict(x=torch.tensor(points(B, seed=s), device=DEV),  # noqa: E731
                                 f=torch.randn(B, L, generator=torch.Generator().manual_seed(s)).to(DEV))
                            for s in (101, 202))
    A, B_ = mk(300, 14)

    def run_eval(i, w, o, s):
        H.eigfunc3_eval(KIND, Z, q, i["x"], out=o["psi"])

    A2, B2 = mk(60, 14)

    def run_acc(i, w, o, s):
        H.eigfunc3_accumulate(KIND, Z, q, i["f"], i["x"], SIGMA, True, LIM, s["gram"], s["cross"], s["cov"])

    zeros = lambda: {k: torch.zeros(14, 14, dtype=F64, device=DEV) for k in ("gram", "cross", "cov")}  # noqa: E731
    return {"eval": SC.Call(run_eval, A, B_, lambda: ([], dict(psi=torch.empty(300, 14, dtype=F64, device=DEV)), {})),
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


CFG = dict(seed=3, ndim=3, n_particles=1, mlp_hidden_dims="16,16", nonlinearity="softplus", parallel=1,
           weight_normalization=0, use_fourier_feature=True, fourier_mapping_size=8, fourier_scale=0.5,
           fourier_deterministic=False, fourier_append_raw=False, apply_boundary=0, boundary_mode="dir_box_sqrt", lim=4.0,
           apply_exp_mask=1, exp_mask_init_scale=4.0, hard_mul_const=1.0, problem="sch", potential_type="hydrogen",
           charge=1.0, laplacian_eps=0.01, operator_scale=1.0, operator_shift=0.0, sampling_mode="gaussian",
           sampling_scale=2.0, batch_size=48, val_eps=1.0, optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0,
           num_iters=100, sort=0, hydrogen_mol_ion_R=1.0)


def _build(neigs):
    """the reference-style construction (main_pde.py) from this package's factories: seeded random weights"""
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    from neural_svd_amd.operators import get_dataloader, get_problem
    args = argparse.Namespace(**dict(CFG, neigs=neigs))
    args.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    args.adam_eps, args.use_lr_scheduler, args.ema_decay = 1e-7, True, 0.995
    args.print_freq, args.eval_freq, args.log_dir = 10 ** 9, 10 ** 9, None
    torch.manual_seed(CFG["seed"])
    operator, _ = get_problem(args, DEV)
    method = get_evd_method(args, "neuralsvd", get_wavefunctions(args)).to(DEV)
    _, val_data, _, imp_train, imp_val = get_dataloader(args, DEV)
    assert val_data is None and imp_val is None  # no validation grid above ndim 2, as the reference
    return args, operator, method, imp_train


@pytest.mark.parametrize("neigs", [5, 6])
def test_end_to_end_on_a_seeded_model(neigs):
    """a 3-D hydrogen model with seeded random weights (hidden 16, 16) on the lim = 4, val_eps = 1 grid (512 points,
    ragged against chunk = 200): the trainer's eigenfunction_accuracy and compute_spectrum_evd(ground_truth=...) against
    the oracle applied to operator_forward's f on the same grid; L = 5 has complete levels (Lg = 5), L = 6 a partial
    last one (Lg = 14, one learned column in the n = 3 shell). A 2-D ground truth on this model is refused."""
    from neural_svd_amd.drop_in import _fused_loop_trainer
    from neural_svd_amd.spectrum import compute_spectrum_evd
    args, operator, method, imp_train = _build(neigs)
    gt = OPS.ground_truth_of(args)
    assert isinstance(gt, OPS.Hydrogen3D)
    lim, val_eps, chunk = 4.0, 1.0, 200
    tr = _fused_loop_trainer(args, method, operator, imp_train, DEV)
    assert tr is not None and tr.shape.D == 3
    got = tr.eigenfunction_accuracy(gt, lim, val_eps, use_ema=False, chunk=chunk)
    ax = torch.from_numpy(np.arange(-lim, lim, val_eps))
    grid = torch.stack([g.reshape(-1) for g in torch.meshgrid(ax, ax, ax, indexing="xy")], dim=1).float().to(DEV)
    assert grid.shape == (512, 3)
    t = E.ground_truth_table_3d(gt, neigs)
    assert t.Lg == {5: 5, 6: 14}[neigs]
    psi, phi = [], []
    for i in range(0, len(grid), chunk):
        xb = grid[i:i + chunk]
        f, _ = H.operator_forward(tr.shape, tr._params, tr.problem, xb, H.new_workspace(tr.shape, len(xb), DEV), False,
                                  tr.path)
        a, b = EO3.weighted(t.param, t.qnums, f.cpu().numpy(), xb.cpu().numpy(), lim,
                            device_weights(xb, tr.problem.sigma, True, lim))
        psi.append(a)
        phi.append(b)
    psi, phi = np.concatenate(psi), np.concatenate(phi)
    n = len(grid)
    for k, m in (("gram", psi.T @ psi / n), ("cross", psi.T @ phi / n), ("cov", phi.T @ phi / n)):
        assert rel_max(got[k], m) < ACC_BOUND, k
    blocks = EO3.metrics(psi, phi, list(t.degeneracy))
    loader = lambda: ((grid[i:i + chunk], 0.0) for i in range(0, len(grid), chunk))  # noqa: E731
    same = compute_spectrum_evd(method, dataloader=loader(), operator=operator, importance_train=imp_train,
                                importance_val=OPS.UniformBoxImportance(lim, 3), device=DEV, ground_truth=gt)
    for name, m in (("trainer", got), ("compute_spectrum_evd", same["eigfunc_metrics"])):
        assert m["levels"] == blocks["levels"]
        assert m["qnums"] == t.qnums
        for k in ("subspace_distance", "angle", "procrustes_residual", "gram_defect"):
            got_k, want_k = np.asarray(m[k]), np.asarray(blocks[k])
            assert np.array_equal(np.isnan(got_k), np.isnan(want_k)), (name, k)
            d = np.nanmax(np.abs(got_k - want_k))
            print(f"L={neigs} {name} {k}: {got_k} (off the oracle by {d:.2e})")
            assert d < 1e-9, (name, k, d)
        for Qa, Qb in zip(m["rotation"], blocks["rotation"]):
            assert (Qa is None) == (Qb is None)
            if Qa is not None:
                d = np.max(np.abs(Qa - Qb))
                print(f"L={neigs} {name} rotation off the oracle by {d:.2e}")
                assert d < 1e-9, (name, d)
    # a ground truth of the other dimension is refused by name, on both routes, before anything is accumulated
    with pytest.raises(H.NsvdError, match="Hydrogen2D"):
        tr.eigenfunction_accuracy(OPS.Hydrogen2D(1.0), lim, val_eps, use_ema=False, chunk=chunk)
    with pytest.raises(H.NsvdError, match="2-D ground truth"):
        compute_spectrum_evd(method, dataloader=loader(), operator=operator, importance_train=imp_train,
                             importance_val=OPS.UniformBoxImportance(lim, 3), device=DEV, ground_truth=OPS.Hydrogen2D(1.0))
