"""NSVD_PATH_GENERIC_EXACT on the GPU: the exact Laplacian (laplacian_eps <= 0) on the generic kernels' forward-mode
jets, for any hidden width and 1 <= D <= 12, against float64.

  * the two kernels of csrc/generic_jets.hip alone against float64 torch, 1e-6 max-normalised per block;
  * operator forward + backward against tests/_exact_nd_oracle.py (double autograd of the float64 model) with the oracle's
    d loss / d f: f 2e-5, Tf 1e-4, every gradient 3e-5 - the bounds of test_exact_mode_three_dimensional. A bound becomes
    max(bound, 4 x the error of torch's float32 evaluation of the same quantity against float64), the project's yardstick
    rule, computed here from the oracle alone and printed; on an MI355X every case met the plain bounds (measured: f at
    most 3.7e-7, Tf at most 3.9e-7, gradients at most 2.2e-7);
  * the reference's own exact mode (tests/golden/exact_nd.npz): Tf within max(2e-5, 3 x its float32 run), as
    test_exact_laplacian_mode;
  * the MFMA jets (PATH_FUSED) and these jets agree on 128-wide models within twice those bounds;
  * FusedTrainer(path=PATH_GENERIC_EXACT): three steps against the oracle's trajectory, host and device sampler, equal
    bits from equal seeds, the spectrum evaluation; NestedLoRA(path=...) through the autograd Function and one
    compute_spectrum_evd pass, built by get_problem / get_evd_method under args.generic_exact_laplacian;
  * workspace hygiene and the refusals.
Every batch keeps 0.1 from each nucleus, coalescence point, wall and (where the operator is singular there) the origin,
by construction; the tests assert it and leave no row out."""
import dataclasses
import types

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _exact_nd_oracle as XO
from tests import _highdim_oracle as HO
from tests import test_box_gpu as TB
from tests import test_generic_exact_oracle as TXO
from tests import test_highdim_gpu as THG
from tests import test_highdim_oracle as THO

pytestmark = pytest.mark.gpu

H = None
DEV = "cuda:0"
rel, to_dev = TB.rel, TB.to_dev
PI32 = float(np.float32(np.pi))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import hip_ops
    H = hip_ops
    TB.H = hip_ops
    THG.H = hip_ops
    yield


def maxnorm_blocks(got, want, B):
    """worst max-normalised error over the column blocks of B samples"""
    got, want = got.double().cpu(), want.double()
    worst = 0.0
    for e in range(want.shape[1] // B):
        g, w = got[:, e * B:(e + 1) * B], want[:, e * B:(e + 1) * B]
        worst = max(worst, float((g - w).abs().max() / w.abs().max().clamp_min(1e-300)))
    return worst


# ---------------------------------------------------------------------------- 1. the two kernels alone
@pytest.mark.parametrize("B", (37, 64))
@pytest.mark.parametrize("m", (8, 64))
@pytest.mark.parametrize("D", (1, 2, 5, 12))
def test_fourier_jets_kernel(D, m, B):
    g = torch.Generator().manual_seed(100 * D + m + B)
    x = (3.0 * torch.randn(B, D, generator=g)).float()
    fB = (2 * np.pi * 0.3 * torch.randn(D, m, generator=g)).float()
    got = H.fourier_features_jets(x.to(DEV), fB.to(DEV).contiguous())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2 * m, (D + 2) * B) and bool(torch.isfinite(got).all())
    e = maxnorm_blocks(got, XO.fourier_jets(x.double(), fB.double()), B)
    print(f"fourier jets D={D} m={m} B={B}: {e:.2e}")
    assert e < 1e-6, e


@pytest.mark.parametrize("D", (1, 5, 12))
@pytest.mark.parametrize("B", (37, 64, 65))  # scalar, vector, scalar instance; ragged last workgroup in each
@pytest.mark.parametrize("rows", (3, 48))
def test_softplus_jets_kernel(rows, B, D):
    g = torch.Generator().manual_seed(7 * rows + B + D)
    z = torch.randn(rows, (D + 2) * B, generator=g).float()
    z[:, :B] = 60.0 * torch.rand(rows, B, generator=g) - 30.0  # pre-activations in (-30, 30): both softplus branches
    z[0, 0], z[0, 1], z[-1, B - 1] = 20.0, 20.5, -29.5           # at and just above torch's threshold
    assert bool((z[:, :B] > 20).any()) and bool((z[:, :B] < -20).any())
    margin = 64
    buf = torch.full((rows * (D + 2) * B + 2 * margin,), 777.0, device=DEV)
    zd = buf[margin:-margin].view(rows, (D + 2) * B)
    zd.copy_(z)
    H.softplus_jets_inplace(zd, B, D)
    torch.cuda.synchronize()
    assert bool((buf[:margin] == 777.0).all()) and bool((buf[-margin:] == 777.0).all())
    e = maxnorm_blocks(zd, XO.softplus_jets(z.double(), B, D), B)
    print(f"softplus jets rows={rows} B={B} D={D}: {e:.2e}")
    assert e < 1e-6, e


# ---------------------------------------------------------------------------- 2. operator forward + backward
def _prob(kind, D, **kw):
    G, U, N = HO.IMP_GAUSSIAN, HO.IMP_UNIFORM, HO.IMP_NONE
    com = dict(eps=0.0, op_scale=1.5, op_shift=0.5, hard_mul_const=0.9)
    com.update(kw)
    if kind == "harmonic":
        return HO.Problem(potential=O.POT_HARMONIC, charge_or_k=0.5, sigma=3.0, importance=G, **com)
    if kind == "harmonic_none":
        return HO.Problem(potential=O.POT_HARMONIC, charge_or_k=0.5, sigma=1.0, importance=N, **com)
    if kind == "hydrogen":
        return HO.Problem(potential=O.POT_HYDROGEN, charge_or_k=1.0, sigma=3.0, importance=G, **com)
    if kind == "cosine_uniform":
        return HO.Problem(potential=HO.POT_COSINE, pot_coef=tuple(0.1 + 0.07 * d for d in range(D)), sigma=PI32,
                          importance=U, **com)
    if kind == "h2":
        return dataclasses.replace(TXO._molecule("H2", D // 2), op_shift=0.5)
    raise KeyError(kind)


SQRT, EXP = dict(box_mode=BO.BOX_SQRT, box_lim=4.0), dict(box_mode=BO.BOX_EXP, box_lim=4.0)
# id: (D, hidden, L, B, m, problem, exponential mask scale or None). On each side of the D = 4 | 5 boundary (nsvd_fd_exact
# | the direction loop): harmonic + exponential mask, hydrogen, cosine + uniform, a molecule, both box modes.
OPERATOR_CASES = {
    "D1_w50_harmonic_mask": (1, (50,), 3, 37, 33, _prob("harmonic", 1), 4.0),
    "D2_w64x3_L17_hydrogen_boxsqrt": (2, (64, 64, 64), 17, 64, 64, _prob("hydrogen", 2, **SQRT), None),
    "D3_w40_24_cosine_uniform_boxexp": (3, (40, 24), 3, 65, 34, _prob("cosine_uniform", 3, **EXP), None),
    "D4_w16_h2_2d_mask": (4, (16, 16), 3, 64, 8, _prob("h2", 4), 4.0),
    "D2_8layers_harmonic_none_mask": (2, (24,) * 7, 2, 64, 16, _prob("harmonic_none", 2), 5.0),
    "D5_w16_L17_cosine_uniform": (5, (16, 16), 17, 65, 8, _prob("cosine_uniform", 5), None),
    "D5_w16_L17_harmonic_mask_boxsqrt": (5, (16, 16), 17, 65, 8, _prob("harmonic", 5, **SQRT), 4.0),
    "D6_w16_h2_3d_mask": (6, (16, 16), 3, 64, 8, _prob("h2", 6), 4.0),
    "D12_w16_hydrogen_boxexp": (12, (16, 16), 3, 64, 8, _prob("hydrogen", 12, **EXP), None),
    "D12_w16_harmonic_none_mask": (12, (16, 16), 3, 64, 8, _prob("harmonic_none", 12), 5.0),
}


def _case(name):
    D, hidden, L, B, m, prob, mask = OPERATOR_CASES[name]
    seed = 1 + sorted(OPERATOR_CASES).index(name)
    p = O.init_params(L, D, m, hidden, 0.2, exp_mask_init=mask, seed=seed)
    g = torch.Generator().manual_seed(seed)
    p.bs = [0.1 * torch.randn(b.shape, generator=g) for b in p.bs]  # (biases off zero: they join the value stream only)
    if p.scales is not None:
        p.scales = p.scales * (1.0 + 0.1 * torch.arange(L))
    x = XO.clear_batch(B, D, 3.5, p.scales, prob, seed)
    return p, prob, x


_REF = {}


def _reference(name):
    """the float64 oracle and torch's float32 evaluation of the same quantities, once per case"""
    if name not in _REF:
        p, prob, x = _case(name)
        L = p.ws[0].shape[0]
        v, M = O.sequential_nesting_masks(L)
        ref = XO.loss_and_grads(x, p.to(torch.float64), prob, v, M)
        c32 = HO.operator_forward(x.float(), p.to(torch.float32), prob)
        g32 = O.operator_backward(c32, p.to(torch.float32), prob, ref["df"].float())
        y = dict(f=rel(c32.f, ref["f"]), Tf=rel(c32.Tf, ref["Tf"]),
                 grads=[rel(a.reshape(-1), b.reshape(-1)) for a, b in zip(g32, ref["grads"])])
        _REF[name] = (p, prob, x, v, M, ref, y)
    return _REF[name]


@pytest.mark.parametrize("name", list(OPERATOR_CASES))
def test_operator_forward_backward_against_the_oracle(name):
    p, prob, x, v, M, ref, y = _reference(name)
    assert float(XO.clearance(x, p.scales, prob).min()) > 0.1  # no row is near a singular point, none is left out
    D = x.shape[1]
    shape = THG.shape_of(p, prob)
    assert H.path_name(shape, x.shape[0], H.PATH_GENERIC_EXACT, THG.hip_problem(prob, D)) == "generic_exact"
    r = THG.run_hip(p, prob, x, v, M, H.PATH_GENERIC_EXACT, df_override=ref["df"])
    bf, bT = max(2e-5, 4 * y["f"]), max(1e-4, 4 * y["Tf"])
    ef, eT = rel(r["f"], ref["f"]), rel(r["Tf"], ref["Tf"])
    eg = [rel(a.view(-1), b.reshape(-1)) for a, b in zip(r["grads"], ref["grads"])]
    print(f"{name}: f {ef:.2e} (float32 torch {y['f']:.2e}) Tf {eT:.2e} ({y['Tf']:.2e}) "
          f"grads max {max(eg):.2e} ({max(y['grads']):.2e})")
    assert bool(torch.isfinite(r["f"]).all()) and bool(torch.isfinite(r["Tf"]).all())
    assert ef < bf, (ef, bf)
    assert eT < bT, (eT, bT)
    for i, (e, e32) in enumerate(zip(eg, y["grads"])):
        assert torch.isfinite(r["grads"][i]).all() and e < max(3e-5, 4 * e32), (i, e, e32)


# ---------------------------------------------------------------------------- 3. the reference's exact mode
@pytest.mark.parametrize("name", TXO.GOLDEN_CASES)
def test_golden_cases(name):
    z = np.load(TXO.GOLDEN)
    cfg, names, p, prob = THO.case_setup(z, name, dtype=torch.float32)
    x = torch.tensor(z[f"{name}_x"][0])
    assert float(XO.clearance(x, p.scales, prob).min()) > 0.1
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    pre = f"{name}_f64_step0_"
    ref = XO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
    r = THG.run_hip(p, prob, x, v, M, H.PATH_GENERIC_EXACT, df_override=ref["df"])
    assert r["path"] == "generic_exact"
    ref32 = rel(z[f"{name}_f32_step0_Tf"], z[pre + "Tf"])
    eT = rel(r["Tf"], z[pre + "Tf"])
    print(f"{name}: f {rel(r['f'], z[pre + 'f']):.2e} Tf {eT:.2e} (the reference's float32 run {ref32:.2e})")
    assert rel(r["f"], z[pre + "f"]) < 2e-5
    assert eT < max(2e-5, 3 * ref32), (eT, ref32)
    for n, g in zip(names, r["grads"]):  # gradients given the same d loss / d f
        assert rel(g.view(-1), ref["grads"][names.index(n)].reshape(-1)) < 3e-5, n
    r2 = THG.run_hip(p, prob, x, v, M, H.PATH_GENERIC_EXACT)  # end to end, against the reference's loss and gradients
    assert abs(float(r2["loss"][0]) - float(z[pre + "loss"])) <= 1e-4 * abs(float(z[pre + "loss"]))
    for n, g in zip(names, r2["grads"]):
        assert rel(g.view(-1), z[pre + "grad_" + n].reshape(-1)) < 1e-4, n


# ---------------------------------------------------------------------------- 4. two implementations of the jets
@pytest.mark.parametrize("D", (2, 3))
def test_generic_jets_agree_with_the_mfma_jets(D):
    L, m, hidden, B = 2, 64, (128, 128, 128), 64
    p = O.init_params(L, D, m, hidden, 0.2, exp_mask_init=4.0, seed=33 + D)
    prob = HO.Problem(potential=O.POT_HYDROGEN, eps=0.0, op_scale=10.0, op_shift=1.0, sigma=3.0, hard_mul_const=0.9)
    x = XO.clear_batch(B, D, 4.0, p.scales, prob, 8 + D)
    assert float(XO.clearance(x, p.scales, prob).min()) > 0.1
    v, M = O.sequential_nesting_masks(L)
    ref = XO.loss_and_grads(x, p.to(torch.float64), prob, v, M)
    a = THG.run_hip(p, prob, x, v, M, H.PATH_FUSED, df_override=ref["df"])
    b = THG.run_hip(p, prob, x, v, M, H.PATH_GENERIC_EXACT, df_override=ref["df"])
    assert a["path"] == "fused_mfma" and b["path"] == "generic_exact"
    assert rel(b["f"], a["f"].double().cpu()) < 2 * 2e-5
    assert rel(b["Tf"], a["Tf"].double().cpu()) < 2 * 1e-4
    for i, (ga, gb) in enumerate(zip(a["grads"], b["grads"])):
        assert rel(gb.view(-1), ga.view(-1).double().cpu()) < 2 * 3e-5, i
    assert rel(b["f"], ref["f"]) < 2e-5 and rel(b["Tf"], ref["Tf"]) < 1e-4


# ---------------------------------------------------------------------------- 5. FusedTrainer on this path
TRAINER_CASES = {"D2_w64x3": (2, (64, 64, 64), 4, 64, 64), "D5_w16": (5, (16, 16), 3, 64, 8)}


def _trainer(case, device_sampler, seed=0, T=10):
    from neural_svd_amd.trainer import FusedTrainer
    D, hidden, L, B, m = TRAINER_CASES[case]
    shape = H.ModelShape(L=L, D=D, m=m, hidden=hidden, has_exp_mask=True)
    prob = H.make_problem(H.POT_HARMONIC, 0.5, 0.0, 1.0, 4.0, 2.0)
    tr = FusedTrainer(shape, prob, B, sequential=False, lr=1e-3, num_iters=T, seed=seed, device=DEV,
                      sampling_scale=2.0, fourier_scale=0.2, exp_mask_init=4.0, path=H.PATH_GENERIC_EXACT,
                      device_sampler=device_sampler, sample_seed=11)
    return tr, O.Problem(potential=O.POT_HARMONIC, charge_or_k=0.5, eps=0.0, op_scale=1.0, op_shift=4.0, sigma=2.0)


@pytest.mark.parametrize("device_sampler", (True, False), ids=("device_sampler", "host_sampler"))
@pytest.mark.parametrize("case", list(TRAINER_CASES))
def test_trainer_three_steps_against_the_oracle(case, device_sampler):
    """test_three_step_trajectory_at_the_headline_shape_against_the_oracle's procedure and bounds (square averages 2e-4,
    updates of the strongly graded elements 2e-3, the EMA recurrence 1e-6, the shadow against the oracle's 2e-3 of the
    update): every step checked against the float64 oracle (exact mode) re-started from the trainer's own state; all
    heads, all rows. The update and shadow bounds follow the yardstick rule, max(bound, 4 x torch's float32 evaluation of
    the same step against float64), computed from the oracle alone: only the mask scales need it."""
    D, hidden, L, B, m = TRAINER_CASES[case]
    T = 10
    tr, prob_o = _trainer(case, device_sampler, T=T)
    assert tr.fused_step and tr.keep_grads and not tr.guest_features and not tr.direct_moments
    v, M = O.joint_nesting_masks(L, 1)
    v, M = v.double(), M.double()
    nl = len(hidden) + 1
    nt = 2 * nl + 1
    for t in range(3):
        before = {k: [u.clone() for u in tr.P.views(getattr(tr.P, k))] for k in ("flat", "sq", "ema")}
        tr.step()
        torch.cuda.synchronize()
        x, f64, Tf64 = tr.x.double().cpu(), tr.f.double().cpu(), tr.Tf.double().cpu()
        loss64, lam1, lam2, _, _ = O.evd_loss_forward(f64, Tf64, v, M)
        assert abs(float(tr.loss[0]) - float(loss64)) < 2e-5 * float(tr.loss[1:].abs().max())
        df64 = O.evd_loss_backward(f64, Tf64, v, M, lam1, lam2)
        lr = O.cosine_lr(1e-3, t, T)
        after = {k: tr.P.views(getattr(tr.P, k)) for k in ("flat", "sq", "ema")}
        cpu = lambda ts: [u.double().cpu() for u in ts]  # noqa: E731
        b_flat, b_sq, b_ema = cpu(before["flat"]), cpu(before["sq"]), cpu(before["ema"])
        ph = O.Params(b_flat[:nl], b_flat[nl:2 * nl], tr.P.fourier_B.double().cpu(), b_flat[2 * nl])
        c = O.operator_forward(x, ph, prob_o)
        assert rel(tr.f, c.f) < 2e-5 and rel(tr.Tf, c.Tf) < 1e-4
        g = O.operator_backward(c, ph, prob_o, df64)
        ps = [q.clone() for q in ph.trainable()]
        p0 = [q.clone() for q in ps]
        sq, sh = [q.clone() for q in b_sq], [q.clone() for q in b_ema]
        O.rmsprop_step(ps, g, sq, lr, alpha=0.999, eps=1e-10)
        assert O.ema_update(sh, ps, 0.995, t) == t + 1
        # the yardstick: torch's float32 evaluation of the same optimiser step from the same float32 state and the
        # oracle's gradient (rounded to float32) - what float32 storage of parameter and shadow alone costs the update
        ps32, sq32, sh32 = ([q.float().clone() for q in u] for u in (b_flat, b_sq, b_ema))
        O.rmsprop_step(ps32, [q.float() for q in g], sq32, lr, alpha=0.999, eps=1e-10)
        O.ema_update(sh32, ps32, 0.995, t)
        for i in range(nt):
            got_p, got_sq, got_e = (after[k][i].double().cpu() for k in ("flat", "sq", "ema"))
            assert rel(got_sq, sq[i]) < 2e-4, (t, i, rel(got_sq, sq[i]))
            strong = g[i].abs() > 0.05 * g[i].abs().mean()
            upd_ref, upd_got = (ps[i] - p0[i])[strong], (got_p - p0[i])[strong]
            un = float(upd_ref.norm())
            y_upd = float(((ps32[i].double() - p0[i])[strong] - upd_ref).norm()) / un
            y_ema = float((sh32[i].double() - sh[i])[strong].norm()) / un
            e_upd = float((upd_got - upd_ref).norm()) / un
            e_ema = float((got_e - sh[i])[strong].norm()) / un
            if max(y_upd, y_ema) > 5e-4:  # (where the yardstick comes into play: DESIGN.md 3.4.1 records these)
                print(f"{case} step {t} tensor {i}: update {e_upd:.2e} (float32 torch {y_upd:.2e}) "
                      f"ema {e_ema:.2e} ({y_ema:.2e})")
            # the existing three-step test's bounds; a bound becomes max(bound, 4 x float32 torch) where float32 storage
            # itself cannot meet it: the mask scales (|p| ~ 4, ulp 4.8e-7) once their updates have shrunk to ~1e-6
            assert e_upd < max(2e-3, 4 * y_upd), (t, i, e_upd, y_upd)
            d = min(0.995, (2 + t) / (11 + t))
            want_e = b_ema[i] - (1 - d) * (b_ema[i] - got_p)
            assert rel(got_e, want_e) < 1e-6, (t, i)
            assert e_ema * un <= max(2e-3, 4 * y_ema) * un + 1e-12, (t, i, e_ema, y_ema)
    assert tr.t == tr.num_updates == 3


@pytest.mark.parametrize("case", list(TRAINER_CASES))
def test_trainer_equal_seeds_equal_bits(case):
    a, _ = _trainer(case, True)
    b, _ = _trainer(case, True)
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.x, b.x) and torch.equal(a.f, b.f) and torch.equal(a.Tf, b.Tf)
    assert torch.equal(a.P.flat, b.P.flat) and torch.equal(a.P.ema, b.P.ema) and torch.equal(a.P.sq, b.P.sq)
    assert torch.equal(a.loss, b.loss) and bool(torch.isfinite(a.P.flat).all())


def test_trainer_spectrum_against_the_oracle():
    """one evaluation pass on the 64 x 64 = 4096 points of a D = 2 grid: Rayleigh quotients within 1e-5 relative"""
    tr, prob_o = _trainer("D2_w64x3", True)
    tr.step()
    lim, val_eps = 3.2, 0.1
    out = tr.spectrum(lim, val_eps, use_ema=True)
    torch.cuda.synchronize()
    D, hidden, L, B, m = TRAINER_CASES["D2_w64x3"]
    nl = len(hidden) + 1
    e = [u.double().cpu() for u in tr.P.views(tr.P.ema)]
    ph = O.Params(e[:nl], e[nl:2 * nl], tr.P.fourier_B.double().cpu(), e[2 * nl])
    grid = O.validation_grid(lim, val_eps, D).double()
    assert grid.shape[0] == 4096
    want = O.spectrum_evd(grid, ph, prob_o, lim)
    err = float(((out["eigvals"].double() - want["eigvals"]) / want["eigvals"]).abs().max())
    print(f"spectrum: Rayleigh quotients {err:.2e}")
    assert err < 1e-5, err


# ---------------------------------------------------------------------------- 5b. the explicit door: NestedLoRA, compute_spectrum_evd
@pytest.mark.parametrize("name", list(THG.DROPIN))
def test_nestedlora_and_compute_spectrum_evd_on_this_path(name):
    """get_problem / get_evd_method under args.generic_exact_laplacian build NestedLoRA(path=PATH_GENERIC_EXACT): one
    compute_loss_operator + backward through the autograd Function against the oracle end to end (loss and gradients
    1e-4, test_highdim_gpu's end-to-end bounds), then one compute_spectrum_evd pass on 4096 points of the box: Rayleigh
    quotients within 1e-5 relative of the oracle's on the same points"""
    import argparse
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    from neural_svd_amd.operators import UniformBoxImportance, get_dataloader, get_problem
    from neural_svd_amd.spectrum import compute_spectrum_evd
    cfg = dict(THG.DROPIN[name], laplacian_eps=0.0, generic_exact_laplacian=True)
    args = argparse.Namespace(**cfg)
    args.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    torch.manual_seed(cfg["seed"])
    operator, _ = get_problem(args, DEV)
    method = get_evd_method(args, "neuralsvd", get_wavefunctions(args)).to(DEV)
    assert method.path == H.PATH_GENERIC_EXACT
    _, _, _, imp_train, _ = get_dataloader(args, DEV)
    D = args.n_particles * args.ndim
    prob = HO.problem_of(dict(cfg, scale_operator=1.0))
    assert prob.eps == 0.0 and D == {"cosine_10d": 10, "h2_3d": 6}[name]
    named = dict(method.named_parameters())
    order = sorted(k for k in named if ".ws." in k) + sorted(k for k in named if ".bs." in k) + \
        [k for k in named if k.endswith("scales")]
    fB = [t for n, t in named.items() if n.endswith("feature_map._B")][0]
    c64 = lambda t: t.detach().double().cpu().clone()  # noqa: E731
    nl = len([k for k in order if ".ws." in k])
    p64 = O.Params([c64(named[k]) for k in order[:nl]], [c64(named[k]) for k in order[nl:2 * nl]], c64(fB),
                   c64(named[order[2 * nl]]) if len(order) > 2 * nl else None)
    lim = cfg["lim"]
    x = XO.clear_batch(64, D, min(lim, 3.5), p64.scales, prob, 23)
    assert float(XO.clearance(x, p64.scales, prob).min()) > 0.1
    v, M = O.sequential_nesting_masks(4)
    ref = XO.loss_and_grads(x, p64, prob, v, M)
    method.train()
    loss, aux = method.compute_loss_operator(operator, x.float().to(DEV).view(64, args.n_particles, args.ndim),
                                             importance=imp_train)
    loss.backward()
    torch.cuda.synchronize()
    assert rel(aux["f"].detach(), ref["f"]) < 2e-5 and rel(aux["Tf"].detach(), ref["Tf"]) < 1e-4
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-4 * abs(float(ref["loss"]))
    for k, gr in zip(order, ref["grads"]):
        assert rel(named[k].grad.reshape(-1), gr.reshape(-1)) < 1e-4, k
    # the spectrum on points of the box, none near a singular point
    pts = XO.clear_batch(4096, D, lim, p64.scales, prob, 29)
    assert float(XO.clearance(pts, p64.scales, prob).min()) > 0.1
    method.eval()
    out = compute_spectrum_evd(method, dataloader=[(pts.float().to(DEV), 0.0)], operator=operator,
                               importance_train=imp_train, importance_val=UniformBoxImportance(lim, D), normalize=True,
                               device=DEV)
    c = HO.operator_forward(pts, p64, prob)
    w = BO.sqrt_importance(pts, prob)  # (the constant sqrt p_val cancels in the quotient)
    phi, Tphi = torch.nan_to_num(w * c.f), torch.nan_to_num(w * c.Tf)
    e64 = (torch.diag(phi.T @ Tphi) / torch.diag(phi.T @ phi)).numpy()
    err = float(np.abs((out["eigvals"].astype(np.float64) - e64) / e64).max())
    print(f"{name}: Rayleigh quotients {err:.2e}")
    assert err < 1e-5, (err, e64)


# ---------------------------------------------------------------------------- 6. workspace hygiene
@pytest.mark.parametrize("name", ("D3_w40_24_cosine_uniform_boxexp", "D5_w16_L17_harmonic_mask_boxsqrt"))
def test_workspace_hygiene(name):
    """a workspace of 0xFF bytes and a zero-filled one give equal bits; 1 KB margins around f, Tf and the gradients keep
    their contents"""
    p, prob, x, v, M, ref, y = _reference(name)
    shape = THG.shape_of(p, prob)
    ws_t, bs_t, fB, sc = to_dev(p)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    hp = THG.hip_problem(prob, shape.D)
    xd = x.float().to(DEV).contiguous()
    B, L, K = xd.shape[0], shape.L, 256  # 256 floats = 1 KB
    df = ref["df"].float().to(DEV).contiguous()

    def guarded(n):
        buf = torch.full((n + 2 * K,), 12345.0, device=DEV)
        return buf, buf[K:K + n]

    def run(fill):
        ws = H.new_workspace(shape, B, DEV)
        ws.fill_(fill)
        bufs = []
        fb, f = guarded(B * L)
        Tb, Tf = guarded(B * L)
        bufs += [fb, Tb]
        gw, gb = [], []
        for w in ws_t:
            b_, g_ = guarded(w.numel())
            bufs.append(b_)
            gw.append(g_.view_as(w))
        for b in bs_t:
            b_, g_ = guarded(b.numel())
            bufs.append(b_)
            gb.append(g_.view_as(b))
        gs = None
        if sc is not None:
            b_, g_ = guarded(sc.numel())
            bufs.append(b_)
            gs = g_.view_as(sc)
        grads = H.pack_params(shape, gw, gb, None, gs)
        H.operator_forward(shape, params, hp, xd, ws, path=H.PATH_GENERIC_EXACT, out=(f.view(B, L), Tf.view(B, L)))
        H.operator_backward(shape, params, hp, xd, df, grads, ws, path=H.PATH_GENERIC_EXACT)
        torch.cuda.synchronize()
        for b_ in bufs:
            assert bool((b_[:K] == 12345.0).all()) and bool((b_[-K:] == 12345.0).all())
        return [f.clone(), Tf.clone()] + [g_.clone() for g_ in gw + gb + ([gs] if gs is not None else [])]

    a, b = run(0xFF), run(0)
    for i, (u, w) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, w), i


# ---------------------------------------------------------------------------- 7. refusals
def test_refusals():
    p, prob, x, v, M, ref, y = _reference("D5_w16_L17_cosine_uniform")
    X = H.PATH_GENERIC_EXACT
    with pytest.raises(H.NsvdError, match="unsupported"):   # eps > 0 cannot be honoured on this path
        THG.run_hip(p, dataclasses.replace(prob, eps=0.01), x, v, M, X)
    with pytest.raises(H.NsvdError, match="unsupported"):   # PATH_AUTO never picks the generic jets
        THG.run_hip(p, prob, x, v, M, H.PATH_AUTO)
    p2, prob2, x2, v2, M2, _, _ = _reference("D1_w50_harmonic_mask")
    with pytest.raises(H.NsvdError, match="unsupported"):
        THG.run_hip(p2, prob2, x2, v2, M2, H.PATH_AUTO)
    with pytest.raises(H.NsvdError, match="unsupported"):
        THG.run_hip(p2, prob2, x2, v2, M2, H.PATH_GENERIC)
    # Fokker-Planck: no exact mode, with either sign of eps
    fp = HO.Problem(potential=HO.POT_SIN_OF_COS, operator_kind=HO.OP_FOKKER_PLANCK, fp_scale=0.5, pot_coef=HO.FP_CS[5],
                    op_scale=1.0, op_shift=1.0, sigma=PI32, importance=HO.IMP_UNIFORM, hard_mul_const=0.9)
    for eps in (0.0, 0.01):
        with pytest.raises(H.NsvdError, match="unsupported"):
            THG.run_hip(p, dataclasses.replace(fp, eps=eps), x, v, M, X)
    # NeuralEF's forward with eps <= 0
    shape = THG.shape_of(p2, prob2)
    ws_t, bs_t, fB, sc = to_dev(p2)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    L = shape.L
    nb, nu = torch.ones(L, device=DEV), torch.ones(L, device=DEV)
    init = torch.zeros(1, dtype=torch.int32, device=DEV)
    for path in (X, H.PATH_AUTO):
        with pytest.raises(H.NsvdError, match="unsupported"):
            H.nef_operator_forward(shape, params, THG.hip_problem(prob2, shape.D), x2.float().to(DEV),
                                   H.new_workspace(shape, x2.shape[0], DEV), nb, nu, init, 0.9, path=path)
    with pytest.raises(H.NsvdError, match="unsupported"):  # ... and on this path with eps > 0 too: no silent stencil
        H.nef_operator_forward(shape, params, THG.hip_problem(dataclasses.replace(prob2, eps=0.01), shape.D),
                               x2.float().to(DEV), H.new_workspace(shape, x2.shape[0], DEV), nb, nu, init, 0.9, path=X)
    # sharded steps: refused with a message that names the path
    from neural_svd_amd.trainer import FusedTrainer
    comm = types.SimpleNamespace(multi=True, world=1, rank=0, force_exchange=True)
    with pytest.raises(NotImplementedError, match="PATH_GENERIC_EXACT"):
        FusedTrainer(H.ModelShape(L=4, D=5, m=8, hidden=(16, 16)), H.make_problem(H.POT_HARMONIC, 0.5, 0.0, 1.0, 4.0, 2.0),
                     64, sequential=False, device=DEV, path=X, comm=comm)
    torch.cuda.synchronize()
