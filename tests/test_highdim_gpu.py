"""Problems above four input dimensions and the many-electron molecules on the GPU: the operator paths against the
reference's float64 run (tests/golden/highdim.npz) and the float64 restatement tests/_highdim_oracle.py.

Bounds are test_periodic_gpu's: f 2e-5, Tf 1e-4, gradients 3e-5 given the oracle's d loss / d f, 1e-4 end to end, the
loss 1e-4 relative. For the molecules the rows with an electron within 0.1 of a nucleus, the rows with two electrons
within 0.1 of each other and all other rows are measured as three groups, each against its own norm; for the box masks
the wall rows and the interior. No row is left out anywhere."""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _highdim_oracle as HO
from tests import test_box_gpu as TB

pytestmark = pytest.mark.gpu

H = None
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "highdim.npz")
CASES = ("cos_5d", "fp_10d", "h2_2d", "h2_3d", "lih_3d")
PI32 = float(np.float32(np.pi))
rel, to_dev = TB.rel, TB.to_dev


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import hip_ops
    H = hip_ops
    TB.H = hip_ops
    yield


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


_path = TB._path


def case_setup(z, name):
    cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
    names = [str(n) for n in z[f"{name}_param_names"]]
    t = lambda n: torch.tensor(z[f"{name}_param0_{n}"])  # noqa: E731
    sc = [t(n) for n in names if n.endswith("scales")]
    p = O.Params([t(n) for n in names if ".ws." in n], [t(n) for n in names if ".bs." in n],
                 torch.tensor(z[f"{name}_fourier_B"]), sc[0] if sc else None)
    return cfg, names, p, HO.problem_of(cfg)


def shape_of(p: O.Params, prob):
    L, h0, F = p.ws[0].shape
    return H.ModelShape(L=L, D=p.fourier_B.shape[0], m=F // 2, hidden=tuple(w.shape[1] for w in p.ws[:-1]),
                        has_exp_mask=p.scales is not None, box_mask=prob.box_mode, box_lim=prob.box_lim)


def hip_problem(prob: HO.Problem, D: int):
    """the nsvd_problem of `prob`: above four dimensions the coefficients travel as a device table, as the molecule's
    nuclei do at any dimension"""
    kw = dict(pot_coef=prob.pot_coef)
    if prob.potential == HO.POT_MOLECULE:
        kw = dict(pot_table=torch.tensor(prob.nuclei, dtype=torch.float32, device=DEV).contiguous(),
                  n_nuclei=len(prob.nuclei), pot_const=prob.pot_const)
    elif D > 4 and prob.pot_coef:
        kw = dict(pot_table=torch.tensor(prob.pot_coef, dtype=torch.float32, device=DEV))
    return H.make_problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                          prob.scale_kinetic, prob.hard_mul_const, importance_kind=prob.importance,
                          operator_kind=prob.operator_kind, fp_scale=prob.fp_scale,
                          n_particles=prob.n_particles if prob.n_particles > 1 else 0, **kw)


def run_hip(p, prob, x, v, M, path, df_override=None):
    shape = shape_of(p, prob)
    ws_t, bs_t, fB, sc = to_dev(p)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    gw = [torch.full_like(w, float("nan")) for w in ws_t]
    gb = [torch.full_like(b, float("nan")) for b in bs_t]
    gs = None if sc is None else torch.full_like(sc, float("nan"))
    grads = H.pack_params(shape, gw, gb, None, gs)
    hp = hip_problem(prob, shape.D)
    xd = x.float().to(DEV).contiguous()
    B = xd.shape[0]
    ws = H.new_workspace(shape, B, DEV)
    f, Tf = H.operator_forward(shape, params, hp, xd, ws, path=path)
    vd, Md = v.float().to(DEV), M.float().to(DEV).contiguous()
    mom = H.evd_moments(f, Tf, H.MASK_CUSTOM, vd)
    loss, df = H.evd_loss_grad(f, Tf, H.MASK_CUSTOM, vd, Md, mom)
    dfin = df if df_override is None else df_override.float().to(DEV).contiguous()
    H.operator_backward(shape, params, hp, xd, dfin, grads, ws, path=path)
    torch.cuda.synchronize()
    return dict(f=f, Tf=Tf, loss=loss, grads=gw + gb + ([gs] if gs is not None else []),
                path=H.path_name(shape, B, path, hp))


def check_rows(r, f64, Tf64, x, prob, what):
    f64, Tf64 = torch.as_tensor(np.asarray(f64)), torch.as_tensor(np.asarray(Tf64))
    if prob.box_mode:
        wall = BO.wall_rows(x.double(), prob)
        groups = (("wall", wall), ("interior", ~wall))
    else:
        groups = HO.row_groups(x.double(), prob)
    for group, rows in groups:
        if not bool(rows.any()):
            continue
        ef, eT = rel(r["f"].cpu()[rows], f64[rows]), rel(r["Tf"].cpu()[rows], Tf64[rows])
        print(f"{what} {group} rows ({int(rows.sum())}): f {ef:.2e} Tf {eT:.2e}")
        assert ef < 2e-5, (what, group, ef)
        assert eT < 1e-4, (what, group, eT)
    assert bool(torch.isfinite(r["f"]).all()) and bool(torch.isfinite(r["Tf"]).all())


# ---------------------------------------------------------------------------- 1. every fixture case
@pytest.mark.parametrize("path", ["generic", "auto", "bf16x3"])
@pytest.mark.parametrize("case", CASES)
def test_fixture_cases(z, case, path):
    """The reference's float64 run of every case; the fixture's models (hidden 16,16) are shapes of the generic
    kernels, which `auto` takes; the bf16x3 request exists on the MFMA kernels only and is REFUSED."""
    cfg, names, p, prob = case_setup(z, case)
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    x = torch.tensor(z[f"{case}_x"][0])
    shape = shape_of(p, prob)
    name = H.path_name(shape, x.shape[0], _path(path), hip_problem(prob, shape.D))
    if path == "bf16x3":
        assert name == ("unsupported" if shape.D > 4 else "generic")
        with pytest.raises(H.NsvdError, match="unsupported"):
            run_hip(p, prob, x, v, M, _path(path))
        return
    assert name == "generic"
    ref = HO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
    pre = f"{case}_f64_step0_"
    r = run_hip(p, prob, x, v, M, _path(path), df_override=ref["df"])
    check_rows(r, z[pre + "f"], z[pre + "Tf"], x, prob, f"{case}/{path}")
    for n, g, gr in zip(names, r["grads"], ref["grads"]):  # gradients given the SAME df (isolates the backward)
        e = rel(g.view(-1), gr.reshape(-1))
        assert torch.isfinite(g).all() and e < 3e-5, (n, e)
    r2 = run_hip(p, prob, x, v, M, _path(path))  # end to end
    le = abs(float(r2["loss"][0]) - float(z[pre + "loss"])) / abs(float(z[pre + "loss"]))
    print(f"{case}/{path} loss {le:.2e}")
    assert le <= 1e-4, le
    for n, g in zip(names, r2["grads"]):
        e = rel(g.view(-1), z[pre + "grad_" + n].reshape(-1))
        print(f"{case}/{path} grad {n} {e:.2e}")
        assert e < 1e-4, (n, e)


def test_refusals_above_four_dimensions(z):
    """the exact-Laplacian mode, an explicitly fused path and NeuralEF stay refused above four input dimensions"""
    cfg, names, p, prob = case_setup(z, "h2_3d")
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    x = torch.tensor(z["h2_3d_x"][0])
    import dataclasses
    with pytest.raises(H.NsvdError, match="unsupported"):
        run_hip(p, dataclasses.replace(prob, eps=0.0), x, v, M, H.PATH_AUTO)
    with pytest.raises(H.NsvdError, match="unsupported"):
        run_hip(p, prob, x, v, M, H.PATH_FUSED)
    shape = shape_of(p, prob)
    ws_t, bs_t, fB, sc = to_dev(p)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    L = shape.L
    nb, nu = torch.ones(L, device=DEV), torch.ones(L, device=DEV)
    init = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(H.NsvdError, match="unsupported"):
        H.nef_operator_forward(shape, params, hip_problem(prob, shape.D), x.to(DEV), H.new_workspace(shape, 64, DEV),
                               nb, nu, init, 0.9)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 2. epilogue sites of the direction-loop kernel
def _site_problem(combo):
    uniform = dict(eps=0.01, sigma=PI32, importance=HO.IMP_UNIFORM, hard_mul_const=0.9)
    if combo == "cos_5d":
        return 5, None, HO.Problem(potential=HO.POT_COSINE, pot_coef=HO.COSINE_CS[5], op_scale=1.0, op_shift=10.0,
                                   **uniform)
    if combo == "fp_10d":
        return 10, None, HO.Problem(potential=HO.POT_SIN_OF_COS, operator_kind=HO.OP_FOKKER_PLANCK, fp_scale=0.5,
                                    pot_coef=HO.FP_CS[10], op_scale=1.0, op_shift=1.0, **uniform)
    if combo == "fp_5d_expmask":
        return 5, 4.0, HO.Problem(potential=HO.POT_SIN_OF_COS, operator_kind=HO.OP_FOKKER_PLANCK, fp_scale=0.5,
                                  pot_coef=HO.FP_CS[5], op_scale=1.0, op_shift=1.0, **uniform)
    if combo in ("h2_3d", "lih_3d", "be_3d"):
        cfg = dict(problem="sch", potential_type="quantum_chemistry", mol_name=dict(h2_3d="H2", lih_3d="LiH",
                   be_3d="Be")[combo], ndim=3, laplacian_eps=0.01, operator_scale=1.0, operator_shift=0.0,
                   sampling_scale=2.0, hard_mul_const=1.0, sampling_mode="gaussian")
        prob = HO.problem_of(cfg)
        return 3 * prob.n_particles, 4.0, prob
    kind = BO.BOX_SQRT if combo.endswith("sqrt") else BO.BOX_EXP
    return 5, None, HO.Problem(potential=BO.POT_ZERO, eps=0.01, sigma=4.0, importance=HO.IMP_UNIFORM, op_scale=1.0,
                               op_shift=0.5, hard_mul_const=0.9, box_mode=kind, box_lim=4.0)


SITE_COMBOS = ("cos_5d", "fp_10d", "fp_5d_expmask", "h2_3d", "lih_3d", "be_3d", "box5_sqrt", "box5_exp")


@pytest.mark.parametrize("L,B", [(5, 96), (18, 70)])
@pytest.mark.parametrize("combo", SITE_COMBOS)
def test_epilogue_sites(combo, L, B):
    """the special rows of each problem through the direction-loop kernel against the float64 restatement: a row at the
    origin and rows with |x_d| = pi (periodic), an electron 1e-3 from a nucleus on the molecule's axis and two
    electrons 1e-3 apart (molecules), rows at and beyond the wall (box). Shapes: B = 96 and 70 (a partial last
    workgroup of 64 rows), L = 5 (not a multiple of the four waves) and 18 (a second head tile of 16)."""
    D, mask_init, prob = _site_problem(combo)
    p = O.init_params(L, D, 8, (16, 16), 0.2, exp_mask_init=mask_init, seed=44)
    g = torch.Generator().manual_seed(9)
    if prob.importance == HO.IMP_UNIFORM:
        x = prob.sigma * (2 * torch.rand(B, D, generator=g) - 1)
    else:
        x = 2.0 * torch.randn(B, D, generator=g)
    x = x.float()
    if prob.potential == HO.POT_MOLECULE:
        R = torch.tensor(prob.nuclei, dtype=torch.float32)[:, :-1]
        npart = prob.n_particles
        xr = x.view(B, npart, 3)
        xr[0, 0] = R[-1]
        xr[0, 0, 0] += 1e-3                        # on the axis through the nuclei, 1e-3 beyond the last one
        xr[1, npart - 1] = R[0]
        xr[1, npart - 1, 0] -= 1e-3
        xr[2, 1] = xr[2, 0]
        xr[2, 1, 2] += 1e-3                        # two electrons 1e-3 apart
        xr[3, 1] = xr[3, 0]
        xr[3, 1, 0] -= 1e-3
        en, ee = HO.distances(x, prob)
        assert float(en.min()) > 0.9e-3 and float(ee.min()) > 0.9e-3
    elif prob.box_mode:
        lim = prob.box_lim
        x[0] = 0.0
        x[1, 0], x[2, 4], x[3, 2] = lim, -lim, lim + 0.5
        x[4, 1], x[5, 3] = lim - 0.005, -lim + 0.005
        x[B - 1, 4] = lim
    else:
        x[0] = 0.0
        x[1] = PI32
        x[2] = -PI32
        x[3, 0], x[3, D - 1] = PI32, float(np.float32(np.pi / 2))
        x[B - 1, D - 1] = -PI32
    v, M = O.sequential_nesting_masks(L)
    ref = HO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
    assert bool(torch.isfinite(ref["Tf"]).all())
    r = run_hip(p, prob, x, v, M, H.PATH_AUTO, df_override=ref["df"])
    assert r["path"] == "generic"
    check_rows(r, ref["f"], ref["Tf"], x, prob, f"{combo}/L{L}/B{B}")
    if prob.box_mode:
        outside = (x.abs() >= prob.box_lim).any(dim=1)
        assert bool((r["f"].cpu()[outside] == 0).all())
    for i, (a, b) in enumerate(zip(r["grads"], ref["grads"])):
        assert torch.isfinite(a).all(), i
        assert rel(a.view(-1), b.reshape(-1)) < 3e-5, (i, rel(a.view(-1), b.reshape(-1)))


# ---------------------------------------------------------------------------- 3. device sampler above four dimensions
@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
@pytest.mark.parametrize("D", [5, 12])
def test_device_sampler(D, kind):
    """same (seed, offset): the same bits; another offset: other values; per-coordinate mean and variance within 5
    standard errors of the density's; no two coordinates of a row equal"""
    B, sigma = 4096, 2.0
    shape = H.ModelShape(L=2, D=D, m=8, hidden=(16,))
    p = O.init_params(2, D, 8, (16,), 0.2, seed=1)
    ws_t, bs_t, fB, sc = to_dev(p)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    imp = H.IMP_GAUSSIAN if kind == "gaussian" else H.IMP_UNIFORM
    prob = H.make_problem(H.POT_HARMONIC, 1.0, 0.01, 1.0, 0.0, sigma, importance_kind=imp)
    ws = H.new_workspace(shape, B, DEV)

    def draw(seed, offset):
        x = torch.full((B, D), float("nan"), device=DEV)
        H.operator_sample_features(shape, params, prob, seed, offset, x, ws, path=H.PATH_GENERIC)
        torch.cuda.synchronize()
        return x

    a, b, c = draw(7, 3), draw(7, 3), draw(7, 4)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # (23-bit draws: two streams agree at a position with probability 2^-23)
    assert float((a == c).float().mean()) < 1e-3 and float((a == draw(8, 3)).float().mean()) < 1e-3
    xs = a.double().cpu()
    if kind == "gaussian":
        var, se_var = sigma ** 2, sigma ** 2 * np.sqrt(2.0 / (B - 1))
    else:
        assert float(xs.abs().max()) < sigma
        var, se_var = sigma ** 2 / 3, sigma ** 2 * np.sqrt(4.0 / 45.0 / B)
    assert bool((xs.mean(0).abs() < 5 * np.sqrt(var / B)).all()), xs.mean(0)
    assert bool(((xs.var(0) - var).abs() < 5 * se_var).all()), xs.var(0)
    srt = xs.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    # the features of the batch drawn LAST are in the workspace: the forward on them is the forward on x
    a = draw(7, 3)
    f1, Tf1 = H.operator_forward(shape, params, prob, a, ws, path=H.PATH_GENERIC, features_ready=True)
    f2, Tf2 = H.operator_forward(shape, params, prob, a, H.new_workspace(shape, B, DEV), path=H.PATH_GENERIC)
    torch.cuda.synchronize()
    assert torch.equal(f1, f2) and torch.equal(Tf1, Tf2)


# ---------------------------------------------------------------------------- 4. fused training steps
def _trainer(z, case, B=None, **kw):
    from neural_svd_amd.trainer import FusedTrainer
    cfg, names, p, prob = case_setup(z, case)
    shape = shape_of(p, prob)
    tr = FusedTrainer(shape, hip_problem(prob, shape.D), B or cfg["batch_size"], sequential=True, step=1, lr=cfg["lr"],
                      rmsprop_decay=cfg["rmsprop_decay"], rmsprop_eps=1e-10, num_iters=cfg["num_iters"],
                      use_lr_scheduler=True, sampling_scale=cfg["sampling_scale"], seed=0, device=DEV,
                      exp_mask_init=None if p.scales is None else 1.0, **kw)
    tr.P.load(p.fourier_B, p.ws, p.bs, p.scales)
    return cfg, names, p, prob, tr


@pytest.mark.parametrize("case", ["cos_5d", "h2_3d"])
def test_fused_trainer_steps(z, case):
    """8 FusedTrainer.step(x) calls from the fixture's weights against the float64 trajectory of the restatement (held
    to the reference at 1e-9 on the CPU), at the bound of test_periodic_gpu.test_fused_trainer_steps_on_the_fixture"""
    n_steps = 8
    cfg, names, p, prob, tr = _trainer(z, case, device_sampler=False)
    g = torch.Generator().manual_seed(11)
    B, D = cfg["batch_size"], p.fourier_B.shape[0]
    if prob.importance == HO.IMP_UNIFORM:
        xs = [(PI32 * (2 * torch.rand(B, D, generator=g) - 1)).float() for _ in range(n_steps)]
    else:
        xs = [(cfg["sampling_scale"] * torch.randn(B, D, generator=g)).float() for _ in range(n_steps)]
    xs[0] = torch.tensor(z[f"{case}_x"][0])
    p64 = p.to(torch.float64)
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    sq = [torch.zeros_like(t) for t in p64.trainable()]
    for it in range(n_steps):
        tr.step(xs[it].to(DEV).contiguous())
        torch.cuda.synchronize()
        r = HO.loss_and_grads(xs[it].double(), p64, prob, v, M)
        if it == 0:
            assert rel(tr.f, z[f"{case}_f64_step0_f"]) < 2e-5
            assert rel(tr.Tf, z[f"{case}_f64_step0_Tf"]) < 1e-4
            l64 = float(z[f"{case}_f64_step0_loss"])
            assert abs(float(tr.loss[0]) - l64) < 1e-4 * abs(l64)
        O.rmsprop_step(p64.trainable(), r["grads"], sq, O.cosine_lr(cfg["lr"], it, cfg["num_iters"]),
                       cfg["rmsprop_decay"], 1e-10)
    upd = n_steps * cfg["lr"] / np.sqrt(1.0 - cfg["rmsprop_decay"])
    for n, got, want in zip(names, tr.P.views(tr.P.flat), p64.trainable()):
        err = float((got.double().cpu() - want.reshape(got.shape)).norm())
        assert err <= 2e-3 * (float(want.norm()) + upd * np.sqrt(want.numel())), (n, err)


@pytest.mark.parametrize("case", ["cos_5d", "h2_3d"])
def test_device_sampler_steps_and_state_round_trip(z, case):
    """8 eager steps on the trainer's own device sampler (the D > 4 stream), then the state (weights, EMA, optimiser
    buffers, counters) into a fresh trainer: its next step equals the original's, bit for bit. The captured graph needs
    the device-resident schedule, which the MFMA kernels read: above four dimensions the step runs on the generic
    kernels, and capture is refused in words."""
    _, _, _, prob, a = _trainer(z, case)
    with pytest.raises(H.NsvdError, match="MFMA path"):
        _trainer(z, case, device_schedule=True)
    for _ in range(8):
        a.step()
    torch.cuda.synchronize()
    assert a.t == 8 and a.batches_drawn == 8
    assert bool(torch.isfinite(a.P.flat).all()) and float(a.f.abs().max()) > 0
    if prob.importance == HO.IMP_UNIFORM:
        assert float(a.x.abs().max()) < PI32
    _, _, _, _, b = _trainer(z, case)
    b.P.load_state_dict(a.state_dict(), a.state_dict(ema=True), reset_optimizer=False)
    b.load_optimizer_state_dict(a.optimizer_state_dict())
    a.step()
    b.step()
    torch.cuda.synchronize()
    for name in ("flat", "sq", "ema"):
        assert torch.equal(getattr(a.P, name), getattr(b.P, name)), name
    assert torch.equal(a.x, b.x) and torch.equal(a.f, b.f) and torch.equal(a.Tf, b.Tf)


# ---------------------------------------------------------------------------- 5. drop-in
DROPIN_ARGS = dict(seed=0, n_particles=1, neigs=4, mlp_hidden_dims="16,16", nonlinearity="softplus", parallel=1,
                   weight_normalization=0, use_fourier_feature=True, fourier_append_raw=False, apply_boundary=0,
                   boundary_mode="dir_box_sqrt", hard_mul_const=1.0, charge=1.0, laplacian_eps=0.01, operator_scale=1.0,
                   batch_size=64, val_eps=1.0, optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0,
                   num_iters=3, sort=0, high_dim_stencil=True)
DROPIN = dict(
    cosine_10d=dict(DROPIN_ARGS, problem="sch", potential_type="cosine", ndim=10, lim=float(np.pi), fourier_mapping_size=4,
                    fourier_scale=1.0, fourier_deterministic=True, apply_exp_mask=0, exp_mask_init_scale=10.0,
                    operator_shift=10.0, sampling_mode="uniform", sampling_scale=float(np.pi)),
    h2_3d=dict(DROPIN_ARGS, problem="sch", potential_type="quantum_chemistry", mol_name="H2", ndim=3, lim=5.0,
               fourier_mapping_size=8, fourier_scale=0.1, fourier_deterministic=False, apply_exp_mask=1,
               exp_mask_init_scale=4.0, operator_shift=0.0, sampling_mode="gaussian", sampling_scale=2.0),
)


class _Rows:
    fieldnames = None

    def __init__(self):
        self.rows = []

    def writerow(self, row):
        self.rows.append(dict(row))


@pytest.mark.parametrize("name", list(DROPIN))
def test_dropin_runs_the_fused_loop(name):
    """get_problem(high_dim_stencil) / get_wavefunctions / get_dataloader / get_evd_method / train_operator: 3 steps
    through FusedTrainer (generic kernels), the first loss the float64 restatement's at 1e-4, then one
    compute_spectrum_evd on 4096 points sampled from the box against the restatement on the same points, at the bound of
    test_periodic_gpu.test_spectrum_matches_the_fixture"""
    import argparse
    import neural_svd_amd.drop_in as DI
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    from neural_svd_amd.operators import UniformBoxImportance, get_dataloader, get_problem
    from neural_svd_amd.spectrum import compute_spectrum_evd
    from neural_svd_amd.trainer import FusedTrainer
    cfg = DROPIN[name]
    args = argparse.Namespace(**cfg)
    args.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    args.adam_eps, args.use_lr_scheduler, args.ema_decay = 1e-7, True, 0.995
    args.print_freq, args.eval_freq, args.log_dir = 1, 10 ** 9, None
    torch.manual_seed(cfg["seed"])
    operator, gt = get_problem(args, DEV)
    method = get_evd_method(args, "neuralsvd", get_wavefunctions(args)).to(DEV)
    _, val_data, batch_ftn_val, imp_train, imp_val = get_dataloader(args, DEV)
    assert val_data is None and batch_ftn_val is None  # no grid above two dimensions / for several particles
    D = args.n_particles * args.ndim
    prob = HO.problem_of(dict(cfg, scale_operator=1.0))
    assert D == {"cosine_10d": 10, "h2_3d": 6}[name] and prob.n_particles == args.n_particles

    def params64():
        named = dict(method.named_parameters())
        ws = [named[n] for n in sorted(k for k in named if ".ws." in k)]
        bs = [named[n] for n in sorted(k for k in named if ".bs." in k)]
        sc = [t for n, t in named.items() if n.endswith("scales")]
        fB = [t for n, t in named.items() if n.endswith("feature_map._B")][0]
        c = lambda t: t.detach().double().cpu().clone()  # noqa: E731
        return O.Params([c(w) for w in ws], [c(b) for b in bs], c(fB), c(sc[0]) if sc else None)

    p0 = params64()
    g = torch.Generator().manual_seed(17)
    if cfg["sampling_mode"] == "uniform":
        xs = [(PI32 * (2 * torch.rand(64, D, generator=g) - 1)).float() for _ in range(3)]
    else:
        xs = [(2.0 * torch.randn(64, D, generator=g)).float() for _ in range(3)]
    it = iter(xs)
    box, rows = {}, _Rows()
    orig_fused = DI._fused_loop_trainer

    def spy_fused(*a, **k):
        box["fused"] = orig_fused(*a, **k)
        return box["fused"]

    DI._fused_loop_trainer = spy_fused
    try:
        DI.train_operator(args, method, operator, lambda: next(it).view(64, args.n_particles, args.ndim), val_data,
                          batch_ftn_val, rows, None, DEV, imp_train, imp_val, gt)
    finally:
        DI._fused_loop_trainer = orig_fused
    tr = box["fused"]
    assert isinstance(tr, FusedTrainer) and tr.t == 3
    assert H.path_name(tr.shape, tr.B, tr.path, tr.problem) == "generic" and tr.shape.D == D
    v, M = O.sequential_nesting_masks(4)
    l64 = float(HO.loss_and_grads(xs[0].double(), p0, prob, v, M)["loss"])
    losses = [r["train_loss"] for r in rows.rows]
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert abs(losses[0] - l64) <= 1e-4 * abs(l64), (losses[0], l64)
    # the spectrum on points sampled from the box
    lim = cfg["lim"]
    pts = (lim * (2 * torch.rand(4096, D, generator=g) - 1)).float()
    method.eval()
    out = compute_spectrum_evd(method, dataloader=[(pts.to(DEV), 0.0)], operator=operator, importance_train=imp_train,
                               importance_val=UniformBoxImportance(lim, D), normalize=True, device=DEV)
    p64 = params64()
    x64 = pts.double()
    c = HO.operator_forward(x64, p64, prob)
    sqrt_val = np.sqrt(float(np.float32(1.0 / (2 * lim) ** D)))
    w = BO.sqrt_importance(x64, prob) / sqrt_val
    phi, Tphi = torch.nan_to_num(w * c.f), torch.nan_to_num(w * c.Tf)
    cov, quad = phi.T @ phi / 4096, phi.T @ Tphi / 4096
    e64, n64 = (torch.diag(quad) / torch.diag(cov)).numpy(), torch.diag(cov).numpy()
    tol = 1e-4 * (c.Tf.norm(dim=0) / c.f.norm(dim=0)).numpy() + 1e-4 * np.abs(e64)
    print(f"{name} eigvals err {np.abs(out['eigvals'] - e64)} tol {tol}")
    assert rel(out["norms"], n64) < 1e-4
    assert np.all(np.abs(out["eigvals"] - e64) <= tol)
