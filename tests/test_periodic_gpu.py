"""Cosine, H2+, 3-D hydrogen and Fokker-Planck problems on the GPU: every operator path against the reference's float64
run (tests/golden/periodic.npz) and the float64 restatement tests/_periodic_oracle.py.

Bounds are test_box_gpu's (test_hip_parity.test_operator_forward_backward_small's): f 2e-5, Tf 1e-4 (exact mode 2e-5),
gradients 3e-5 given the oracle's d loss / d f, 1e-4 end to end, the loss 1e-4 relative. For H2+ the rows within 0.1 of
a nucleus (|V| up to 2 q / 1e-3) and all other rows are measured as two groups, each against its own norm, never
pooled: the near-nucleus rows would otherwise hide the rest. No row is left out anywhere."""
import argparse
import ast
import os

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _golden as G
from tests import _periodic_oracle as PO
from tests import test_box_gpu as TB

pytestmark = pytest.mark.gpu

H = None
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "periodic.npz")
CASES = ("cos_2d", "cos_1d", "cos_2d_exact", "fp_2d", "fp_2d_eps01", "fp_1d", "fp_2d_expmask", "h2p_2d", "h2p_3d_exact",
         "hyd_3d")
SITES, SITE_RUNS = TB.SITES, TB.SITE_RUNS
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
    return cfg, names, p, PO.problem_of(cfg)


def shape_of(p: O.Params):
    L, h0, F = p.ws[0].shape
    return H.ModelShape(L=L, D=p.fourier_B.shape[0], m=F // 2, hidden=tuple(w.shape[1] for w in p.ws[:-1]),
                        has_exp_mask=p.scales is not None)


def hip_problem(prob: PO.Problem):
    return H.make_problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                          prob.scale_kinetic, prob.hard_mul_const, importance_kind=prob.importance,
                          operator_kind=prob.operator_kind, fp_scale=prob.fp_scale, pot_coef=prob.pot_coef)


def run_hip(p, prob, x, v, M, path, df_override=None):
    """test_box_gpu.run_hip with the potential's coefficients and the operator kind in the problem"""
    shape = shape_of(p)
    ws_t, bs_t, fB, sc = to_dev(p)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    gw = [torch.full_like(w, float("nan")) for w in ws_t]
    gb = [torch.full_like(b, float("nan")) for b in bs_t]
    gs = None if sc is None else torch.full_like(sc, float("nan"))
    grads = H.pack_params(shape, gw, gb, None, gs)
    hp = hip_problem(prob)
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
    """f and Tf of every row; H2+: the rows within 0.1 of a nucleus and the others, each group against its own norm"""
    tf_tol = 1e-4 if prob.eps > 0 else 2e-5
    f64, Tf64 = torch.as_tensor(np.asarray(f64)), torch.as_tensor(np.asarray(Tf64))
    every = torch.ones(x.shape[0], dtype=torch.bool)
    groups = (("all", every),)
    if prob.potential == PO.POT_H2_ION:
        near = PO.nucleus_rows(x.double(), prob)
        assert bool(near.any()) and bool((~near).any())
        groups = (("nucleus", near), ("other", ~near))
    for group, rows in groups:
        ef, eT = rel(r["f"].cpu()[rows], f64[rows]), rel(r["Tf"].cpu()[rows], Tf64[rows])
        print(f"{what} {group} rows ({int(rows.sum())}): f {ef:.2e} Tf {eT:.2e}")
        assert ef < 2e-5, (what, group, ef)
        assert eT < tf_tol, (what, group, eT)
    assert bool(torch.isfinite(r["f"]).all()) and bool(torch.isfinite(r["Tf"]).all())


# ---------------------------------------------------------------------------- 1. every fixture case on every path
@pytest.mark.parametrize("path", ["generic", "auto", "bf16x3"])
@pytest.mark.parametrize("case", CASES)
def test_fixture_cases(z, case, path):
    """The reference's float64 run of every case on the three path requests, with test_box_gpu.test_fixture_cases'
    refusal pattern: the fixture's models (hidden 16,16) are shapes of the generic kernels; the exact-Laplacian cases
    and the bf16x3 request exist on the MFMA kernels only and are REFUSED for these shapes."""
    cfg, names, p, prob = case_setup(z, case)
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    x = torch.tensor(z[f"{case}_x"][0])
    shape, hp = shape_of(p), hip_problem(prob)
    name = H.path_name(shape, x.shape[0], _path(path), hp)
    if prob.eps <= 0 or path == "bf16x3":
        assert name == ("unsupported" if prob.eps <= 0 else "generic")
        with pytest.raises(H.NsvdError, match="unsupported"):
            run_hip(p, prob, x, v, M, _path(path))
        return
    assert name == "generic"
    ref = PO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
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


# ---------------------------------------------------------------------------- 2. every epilogue site of the MFMA kernels
PI32 = float(np.float32(np.pi))


def planted(x, prob):
    """the fixture's planted rows: the periodic problems on x_d in {0, pi/2, pi, -pi}, H2+ 1e-3 and eps / 2 (exact mode:
    5e-3) from each nucleus, beside it and on the axis (one input dimension: on the axis only)"""
    x = x.float().clone()
    D = x.shape[1]
    last = D - 1
    if prob.potential == PO.POT_H2_ION:
        R = float(prob.pot_coef[0])
        near = float(np.float32(prob.eps)) / 2 if prob.eps > 0 else 5e-3
        x[:4] = 0.0
        if D == 1:
            x[0, 0], x[1, 0], x[2, 0], x[3, 0] = R + 1e-3, -R + 1e-3, -R - near, R - near
        else:
            x[0, 0], x[0, last] = 1e-3, R
            x[1, last] = -R + 1e-3
            x[2, 0], x[2, last] = near, -R
            x[3, last] = R - near
        return x
    vals = [0.0, float(np.float32(np.pi / 2)), PI32, -PI32]
    for j, v in enumerate(vals):
        x[2 * j, 0] = v
        x[2 * j + 1, last] = v
    x[8, :] = vals[2]
    x[9, :] = vals[0]
    x[9, last] = vals[1]
    return x


COMBOS = ("cosine_uniform", "fp_uniform", "fp_uniform_expmask", "h2p_gauss")


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("site,path", SITE_RUNS)
def test_epilogue_sites(site, path, combo):
    """cosine + uniform, Fokker-Planck + uniform (without and with the exponential mask) and H2+ + Gaussian at every
    place the MFMA kernels form f, Tf (test_box_gpu.SITES, unchanged), against the float64 restatement; the planted
    rows are always in the batch. The exact sites do not exist for Fokker-Planck: "unsupported", and refused."""
    D, L, B, m, hidden, eps = SITES[site]
    cs = (0.814723686393179, 0.905791937075619, 0.126986816293506)[:D]
    uniform = dict(eps=eps, sigma=PI32, importance=PO.IMP_UNIFORM, hard_mul_const=0.9)
    mask_init = None
    if combo == "cosine_uniform":
        prob = PO.Problem(potential=PO.POT_COSINE, pot_coef=cs, op_scale=1.0, op_shift=10.0, **uniform)
    elif combo.startswith("fp_"):
        prob = PO.Problem(potential=PO.POT_SIN_OF_COS, operator_kind=PO.OP_FOKKER_PLANCK, fp_scale=0.5,
                          pot_coef=(1.0, 0.8, 0.6)[:D], op_scale=1.0, op_shift=1.0, **uniform)
        mask_init = 4.0 if combo.endswith("expmask") else None
    else:
        prob = PO.Problem(potential=PO.POT_H2_ION, charge_or_k=2.0, pot_coef=(1.0,), eps=eps, op_scale=1.0, op_shift=0.0,
                          sigma=2.0, importance=PO.IMP_GAUSSIAN)
        mask_init = 4.0
    if site == "hyd_med":  # weights from the seed recipe of the golden case
        zz = G.load("model_headline")
        c = dict(G.cfg_of(zz, "hyd_med"), apply_exp_mask=int(mask_init is not None), exp_mask_init_scale=mask_init)
        p = G.params_from_seed(c)
    else:
        p = O.init_params(L, D, m, hidden, 0.2, exp_mask_init=mask_init, seed=44)
    g = torch.Generator().manual_seed(9)
    if prob.importance == PO.IMP_UNIFORM:
        x = PI32 * (2 * torch.rand(B, D, generator=g) - 1)
    else:
        x = 2.0 * torch.randn(B, D, generator=g)
    x = planted(x, prob)
    v, M = O.sequential_nesting_masks(L)
    if prob.operator_kind == PO.OP_FOKKER_PLANCK and eps <= 0:
        assert H.path_name(shape_of(p), B, _path(path), hip_problem(prob)) == "unsupported"
        with pytest.raises(H.NsvdError, match="unsupported"):
            run_hip(p, prob, x, v, M, _path(path))
        return
    ref = PO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
    r = run_hip(p, prob, x, v, M, _path(path), df_override=ref["df"])
    assert r["path"] == "fused_mfma", r["path"]  # (never the generic kernels)
    check_rows(r, ref["f"], ref["Tf"], x, prob, f"{site}/{path}/{combo}")
    for i, (a, b) in enumerate(zip(r["grads"], ref["grads"])):
        assert torch.isfinite(a).all(), i
        assert rel(a.view(-1), b.reshape(-1)) < 3e-5, (i, rel(a.view(-1), b.reshape(-1)))


# ---------------------------------------------------------------------------- 3. fused training steps
def _trainer_on_fixture(z, case, **kw):
    from neural_svd_amd.trainer import FusedTrainer
    cfg, names, p, prob = case_setup(z, case)
    tr = FusedTrainer(shape_of(p), hip_problem(prob), cfg["batch_size"], sequential=True, step=1, lr=cfg["lr"],
                      rmsprop_decay=cfg["rmsprop_decay"], rmsprop_eps=1e-10, num_iters=cfg["num_iters"],
                      use_lr_scheduler=True, sampling_scale=cfg["sampling_scale"], seed=0, device=DEV,
                      device_sampler=False, exp_mask_init=None if p.scales is None else 1.0, **kw)
    tr.P.load(p.fourier_B, p.ws, p.bs, p.scales)  # (the constructor's own initial values are replaced)
    return cfg, names, tr


@pytest.mark.parametrize("case", ["fp_2d", "cos_2d"])
def test_fused_trainer_steps_on_the_fixture(z, case):
    """three FusedTrainer.step(x) calls on the fixture's weights and recorded batches against the float64 trajectory
    (the reference's parameters after its three steps, which the restatement reproduces to 1e-9), at the bound of
    test_box_gpu.test_fused_trainer_steps_on_the_fixture (RMSprop's early updates are sign-like)."""
    n_steps = 3
    cfg, names, tr = _trainer_on_fixture(z, case)
    xs = [torch.tensor(z[f"{case}_x"][it]).to(DEV).contiguous() for it in range(n_steps)]
    for it in range(n_steps):
        tr.step(xs[it])
        torch.cuda.synchronize()
        if it == 0:  # (from the second step on the two trajectories differ by the sign-like updates)
            assert rel(tr.f, z[f"{case}_f64_step0_f"]) < 2e-5
            assert rel(tr.Tf, z[f"{case}_f64_step0_Tf"]) < 1e-4
            l64 = float(z[f"{case}_f64_step0_loss"])
            assert abs(float(tr.loss[0]) - l64) < 1e-4 * abs(l64)
    upd = n_steps * cfg["lr"] / np.sqrt(1.0 - cfg["rmsprop_decay"])
    for n, got in zip(names, tr.P.views(tr.P.flat)):
        want = torch.tensor(z[f"{case}_f64_step{n_steps - 1}_param_{n}"])
        err = float((got.double().cpu() - want).norm())
        assert err <= 2e-3 * (float(want.norm()) + upd * np.sqrt(want.numel())), (n, err)


# ---------------------------------------------------------------------------- 4. captured graph, uniform device sampler
def test_graphed_fokker_planck_steps_with_the_uniform_device_sampler():
    """test_box_gpu's graph shape (L 4, D 2, m 64, (128,128,128)) on the Fokker-Planck problem with the uniform density:
    FusedTrainer.capture_graph against the same number of eager steps, equal bits; every batch inside [-pi, pi]^2."""
    from neural_svd_amd.trainer import FusedTrainer
    shape = H.ModelShape(L=4, D=2, m=64, hidden=(128, 128, 128))
    prob = H.make_problem(H.POT_SIN_OF_COS, 0.0, 0.01, 1.0, 1.0, PI32, importance_kind=H.IMP_UNIFORM,
                          operator_kind=H.OP_FOKKER_PLANCK, fp_scale=1.0, pot_coef=(1.0, 1.0))
    assert H.path_name(shape, 64, H.PATH_AUTO, prob) == "fused_mfma"

    def make(sched):
        return FusedTrainer(shape, prob, 64, sequential=True, lr=1e-3, num_iters=60, seed=4, device=DEV,
                            sampling_scale=PI32, fourier_scale=0.1, device_schedule=sched)
    a, g = make(False), make(True)
    gs = g.capture_graph(2)
    gs.replay(5)
    for _ in range(g.t):
        a.step()
        assert float(a.x.abs().max()) < PI32
    torch.cuda.synchronize()
    for name in ("flat", "sq", "ema"):
        assert torch.equal(getattr(a.P, name), getattr(g.P, name)), name
    assert torch.equal(a.x, g.x) and torch.equal(a.f, g.f) and torch.equal(a.Tf, g.Tf)
    assert bool(torch.isfinite(a.P.flat).all()) and float(a.f.abs().max()) > 0


# ---------------------------------------------------------------------------- 5. compute_spectrum_evd
def _args(cfg):
    a = argparse.Namespace(**cfg)
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    a.adam_eps, a.use_lr_scheduler, a.ema_decay = 1e-7, True, 0.995
    a.print_freq, a.eval_freq, a.log_dir = 10 ** 9, 10 ** 9, None
    return a


def _build(cfg):
    """the reference-style construction (main_pde.py) from this package's factories"""
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    from neural_svd_amd.operators import get_dataloader, get_problem
    args = _args(cfg)
    torch.manual_seed(cfg["seed"])
    operator, gt = get_problem(args, DEV)
    method = get_evd_method(args, "neuralsvd", get_wavefunctions(args)).to(DEV)
    return args, operator, gt, method, get_dataloader(args, DEV)


@pytest.mark.parametrize("case", ["cos_2d", "fp_2d"])
def test_spectrum_matches_the_fixture(z, case):
    """compute_spectrum_evd (the device spectrum) and FusedTrainer.spectrum on the fixture's grid with the parameters
    the reference evaluated (after its third step). Norms at 1e-4 (f at 2e-5, squared). An eigenvalue is
    <phi, T phi> / <phi, phi>: with T phi within 1e-4 of its norm the quotient moves by at most
    1e-4 |T phi| / |phi| (Cauchy-Schwarz), plus 1e-4 of itself for the norm - it can be a small difference of large
    terms, so the bound is not relative to the eigenvalue alone."""
    from neural_svd_amd.spectrum import compute_spectrum_evd
    cfg, names, p0, prob = case_setup(z, case)
    args, operator, gt, method, (_, val_data, batch_ftn_val, imp_train, imp_val) = _build(cfg)
    with torch.no_grad():
        for n, t in method.named_parameters():
            if t.requires_grad:
                t.copy_(torch.tensor(z[f"{case}_f64_step2_param_{n}"]).float())
            elif n.endswith("feature_map._B"):
                t.copy_(torch.tensor(z[f"{case}_fourier_B"]))
    assert np.array_equal(val_data.cpu().numpy(), z[f"{case}_val_data"])
    pt = [torch.tensor(z[f"{case}_f64_step2_param_{n}"]) for n in names]
    nl = len(p0.ws)
    p64 = O.Params(pt[:nl], pt[nl:2 * nl], p0.fourier_B.double(), None)
    c = PO.operator_forward(torch.tensor(z[f"{case}_val_data"], dtype=torch.float64), p64, prob)
    e64 = z[f"{case}_f64_spec_eigvals"]
    tol = 1e-4 * (c.Tf.norm(dim=0) / c.f.norm(dim=0)).numpy() + 1e-4 * np.abs(e64)
    method.eval()
    out = compute_spectrum_evd(method, dataloader=batch_ftn_val(), operator=operator, importance_train=imp_train,
                               importance_val=imp_val, normalize=True, device=DEV)
    print(f"{case} eigvals err {np.abs(out['eigvals'] - e64)} tol {tol}")
    assert rel(out["norms"], z[f"{case}_f64_spec_norms"]) < 1e-4
    assert np.all(np.abs(out["eigvals"] - e64) <= tol)
    _, _, tr = _trainer_on_fixture(z, case)
    tr.P.load(p0.fourier_B, [t.float() for t in pt[:nl]], [t.float() for t in pt[nl:2 * nl]], None)
    s = tr.spectrum(cfg["lim"], cfg["val_eps"], use_ema=False, chunk=150)
    assert np.all(np.abs(s["eigvals"].numpy() - e64) <= tol)
    assert rel(s["norms"], z[f"{case}_f64_spec_norms"]) < 1e-4


# ---------------------------------------------------------------------------- 6. drop-in
PERIODIC_ARGS = dict(seed=0, ndim=2, n_particles=1, neigs=4, mlp_hidden_dims="128,128,128", nonlinearity="softplus",
                     parallel=1, weight_normalization=0, use_fourier_feature=True, fourier_mapping_size=32,
                     fourier_scale=1.0, fourier_deterministic=True, fourier_append_raw=False, apply_boundary=0,
                     boundary_mode="dir_box_sqrt", lim=float(np.pi), apply_exp_mask=0, exp_mask_init_scale=10.0,
                     hard_mul_const=1.0, problem="sch", potential_type="cosine", charge=1.0, laplacian_eps=0.01,
                     operator_scale=1.0, operator_shift=10.0, sampling_mode="uniform", sampling_scale=float(np.pi),
                     batch_size=64, val_eps=1.0, optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0,
                     num_iters=20, sort=0)


@pytest.mark.parametrize("over", [dict(), dict(problem="fp", operator_shift=1.0)], ids=["cosine", "fp"])
def test_dropin_runs_the_fused_loop(over):
    """get_problem / get_wavefunctions / get_dataloader / get_evd_method / train_operator from the argument set of
    main_pde.py's parser (neither use_gaussian_sampling nor scale_operator in it): 20 iterations with two evaluations;
    the loop taken is FusedTrainer on the MFMA kernels."""
    import neural_svd_amd.drop_in as DI
    from neural_svd_amd.trainer import FusedTrainer
    args, operator, gt, method, (make_batch, val_data, batch_ftn_val, imp_train, imp_val) = \
        _build(dict(PERIODIC_ARGS, **over))
    args.eval_freq = args.num_iters // 2
    box = {}
    orig_fused = DI._fused_loop_trainer

    def spy_fused(*a, **k):
        box["fused"] = orig_fused(*a, **k)
        return box["fused"]

    DI._fused_loop_trainer = spy_fused
    try:
        torch.manual_seed(123)
        eig, norms = DI.train_operator(args, method, operator, make_batch, val_data, batch_ftn_val, None, None, DEV,
                                       imp_train, imp_val, gt)
    finally:
        DI._fused_loop_trainer = orig_fused
    tr = box["fused"]
    fp = over.get("problem") == "fp"
    assert isinstance(tr, FusedTrainer) and tr.t == 20
    assert tr.problem.use_importance == H.IMP_UNIFORM
    assert tr.problem.operator_kind == (H.OP_FOKKER_PLANCK if fp else H.OP_SCHROEDINGER)
    assert tr.problem.potential == (H.POT_SIN_OF_COS if fp else H.POT_COSINE)
    assert H.path_name(tr.shape, tr.B, tr.path, tr.problem) == "fused_mfma"
    assert gt.shape == (4,) and val_data.shape == (49, 2)
    assert len(eig) == len(norms) == 2
    for e, n in zip(eig, norms):
        assert e.shape == (4,) and n.shape == (4,) and np.isfinite(e).all() and np.isfinite(n).all() and (n > 0).all()
    for n, p in method.named_parameters():
        assert torch.isfinite(p).all(), n


# ---------------------------------------------------------------------------- 7. NeuralEF
def test_neuralef_takes_the_new_potentials_and_refuses_fokker_planck():
    """nsvd_nef_operator_forward evaluates V through the shared nsvd_potential (cosine, no importance: phi, Tphi finite
    and Tphi's potential term present) and refuses the Fokker-Planck kind."""
    L, D, m, hidden, B = 4, 2, 16, (32, 32), 48
    shape = H.ModelShape(L=L, D=D, m=m, hidden=hidden)
    p = O.init_params(L, D, m, hidden, 0.2, seed=3)
    ws_t, bs_t, fB, sc = to_dev(p)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    x = (PI32 * (2 * torch.rand(B, D, generator=torch.Generator().manual_seed(1)) - 1)).to(DEV)

    def run(prob):
        nb, nu = torch.ones(L, device=DEV), torch.ones(L, device=DEV)
        init = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = H.nef_operator_forward(shape, params, prob, x, H.new_workspace(shape, B, DEV), nb, nu, init, 0.9)
        torch.cuda.synchronize()
        return out

    cos = dict(pot_coef=(0.8, 0.9), importance_kind=H.IMP_NONE)
    phi, Tphi, _ = run(H.make_problem(H.POT_COSINE, 0.0, 0.01, 1.0, 0.0, 1.0, **cos))
    phi0, Tphi0, _ = run(H.make_problem(H.POT_ZERO, 0.0, 0.01, 1.0, 0.0, 1.0, importance_kind=H.IMP_NONE))
    assert torch.equal(phi, phi0) and bool(torch.isfinite(Tphi).all())
    V = (torch.cos(x.double().cpu()) * torch.tensor([float(np.float32(0.8)), float(np.float32(0.9))])).sum(-1, keepdim=True)
    # Tphi = Tphi(V = 0) - V phi: the float32 rounding of the two O(|Tphi|) terms it is the difference of
    got, want = (Tphi0.double().cpu() - Tphi.double().cpu()), V * phi.double().cpu()
    assert float((got - want).abs().max()) <= 4 * 2.0 ** -24 * float(Tphi0.abs().max() + Tphi.abs().max())
    with pytest.raises(H.NsvdError, match="unsupported"):
        run(H.make_problem(H.POT_SIN_OF_COS, 0.0, 0.01, 1.0, 0.0, 1.0, importance_kind=H.IMP_NONE,
                           operator_kind=H.OP_FOKKER_PLANCK, fp_scale=1.0, pot_coef=(1.0, 1.0)))
