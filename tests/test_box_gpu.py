"""Bounded-domain problems on the GPU: the Dirichlet box mask (alone and inside the exponential mask), the uniform
density / device sampler and V = 0 in every operator path, against the reference's float64 run (tests/golden/box.npz)
and the float64 restatement tests/_box_oracle.py.

Rows are measured in two groups, never pooled: WALL rows (some stencil point clamped or outside the box: the kink makes
their Tf ~ f / eps) and INTERIOR rows - one relative norm over both would let the wall rows hide a broken interior.
Bounds are test_hip_parity.test_operator_forward_backward_small's: f 2e-5, Tf 1e-4 per group, gradients 3e-5 given the
oracle's d loss / d f, 1e-4 end to end, the loss 1e-4 relative; exact mode holds Tf to 2e-5 (test_exact_laplacian_mode)."""
import argparse
import ast
import os

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _golden as G

pytestmark = pytest.mark.gpu

H = None
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box.npz")
CASES = ("iw_sqrt", "iw_exp", "box_expmask", "iw_exact_sqrt", "iw_exact_exp", "iw_1d", "iw_3d_exact")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import hip_ops
    H = hip_ops
    yield


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _path(name):
    return {"generic": H.PATH_GENERIC, "auto": H.PATH_AUTO, "bf16x3": H.PATH_FUSED_BF16X3}[name]


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().numpy()
    b = np.asarray(torch.as_tensor(b).double().cpu().numpy())
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def case_setup(z, name):
    cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
    names = [str(n) for n in z[f"{name}_param_names"]]
    t = lambda n: torch.tensor(z[f"{name}_param0_{n}"])  # noqa: E731
    sc = [t(n) for n in names if n.endswith("scales")]
    p = O.Params([t(n) for n in names if ".ws." in n], [t(n) for n in names if ".bs." in n],
                 torch.tensor(z[f"{name}_fourier_B"]), sc[0] if sc else None)
    return cfg, names, p, BO.problem_of(cfg)


def to_dev(p: O.Params):
    ws = [w.float().to(DEV).contiguous() for w in p.ws]
    bs = [b.float().to(DEV).contiguous() for b in p.bs]
    sc = None if p.scales is None else p.scales.float().to(DEV).contiguous()
    return ws, bs, p.fourier_B.float().to(DEV).contiguous(), sc


def shape_of(p: O.Params, prob: BO.Problem):
    L, h0, F = p.ws[0].shape
    return H.ModelShape(L=L, D=p.fourier_B.shape[0], m=F // 2, hidden=tuple(w.shape[1] for w in p.ws[:-1]),
                        has_exp_mask=p.scales is not None, box_mask=prob.box_mode, box_lim=prob.box_lim)


def hip_problem(prob: BO.Problem):
    return H.make_problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                          prob.scale_kinetic, prob.hard_mul_const, importance_kind=prob.importance)


def run_hip(p, prob, x, v, M, path, df_override=None):
    """test_hip_parity.run_hip with the box mask in the shape and the density in the problem"""
    shape = shape_of(p, prob)
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
    """f and Tf of the wall rows and of the interior rows, each group against its own norm; rows outside the box: f = 0"""
    wall = BO.wall_rows(x.double(), prob)
    tf_tol = 1e-4 if prob.eps > 0 else 2e-5
    f64, Tf64 = torch.as_tensor(np.asarray(f64)), torch.as_tensor(np.asarray(Tf64))
    for group, rows in (("wall", wall), ("interior", ~wall)):
        if not bool(rows.any()):
            continue
        ef, eT = rel(r["f"].cpu()[rows], f64[rows]), rel(r["Tf"].cpu()[rows], Tf64[rows])
        print(f"{what} {group} rows ({int(rows.sum())}): f {ef:.2e} Tf {eT:.2e}")
        assert ef < 2e-5, (what, group, ef)
        assert eT < tf_tol, (what, group, eT)
    outside = (x.abs() >= prob.box_lim).any(dim=1)
    assert bool((r["f"].cpu()[outside] == 0).all()), what
    assert bool(torch.isfinite(r["f"]).all()) and bool(torch.isfinite(r["Tf"]).all())


# ---------------------------------------------------------------------------- 1. every fixture case on every path
@pytest.mark.parametrize("path", ["generic", "auto", "bf16x3"])
@pytest.mark.parametrize("case", CASES)
def test_fixture_cases(z, case, path):
    """The reference's float64 run of every case on the three path requests. The fixture's models (hidden 16,16) are
    shapes of the generic kernels: `auto` takes them there, the exact-Laplacian cases and the bf16x3 request exist on
    the MFMA kernels only and are REFUSED for these shapes (never computed without the mask) - the MFMA sites are held
    to the float64 restatement in test_epilogue_sites."""
    cfg, names, p, prob = case_setup(z, case)
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    x = torch.tensor(z[f"{case}_x"][0])
    shape, hp = shape_of(p, prob), hip_problem(prob)
    name = H.path_name(shape, x.shape[0], _path(path), hp)
    if prob.eps <= 0 or path == "bf16x3":
        assert name == ("unsupported" if prob.eps <= 0 else "generic")
        with pytest.raises(H.NsvdError, match="unsupported"):
            run_hip(p, prob, x, v, M, _path(path))
        return
    assert name == "generic"
    ref = BO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
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
def planted(x, prob):
    """rows 0-5 (exact mode: 0-1) on and around the wall, like the fixture's"""
    lim, eps = np.float32(prob.box_lim), np.float32(prob.eps)
    x = x.float().clone()
    last = x.shape[1] - 1
    x[:5] = torch.clamp(x[:5], min=-0.8 * float(lim), max=0.8 * float(lim))
    if prob.eps > 0:
        x[0, 0] = float(lim - eps / 2)
        x[1, last] = float(-lim + eps / 2)
        x[2, 0] = float(lim)
        x[3, last] = float(lim + eps / 2)
        x[4, :] = float(lim - eps / 2)
        x[4, last] = float(-lim + eps / 3)
        x[5, :] = float(2 * lim)
        x[5, 0] = float(-1.7 * lim)
    else:
        x[0, 0] = float(lim - np.float32(1e-3))
        x[1, last] = float(1.5 * lim)
    return x


# site: (D, L, B, m, hidden, eps). hyd_med: test_operator_headline_shapes' shape (split form + epilogue kernel);
# ksplit: the K-split shape whose last-arriving direction group forms f, Tf inside the forward; split3d: 7 stencil
# columns, epilogue kernel; fused5: more than 128 workgroups, and fused3: D = 1 (the E = 3 instance) - f, Tf in the
# forward's own epilogue; exact2d / exact3d: the jets' epilogue
SITES = dict(
    hyd_med=(2, 4, 64, 64, (128, 128, 128), 0.01),
    ksplit=(2, 16, 128, 256, (128, 128, 128), 0.01),
    split3d=(3, 3, 96, 64, (128, 128, 128), 0.01),
    fused5=(2, 8, 544, 64, (128, 128), 0.01),
    fused3=(1, 3, 64, 64, (128, 128), 0.01),
    exact2d=(2, 4, 64, 64, (128, 128, 128), 0.0),
    exact3d=(3, 2, 64, 64, (128, 128), 0.0),
)
SITE_RUNS = [(s, "auto") for s in SITES] + [("fused5", "bf16x3"), ("ksplit", "bf16x3"), ("exact2d", "bf16x3")]


@pytest.mark.parametrize("combo", ["box", "box_expmask_gauss"])
@pytest.mark.parametrize("mode", ["sqrt", "exp"])
@pytest.mark.parametrize("site,path", SITE_RUNS)
def test_epilogue_sites(site, path, mode, combo):
    """box alone (uniform density, V = 0) and box x exponential mask x Gaussian importance (oscillator) at every place
    the MFMA kernels form f, Tf, against the float64 restatement; the planted rows are always in the batch."""
    D, L, B, m, hidden, eps = SITES[site]
    lim = 4.0
    kind = BO.BOX_SQRT if mode == "sqrt" else BO.BOX_EXP
    if combo == "box":
        prob = BO.Problem(potential=BO.POT_ZERO, eps=eps, op_scale=1.0, op_shift=0.0, sigma=lim, hard_mul_const=0.9,
                          importance=BO.IMP_UNIFORM, box_mode=kind, box_lim=lim)
        mask_init = None
    else:
        prob = BO.Problem(potential=O.POT_HARMONIC, eps=eps, op_scale=1.0, op_shift=16.0, sigma=3.0,
                          importance=BO.IMP_GAUSSIAN, box_mode=kind, box_lim=lim)
        mask_init = 4.0
    if site == "hyd_med":  # weights from the seed recipe of the golden case
        zz = G.load("model_headline")
        c = dict(G.cfg_of(zz, "hyd_med"), apply_exp_mask=int(mask_init is not None), exp_mask_init_scale=mask_init)
        p = G.params_from_seed(c)
    else:
        p = O.init_params(L, D, m, hidden, 0.2, exp_mask_init=mask_init, seed=44)
    g = torch.Generator().manual_seed(9)
    if combo == "box":
        x = lim * (2 * torch.rand(B, D, generator=g) - 1)
    else:
        x = 3.0 * torch.randn(B, D, generator=g)
    x = planted(x, prob)
    v, M = O.sequential_nesting_masks(L)
    ref = BO.loss_and_grads(x.double(), p.to(torch.float64), prob, v, M)
    r = run_hip(p, prob, x, v, M, _path(path), df_override=ref["df"])
    assert r["path"] == "fused_mfma", r["path"]  # (never the generic kernels)
    check_rows(r, ref["f"], ref["Tf"], x, prob, f"{site}/{path}/{mode}/{combo}")
    for i, (a, b) in enumerate(zip(r["grads"], ref["grads"])):
        assert torch.isfinite(a).all(), i
        assert rel(a.view(-1), b.reshape(-1)) < 3e-5, (i, rel(a.view(-1), b.reshape(-1)))


# ---------------------------------------------------------------------------- 3. WaveFunctions(x) and its autograd
@pytest.mark.parametrize("inside_exp_mask", [False, True])
@pytest.mark.parametrize("mode", ["dir_box_sqrt", "dir_box_exp"])
@pytest.mark.parametrize("D,L,B,m,hidden", [(2, 4, 24, 8, (16, 16)), (2, 4, 96, 64, (128, 128)), (3, 16, 2048, 64, (128, 128))])
def test_wavefunctions_forward_backward(D, L, B, m, hidden, mode, inside_exp_mask):
    """model(x) = c base mask M through nsvd_model_forward / _backward: the generic kernels, the MFMA plain tile and (the
    last shape) the streaming plain forward; x has rows on the wall, outside and within 1e-3 of it."""
    from neural_svd_amd.models import (DirichletBoundaryMaskBox, ExponentialMask, GaussianFourierFeatureTransform,
                                       ParallelMLP, WaveFunctions)
    lim, c = 3.0, 0.7
    torch.manual_seed(D * 100 + L)
    fm = GaussianFourierFeatureTransform(D, mapping_size=m, scale=0.05)
    base = ParallelMLP(D, list(hidden), 1, L, "softplus", bias=True, feature_map=fm)
    box = DirichletBoundaryMaskBox(lim, mode)
    bm = ExponentialMask(L, init_scale=6.0, boundary_mask=box) if inside_exp_mask else box
    model = WaveFunctions(base, bm, hard_mul_const=c).to(DEV)
    assert model.shape.box_mask == box.kind and model.shape.has_exp_mask == inside_exp_mask
    g = torch.Generator().manual_seed(B)
    x = 1.2 * lim * (2 * torch.rand(B, D, generator=g) - 1)
    x[0, 0], x[1, D - 1], x[2, 0], x[3, :] = lim, -lim - 0.5, lim - 1e-3, -lim + 1e-3
    dout = torch.randn(B, L, generator=g)
    out = model(x.to(DEV))
    out.backward(dout.to(DEV))
    # float64: the oracle's pieces with autograd
    leaves = [t.detach().double().cpu().clone().requires_grad_(True) for t in model.trainable_tensors()]
    nl = len(hidden) + 1
    q = O.Params(leaves[:nl], leaves[nl:2 * nl], fm._B.detach().double().cpu(), leaves[2 * nl] if inside_exp_mask else None)
    prob = BO.Problem(hard_mul_const=c, box_mode=box.kind, box_lim=lim)
    want = BO.wave(x.double(), q, prob)
    (want * dout.double()).sum().backward()
    inside = (x.abs() < lim).all(dim=1)
    assert bool((out.detach().cpu()[~inside] == 0).all()) and bool(inside.any()) and bool((~inside).any())
    assert rel(out, want.detach()) < 1e-5
    for i, (t, leaf) in enumerate(zip(model.trainable_tensors(), leaves)):
        assert t.grad is not None and torch.isfinite(t.grad).all()
        assert rel(t.grad, leaf.grad) < 3e-5, (i, rel(t.grad, leaf.grad))
    # the torch forward of the mask (foreign callers) is the same function
    assert rel(box(x.to(DEV)), BO.box_mask(x.double(), prob)) < 1e-6


# ---------------------------------------------------------------------------- 4. the uniform device sampler
@pytest.mark.parametrize("hidden", [(128,), (16,)])
def test_uniform_device_sampler(hidden):
    """nsvd_operator_sample_features with NSVD_IMP_UNIFORM: s (2 u - 1) strictly inside (-s, s), the moments of the
    uniform density, a pure function of (seed, offset); values 0 and 1 draw the unchanged Gaussian (MFMA path: inside
    the feature kernel; generic path: the stand-alone sampler)."""
    B, D, m, s = 65536, 2, 64, 5.0
    shape = H.ModelShape(L=1, D=D, m=m, hidden=hidden, box_mask=H.BOX_SQRT, box_lim=s)
    p = O.init_params(1, D, m, hidden, 0.1, seed=1)
    ws_t, bs_t, fB, sc = to_dev(p)
    params = H.pack_params(shape, ws_t, bs_t, fB, sc)
    prob = H.make_problem(H.POT_ZERO, 0.0, 0.01, 1.0, 0.0, s, importance_kind=H.IMP_UNIFORM)
    ws = H.new_workspace(shape, B, DEV)
    x = torch.empty(B, D, device=DEV)
    H.operator_sample_features(shape, params, prob, 1234, 7, x, ws)
    f1, Tf1 = H.operator_forward(shape, params, prob, x, ws, features_ready=True)
    xs = x.double().cpu()
    assert float(xs.abs().max()) < s
    for d in range(D):
        assert abs(float(xs[:, d].mean())) < 6 * s / np.sqrt(3 * B)
        # var of the sample variance of U(-s, s): (mu4 - sigma^4) / B = (s^4 / 5 - s^4 / 9) / B
        assert abs(float(xs[:, d].var()) - s * s / 3) < 6 * np.sqrt((s ** 4 / 5 - s ** 4 / 9) / B)
    assert abs(float((xs[:, 0] * xs[:, 1]).mean())) < 6 * (s * s / 3) / np.sqrt(B)
    x2 = torch.empty_like(x)
    H.operator_sample_features(shape, params, prob, 1234, 7, x2, ws)
    assert torch.equal(x, x2)
    H.operator_sample_features(shape, params, prob, 1234, 8, x2, ws)
    assert not torch.equal(x, x2) and float((x != x2).double().mean()) > 0.99
    # the features written next to the draw are those of that x
    f2, Tf2 = H.operator_forward(shape, params, prob, x, H.new_workspace(shape, B, DEV))
    assert torch.equal(f1, f2) and torch.equal(Tf1, Tf2)
    # values 0 and 1: the Gaussian draw of test_device_sampler, whatever the box mask
    sigma = 16.0
    xg, xn = torch.empty_like(x), torch.empty_like(x)
    H.operator_sample_features(shape, params, H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, sigma), 1234, 7, xg, ws)
    H.operator_sample_features(shape, params, H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, sigma,
                                                             use_importance=False), 1234, 7, xn, ws)
    plain = H.ModelShape(L=1, D=D, m=m, hidden=hidden)
    xp = torch.empty_like(x)
    H.operator_sample_features(plain, H.pack_params(plain, ws_t, bs_t, fB, sc),
                               H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, sigma), 1234, 7, xp,
                               H.new_workspace(plain, B, DEV))
    assert torch.equal(xg, xn) and torch.equal(xg, xp)
    zg = xg.double().cpu()
    n = zg.numel()
    assert abs(float(zg.mean())) < 5 * sigma / np.sqrt(n) and abs(float(zg.std()) / sigma - 1) < 5 / np.sqrt(2 * n)
    assert float(zg.abs().max()) > 3 * sigma  # (not a bounded draw)


# ---------------------------------------------------------------------------- 5. fused training steps
def _trainer_on_fixture(z, case, **kw):
    from neural_svd_amd.trainer import FusedTrainer
    cfg, names, p, prob = case_setup(z, case)
    shape = shape_of(p, prob)
    tr = FusedTrainer(shape, hip_problem(prob), cfg["batch_size"], sequential=True, step=1, lr=cfg["lr"],
                      rmsprop_decay=cfg["rmsprop_decay"], rmsprop_eps=1e-10, num_iters=cfg["num_iters"],
                      use_lr_scheduler=True, sampling_scale=cfg["sampling_scale"], seed=0, device=DEV,
                      device_sampler=False, exp_mask_init=None if p.scales is None else 1.0, **kw)
    tr.P.load(p.fourier_B, p.ws, p.bs, p.scales)  # (the constructor's own initial values are replaced)
    return cfg, names, tr


def test_fused_trainer_steps_on_the_fixture(z):
    """three FusedTrainer.step(x) calls on iw_sqrt's weights and recorded batches against the reference's float64
    parameters after its three steps, at the bound of test_train_operator_fused_loop_matches_plain_loop (RMSprop's
    early updates are sign-like: +-lr / sqrt(1 - alpha) whatever |g|); then the same three steps recorded into one HIP
    graph and replayed on a second trainer: equal bits."""
    case, n_steps = "iw_sqrt", 3
    cfg, names, tr = _trainer_on_fixture(z, case)
    xs = [torch.tensor(z[f"{case}_x"][it]).to(DEV).contiguous() for it in range(n_steps)]
    for it in range(n_steps):
        tr.step(xs[it])
        torch.cuda.synchronize()
        if it == 0:  # (from the second step on the two trajectories differ by the sign-like updates)
            assert rel(tr.f, z[f"{case}_f64_step0_f"]) < 2e-5
            l64 = float(z[f"{case}_f64_step0_loss"])
            assert abs(float(tr.loss[0]) - l64) < 1e-4 * abs(l64)
    upd = n_steps * cfg["lr"] / np.sqrt(1.0 - cfg["rmsprop_decay"])
    for n, got in zip(names, tr.P.views(tr.P.flat)):
        want = torch.tensor(z[f"{case}_f64_step{n_steps - 1}_param_{n}"])
        err = float((got.double().cpu() - want).norm())
        assert err <= 2e-3 * (float(want.norm()) + upd * np.sqrt(want.numel())), (n, err)
    # the same steps from a captured graph (host schedule: each step's learning rate is its launch argument)
    _, _, g = _trainer_on_fixture(z, case)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for it in range(n_steps):
                g.step(xs[it])
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for name in ("flat", "sq", "ema"):
        assert torch.equal(getattr(tr.P, name), getattr(g.P, name)), name
    assert torch.equal(tr.f, g.f) and torch.equal(tr.Tf, g.Tf)


def test_graphed_steps_with_the_uniform_device_sampler():
    """an MFMA shape with the box mask and the uniform density: FusedTrainer.capture_graph (device-resident schedule,
    the next batch drawn by the backward's guest workgroups) against the same number of eager steps, equal bits; every
    batch drawn lies strictly inside the box."""
    from neural_svd_amd.trainer import FusedTrainer
    lim = 5.0
    shape = H.ModelShape(L=4, D=2, m=64, hidden=(128, 128, 128), box_mask=H.BOX_SQRT, box_lim=lim)
    prob = H.make_problem(H.POT_ZERO, 0.0, 0.01, 1.0, 0.0, lim, importance_kind=H.IMP_UNIFORM)

    def make(sched):
        return FusedTrainer(shape, prob, 64, sequential=True, lr=1e-3, num_iters=60, seed=4, device=DEV,
                            sampling_scale=lim, fourier_scale=0.1, device_schedule=sched)
    a, g = make(False), make(True)
    assert a.guest_features and g.guest_features
    gs = g.capture_graph(2)
    gs.replay(5)
    for _ in range(g.t):
        a.step()
        assert float(a.x.abs().max()) < lim
    torch.cuda.synchronize()
    for name in ("flat", "sq", "ema"):
        assert torch.equal(getattr(a.P, name), getattr(g.P, name)), name
    assert torch.equal(a.x, g.x) and torch.equal(a.f, g.f) and torch.equal(a.Tf, g.Tf)
    assert bool(torch.isfinite(a.P.flat).all()) and float(a.f.abs().max()) > 0
    # the host sampler of the same trainer draws from the same density
    b = FusedTrainer(shape, prob, 64, sequential=True, seed=4, device=DEV, sampling_scale=lim, device_sampler=False)
    xb = b.sample()
    assert float(xb.abs().max()) <= lim and float(xb.abs().max()) > 0.8 * lim


# ---------------------------------------------------------------------------- 6. compute_spectrum_evd
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
    from neural_svd_amd.operators import (NegativeHamiltonian, OperatorWrapper, get_dataloader, get_problem,
                                          infinite_well_potential)
    args = _args(cfg)
    torch.manual_seed(cfg["seed"])
    if cfg["ndim"] == 2:
        operator, gt = get_problem(args, DEV)
    else:  # (get_problem asserts ndim == 2 for the well, like the reference)
        args.n_particles = 1
        operator, gt = OperatorWrapper(NegativeHamiltonian(infinite_well_potential, 1.0, args.laplacian_eps, 1),
                                       scale=args.operator_scale, shift=args.operator_shift), None
    method = get_evd_method(args, "neuralsvd", get_wavefunctions(args)).to(DEV)
    return args, operator, gt, method, get_dataloader(args, DEV)


@pytest.mark.parametrize("case", ["iw_sqrt", "iw_exp", "box_expmask", "iw_1d"])
def test_spectrum_matches_the_fixture(z, case):
    """compute_spectrum_evd on the fixture's grid with the parameters the reference evaluated (after its third step):
    norms and eigenvalues at test_spectrum_matches_reference's bound."""
    from neural_svd_amd.spectrum import compute_spectrum_evd
    cfg = ast.literal_eval(str(z[f"{case}_cfg"]))
    args, operator, gt, method, (_, val_data, batch_ftn_val, imp_train, imp_val) = _build(cfg)
    with torch.no_grad():
        for n, t in method.named_parameters():
            if t.requires_grad:
                t.copy_(torch.tensor(z[f"{case}_f64_step2_param_{n}"]).float())
            elif n.endswith("feature_map._B"):
                t.copy_(torch.tensor(z[f"{case}_fourier_B"]))
    assert np.array_equal(val_data.cpu().numpy(), z[f"{case}_val_data"])
    method.eval()
    out = compute_spectrum_evd(method, dataloader=batch_ftn_val(), operator=operator, importance_train=imp_train,
                               importance_val=imp_val, normalize=True, device=DEV)
    assert rel(out["norms"], z[f"{case}_f64_spec_norms"]) < 1e-4
    e64, e32 = z[f"{case}_f64_spec_eigvals"], z[f"{case}_f32_spec_eigvals"]
    ref_err = float(np.max(np.abs(e32 - e64) / np.abs(e64)))
    got_err = float(np.max(np.abs(out["eigvals"] - e64) / np.abs(e64)))
    print(f"{case} eigvals {got_err:.2e} (float32 reference {ref_err:.2e})")
    assert got_err < max(3 * ref_err, 1e-4), (got_err, ref_err)
    # FusedTrainer.spectrum (its own grid and row weighting) on the same weights
    if cfg["ndim"] == 2:
        _, names, tr = _trainer_on_fixture(z, case)
        p = [torch.tensor(z[f"{case}_f64_step2_param_{n}"]).float() for n in names]
        nl = len([n for n in names if ".ws." in n])
        tr.P.load(torch.tensor(z[f"{case}_fourier_B"]), p[:nl], p[nl:2 * nl], p[2 * nl] if len(p) > 2 * nl else None)
        s = tr.spectrum(cfg["lim"], cfg["val_eps"], use_ema=False, chunk=150)
        assert float(np.max(np.abs(s["eigvals"].numpy() - e64) / np.abs(e64))) < max(3 * ref_err, 1e-4)
        assert rel(s["norms"], z[f"{case}_f64_spec_norms"]) < 1e-4


# ---------------------------------------------------------------------------- 7. drop-in
WELL_ARGS = dict(seed=0, ndim=2, n_particles=1, neigs=4, mlp_hidden_dims="128,128,128", nonlinearity="softplus", parallel=1,
                 weight_normalization=0, use_fourier_feature=True, fourier_mapping_size=64, fourier_scale=0.1,
                 fourier_deterministic=False, fourier_append_raw=False, apply_boundary=1, boundary_mode="dir_box_sqrt",
                 lim=5.0, apply_exp_mask=0, exp_mask_init_scale=10.0, hard_mul_const=1.0, problem="sch",
                 potential_type="infinite_well", charge=1.0, laplacian_eps=0.01, operator_scale=1.0, operator_shift=0.0,
                 sampling_mode="uniform", sampling_scale=5.0, batch_size=64, val_eps=1.0, optimizer="rmsprop", lr=1e-4,
                 rmsprop_decay=0.999, momentum=0.0, num_iters=20, sort=0)


def _train(over, spy=None):
    import neural_svd_amd.drop_in as DI
    args, operator, gt, method, (make_batch, val_data, batch_ftn_val, imp_train, imp_val) = _build(dict(WELL_ARGS, **over))
    args.eval_freq = args.num_iters // 2
    box = {}
    orig_fused, orig_cap = DI._fused_loop_trainer, DI.CapturedPlainStep

    def spy_fused(*a, **k):
        box["fused"] = orig_fused(*a, **k)
        return box["fused"]

    class SpyStep(orig_cap):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            box["captured"] = self

    DI._fused_loop_trainer, DI.CapturedPlainStep = spy_fused, SpyStep
    try:
        torch.manual_seed(123)
        eig, norms = DI.train_operator(args, method, operator, make_batch, val_data, batch_ftn_val, None, None, DEV,
                                       imp_train, imp_val, gt)
    finally:
        DI._fused_loop_trainer, DI.CapturedPlainStep = orig_fused, orig_cap
    return args, method, val_data, gt, eig, norms, box


def test_dropin_infinite_well_runs_the_fused_loop():
    """get_problem / get_wavefunctions / get_dataloader / get_evd_method / train_operator from a reference-style
    argument set: 20 iterations with two evaluations; the loop taken is FusedTrainer on the MFMA kernels."""
    from neural_svd_amd.trainer import FusedTrainer
    args, method, val_data, gt, eig, norms, box = _train({})
    tr = box["fused"]
    assert isinstance(tr, FusedTrainer) and "captured" not in box
    assert tr.t == 20 and tr.shape.box_mask == H.BOX_SQRT and tr.problem.use_importance == H.IMP_UNIFORM
    assert H.path_name(tr.shape, tr.B, tr.path, tr.problem) == "fused_mfma"
    assert gt.shape == (4,) and val_data.shape == (100, 2)
    assert len(eig) == len(norms) == 2
    for e, n in zip(eig, norms):
        assert e.shape == (4,) and n.shape == (4,) and np.isfinite(e).all() and np.isfinite(n).all() and (n > 0).all()
    for n, p in method.named_parameters():
        assert torch.isfinite(p).all(), n


def test_dropin_plain_loops_take_the_box_mask():
    """without the fused loop the captured plain loop (CapturedPlainStep: autograd around the HIP Functions, replayed
    from a HIP graph) takes the steps and agrees with its eager twin at test_train_operator_plain_loop_replayed_from_a_
    graph's bound; with --optimizer adam (neither loop implements it) the eager plain loop does."""
    res = {}
    iters = 8
    for graph in (True, False):
        args, method, _, _, eig, _, box = _train(dict(num_iters=iters, lr=1e-5, fused_loop=False, graph_loop=graph))
        assert box["fused"] is None and ("captured" in box) == graph
        if graph:
            assert box["captured"].steps == iters and box["captured"].graph is not None
        res[graph] = {n: p.detach().clone() for n, p in method.named_parameters() if p.requires_grad}, eig[-1]
    upd = iters * 1e-5 / np.sqrt(1.0 - 0.999)
    for n, a in res[True][0].items():
        b = res[False][0][n].double()
        assert float((a.double() - b).norm()) <= 2e-3 * (float(b.norm()) + upd * np.sqrt(b.numel())), n
    assert np.isfinite(res[True][1]).all() and np.isfinite(res[False][1]).all()
    args, method, _, _, eig, norms, box = _train(dict(num_iters=6, optimizer="adam", lr=1e-4))
    assert box["fused"] is None and "captured" not in box
    assert len(eig) == 2 and np.isfinite(eig[-1]).all()
    for n, p in method.named_parameters():
        assert torch.isfinite(p).all(), n


def test_use_amp_takes_the_box_mask():
    """use_amp selects NSVD_PATH_FUSED_BF16X3, which carries the box mask in the same epilogue: no refusal"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # (a grid of 8 x 8 = 64 rows: one whole batch)
        args, method, _, _, eig, _, box = _train(dict(num_iters=4, use_amp=True, val_eps=1.25))
    assert method.path == H.PATH_FUSED_BF16X3 and box["fused"] is not None and np.isfinite(eig[-1]).all()
