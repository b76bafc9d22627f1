"""The optimisers of the reference's PDE loop beside RMSprop without momentum (examples/utils.py:48-72: SGD with /
without momentum, RMSprop with momentum, Adam) on the GPU: the stand-alone kernel (host scalars and device-resident
schedule), the weight-gradient kernel's epilogue against separate calls, the bf16x3 planes, FusedTrainer and the drop-in
loops. Tolerance against the float64 oracle tests/_optim_oracle.py: rel < 1e-6 on p, every state slot and the EMA - what
tests/test_hip_parity.py holds the float32 RMSprop kernel to; fused against unfused: the same bits."""
import argparse  # noqa: F401

import numpy as np
import pytest
import torch

from tests import _optim_oracle as OO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N, STEPS, T_MAX, LR0, ALPHA, DECAY, ADAM_EPS = 100003, 12, 30, 1e-3, 0.999, 0.995, 1e-8
RULES = [("sgd", 0.0), ("sgd", 0.9), ("rmsprop", 0.9), ("adam", 0.0)]


def trainer_lr(kind):
    """Learning rate of the FusedTrainer cases. RMSprop and Adam normalise the gradient and take 1e-3, the rate of
    test_optimiser_step_fused_into_backward_is_bit_identical. Plain SGD multiplies the raw gradient: at 1e-3 the float64
    oracle itself diverges on these problems (largest gradient element 7e2 at the first step of the (128, 128) / B = 160
    oscillator shape, 7e6 at the second, 1e60 at the fourth; the hydrogen shape overflows at its fifth step), and a run
    full of NaN compares unequal to itself. At 1e-5 the oracle's loss falls over the same steps (609 -> 333 -> 195 -> 156),
    with and without momentum 0.9."""
    return 1e-5 if kind == "sgd" else 1e-3


def rel(a, b):
    a = torch.as_tensor(a).double().cpu().numpy()
    b = np.asarray(torch.as_tensor(b).double().cpu().numpy())
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal(N).astype(np.float32)
    grads = np.stack([rng.standard_normal(N) * (1.0 + 0.3 * t) for t in range(STEPS)]).astype(np.float32)
    grads[:, 5000:6000] = 0.0  # elements that never see a gradient
    return p0, grads, torch.tensor(p0, device=DEV), torch.tensor(grads, device=DEV)


@pytest.fixture(scope="module")
def oracle(data):
    """the float64 runs, once per (rule, EMA)"""
    p0, grads = data[0].astype(np.float64), [g.astype(np.float64) for g in data[1]]
    out = {}
    for kind, mu in RULES:
        for with_ema in (True, False):
            out[kind, mu, with_ema] = OO.run(kind, mu, p0, grads, LR0, T_MAX, ALPHA, ADAM_EPS if kind == "adam" else 1e-10,
                                             (0.9, 0.999), DECAY if with_ema else None)
    return out


def _cfg(H, kind, mu):
    return H.opt_config(kind, LR0, ALPHA, ADAM_EPS if kind == "adam" else 1e-10, mu, (0.9, 0.999), DECAY)


def _buffers(H, cfg, kind, p0d, with_ema):
    uses_sq, uses_mom = H.opt_uses(cfg)
    sq = torch.zeros_like(p0d) if uses_sq else None
    # SGD's first step must not read the buffer: hand it garbage
    mom = (torch.full_like(p0d, 7.0) if kind == "sgd" else torch.zeros_like(p0d)) if uses_mom else None
    return p0d.clone(), sq, mom, (p0d.clone() if with_ema else None)


@pytest.mark.parametrize("with_ema", [True, False])
@pytest.mark.parametrize("kind,mu", RULES)
def test_standalone_kernel(data, oracle, kind, mu, with_ema):
    """nsvd_opt_step (host scalars) against the oracle over 12 steps of a cosine schedule, n odd (the vector tail runs);
    nsvd_opt_step_dev captured ONCE and replayed 12 times against the host-scalar form; one case with grad_scale."""
    from neural_svd_amd import hip_ops as H
    p0, grads, p0d, gd = data
    want = oracle[kind, mu, with_ema]
    cfg = _cfg(H, kind, mu)
    gs = 0.25 if (kind == "adam" and with_ema) else 1.0  # grad_scale 0.25 on 4 x gradients
    gin = gd / gs
    p, sq, mom, ema = _buffers(H, cfg, kind, p0d, with_ema)
    for t in range(STEPS):
        H.opt_step(cfg, p, gin[t], sq, mom, ema, t, lr=OO.cosine_lr(LR0, t, T_MAX),
                   ema_decay=OO.ema_decay_at(DECAY, t + 1), grad_scale=gs)
    torch.cuda.synchronize()
    figures = {"p": rel(p, want.p)}
    for name, got, ref in (("sq", sq, want.sq), ("mom", mom, want.mom), ("ema", ema, want.ema)):
        assert (got is None) == (ref is None), name
        if got is not None:
            figures[name] = rel(got, ref)
    print(kind, mu, with_ema, "host form vs float64:", figures)
    assert all(v < 1e-6 for v in figures.values()), figures
    assert torch.equal(p[5000:6000], p0d[5000:6000]) and bool(torch.isfinite(p).all())

    # device-resident schedule: captured once, replayed along the schedule
    pb, sqb, momb, emab = _buffers(H, cfg, kind, p0d, with_ema)
    st = H.OptState(DEV, cfg, T_MAX)
    gbuf = torch.empty_like(p0d)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            st.begin()
            H.opt_step_dev(pb, gbuf, sqb, momb, emab, st, gs, True)
    torch.cuda.current_stream().wait_stream(side)
    for t in range(STEPS):
        gbuf.copy_(gin[t])
        graph.replay()
    torch.cuda.synchronize()
    h = st.read()
    assert h.step == STEPS and h.mismatch == 0
    dev_figures = {n: rel(b, a) for n, a, b in (("p", p, pb), ("sq", sq, sqb), ("mom", mom, momb), ("ema", ema, emab))
                   if a is not None}
    print(kind, mu, with_ema, "device form vs host form:", dev_figures)
    assert all(v < 1e-6 for v in dev_figures.values()), dev_figures


def test_standalone_kernel_refuses_what_it_cannot_do(data):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    p = data[2].clone()
    g = torch.zeros_like(p)
    bad = _cfg(H, "adam", 0.0)
    bad.kind = 7
    with pytest.raises(NsvdError, match="NSVD_EINVAL"):
        H.opt_step(bad, p, g, torch.zeros_like(p), torch.zeros_like(p), None, 0)
    with pytest.raises(NsvdError, match="NSVD_EINVAL"):  # Adam without its first-moment slot
        H.opt_step(_cfg(H, "adam", 0.0), p, g, torch.zeros_like(p), None, None, 0)
    # a device state of another rule: the launch touches nothing and leaves a mark
    st = H.OptState(DEV, _cfg(H, "sgd", 0.9), T_MAX)
    st.cfg = _cfg(H, "adam", 0.0)
    sq, mom = torch.zeros_like(p), torch.zeros_like(p)
    H.opt_step_dev(p, torch.ones_like(p), sq, mom, None, st)
    torch.cuda.synchronize()
    h = st.read()
    assert h.mismatch == 1 and h.step == 0 and torch.equal(p, data[2]) and float(mom.abs().max()) == 0.0
    torch.cuda.synchronize()
    assert torch.equal(p, data[2])


# ------------------------------------------------------------------------- fused epilogue against separate calls
SHAPES = [((32, 32), 16, 24, False), ((128, 128, 128), 128, 64, True), ((128, 128), 64, 96, False),
          ((128, 128), 128, 1024, True), ((128, 128), 64, 160, False)]
FUSED_CASES = [(k, mu, i) for k, mu in (("adam", 0.0), ("rmsprop", 0.9)) for i in range(5)] + \
              [(k, mu, i) for k, mu in (("sgd", 0.0), ("sgd", 0.9)) for i in (0, 4)]


def _three(kind, mu, shape_index, **extra):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.trainer import FusedTrainer
    hidden, m, B, mask = SHAPES[shape_index]
    shape = H.ModelShape(L=4, D=2, m=m, hidden=hidden, has_exp_mask=mask)
    prob = H.make_problem(H.POT_HARMONIC, 1.0, 0.01, 1.0, 16.0, 4.0)
    kw = dict(sequential=False, lr=trainer_lr(kind), num_iters=50, sampling_scale=4.0, fourier_scale=0.15,
              exp_mask_init=10.0 if mask else None, seed=2, device=DEV, optimizer=kind, momentum=mu, **extra)
    a = FusedTrainer(shape, prob, B, fused_step=True, **kw)
    b = FusedTrainer(shape, prob, B, fused_step=False, **kw)
    c = FusedTrainer(shape, prob, B, fused_step=True, keep_grads=True, **kw)
    return H, shape, B, a, b, c


def _state_names(tr):
    return ["flat", "ema"] + (["sq"] if tr._uses_sq else []) + (["mom"] if tr._uses_mom else [])


@pytest.mark.parametrize("kind,mu,shape_index", FUSED_CASES)
def test_fused_epilogue_is_bit_identical_to_separate_calls(kind, mu, shape_index):
    """nsvd_operator_backward_evd_opt_step (the rule inside the weight-gradient kernel's epilogue, gradients never
    stored) against nsvd_operator_backward_evd + nsvd_opt_step: parameters, every state slot, the EMA shadow and the
    loss bit for bit after four steps, on the generic path, the MFMA path and its split-K form (last shape)."""
    H, shape, B, a, b, c = _three(kind, mu, shape_index)
    assert a.fused_step and not b.fused_step and (a.P.mom is not None) == (kind != "sgd" or mu != 0.0)
    for _ in range(4):
        x = b.sample().clone()
        a.step(x)
        b.step(x)
        c.step(x)
    torch.cuda.synchronize()
    for name in _state_names(a):
        assert bool(torch.isfinite(getattr(b.P, name)).all()), name  # (a diverged run would compare unequal to itself)
        assert torch.equal(getattr(a.P, name), getattr(b.P, name)), name
        assert torch.equal(getattr(c.P, name), getattr(b.P, name)), name
    assert float((a.P.flat - a.P.ema).abs().max()) > 0  # (the parameters did move)
    assert torch.equal(c.P.grad, b.P.grad)
    if H.path_name(shape, B) == "fused_mfma":
        assert float(a.P.grad.abs().max()) == 0.0  # never written
    assert torch.equal(a.loss, b.loss) and a.t == b.t == 4 and a.num_updates == b.num_updates == 4


@pytest.mark.parametrize("shape_index", [0, 1, 4])
def test_rmsprop_through_the_new_entry_point_is_the_old_entry_point(shape_index):
    """NSVD_OPT_RMSPROP without momentum given to nsvd_operator_backward_evd_opt_step takes the kernels of
    nsvd_operator_backward_evd_step: the same bits"""
    H, shape, B, a, b, c = _three("rmsprop", 0.0, shape_index)
    assert not a._other_rule and a.P.mom is None
    c._other_rule = True  # this trainer's fused step goes through the new entry point
    for _ in range(4):
        x = b.sample().clone()
        a.step(x)
        b.step(x)
        c.step(x)
    torch.cuda.synchronize()
    assert c._opt_desc is not None and a._opt_desc is None
    for name in ("flat", "sq", "ema"):
        assert torch.equal(getattr(a.P, name), getattr(c.P, name)), name
        assert torch.equal(getattr(a.P, name), getattr(b.P, name)), name
    assert torch.equal(a.loss, c.loss)


# ------------------------------------------------------------------------------------------------------ bf16x3
def _hydrogen(kind, mu, device_schedule=False, L=4, m=64, B=64, **kw):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.trainer import FusedTrainer
    shape = H.ModelShape(L=L, D=2, m=m, hidden=(128, 128, 128))
    prob = H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, 16.0)
    return FusedTrainer(shape, prob, B, sequential=False, lr=trainer_lr(kind), num_iters=60, seed=4, device=DEV,
                        device_schedule=device_schedule, sampling_scale=16.0, fourier_scale=0.1, optimizer=kind,
                        momentum=mu, **kw)


def _same(a, b):
    for name in _state_names(a):
        assert bool(torch.isfinite(getattr(b.P, name)).all()), name
        assert torch.equal(getattr(a.P, name), getattr(b.P, name)), name
    assert torch.equal(a.x, b.x) and torch.equal(a.f, b.f) and torch.equal(a.Tf, b.Tf)
    assert torch.equal(a.loss, b.loss)


@pytest.mark.parametrize("kind,mu", RULES)
def test_bf16x3_planes_are_those_of_the_updated_weights(kind, mu):
    """three bf16x3 steps: the planes the epilogue of every rule leaves for the next forward are a fresh split of the
    updated weights (a trainer whose forwards always split gets the same bits)"""
    from neural_svd_amd import hip_ops as H
    a, b = _hydrogen(kind, mu), _hydrogen(kind, mu)
    a.path = b.path = H.PATH_FUSED_BF16X3
    assert H.step_emits_planes(a.shape, a.B, a.path)
    b._note_planes = lambda ws: None  # never claims the planes: every forward of b splits the weights itself
    used = 0
    for _ in range(3):
        a.step()
        b.step()
        used += a._planes_ws is not None
    # a fourth forward on each: a reads the planes of the third step's weights, b splits them
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert used == 3 and b._planes_ws is None
    _same(a, b)


@pytest.mark.parametrize("kind,mu", [("adam", 0.0), ("sgd", 0.9)])
def test_graph_replay_moves_the_bias_corrections_and_the_first_step_flag(kind, mu):
    """device_schedule=True: steps captured into a HIP graph and replayed are the eager device-schedule steps bit for
    bit, and the host-schedule steps at rel < 1e-6 (the device pow / cos may differ from libm's in the last bit)"""
    g, e, h = _hydrogen(kind, mu, True), _hydrogen(kind, mu, True), _hydrogen(kind, mu, False)
    gs = g.capture_graph(2)
    pre = g.t
    gs.replay(4)
    for _ in range(pre + 8):
        e.step()
        h.step()
    torch.cuda.synchronize()
    assert g.t == e.t == pre + 8 and g.state.read().step == pre + 8
    _same(e, g)
    for name in _state_names(h):
        assert rel(getattr(e.P, name), getattr(h.P, name)) < 1e-6, name


# ------------------------------------------------------------------------------------------------ FusedTrainer
def test_fused_trainer_adam_learns_and_round_trips():
    """the oscillator smoke shape of test_fused_trainer_learns_oscillator, 300 Adam steps: the loss falls, the weights
    stay finite; state_dict + optimizer_state_dict into a new trainer, one more step on both: the same bits"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.trainer import FusedTrainer
    shape = H.ModelShape(L=6, D=2, m=64, hidden=(64, 64, 64), has_exp_mask=True)
    prob = H.make_problem(H.POT_HARMONIC, 1.0, 0.01, 1.0, 16.0, 4.0)
    kw = dict(sequential=True, lr=1e-3, num_iters=4000, sampling_scale=4.0, fourier_scale=0.15, exp_mask_init=10.0,
              device=DEV, optimizer="adam")
    tr = FusedTrainer(shape, prob, 256, seed=0, **kw)
    assert tr.P.mom is not None
    losses = []
    for _ in range(300):
        tr.step()
        losses.append(tr.loss[0].clone())
    losses = torch.stack(losses).cpu().numpy()
    first, last = float(np.median(losses[:30])), float(np.median(losses[-30:]))
    print("adam: median loss of the first / last 30 steps:", first, last)
    assert last < first and np.isfinite(losses).all()
    for name in ("flat", "sq", "mom", "ema"):
        assert bool(torch.isfinite(getattr(tr.P, name)).all()), name
    sd, ema_sd, osd = tr.state_dict(), tr.state_dict(ema=True), tr.optimizer_state_dict()
    new = FusedTrainer(shape, prob, 256, seed=1, **kw)
    new.P.load_state_dict(sd, ema_sd, reset_optimizer=False)
    new.load_optimizer_state_dict(osd)
    assert new.t == tr.t == 300
    x = tr.sample().clone()
    tr.step(x)
    new.step(x)
    torch.cuda.synchronize()
    for name in ("flat", "sq", "mom", "ema"):
        assert torch.equal(getattr(tr.P, name), getattr(new.P, name)), name
    assert torch.equal(tr.loss, new.loss)
    with pytest.raises(ValueError, match="optimizer state"):
        FusedTrainer(shape, prob, 256, seed=1, **dict(kw, optimizer="sgd", momentum=0.9)).load_optimizer_state_dict(osd)


# ----------------------------------------------------------------------------------------------------- drop-in
# tests/test_box_gpu.py's WELL_ARGS
WELL_ARGS = dict(seed=0, ndim=2, n_particles=1, neigs=4, mlp_hidden_dims="128,128,128", nonlinearity="softplus", parallel=1,
                 weight_normalization=0, use_fourier_feature=True, fourier_mapping_size=64, fourier_scale=0.1,
                 fourier_deterministic=False, fourier_append_raw=False, apply_boundary=1, boundary_mode="dir_box_sqrt",
                 lim=5.0, apply_exp_mask=0, exp_mask_init_scale=10.0, hard_mul_const=1.0, problem="sch",
                 potential_type="infinite_well", charge=1.0, laplacian_eps=0.01, operator_scale=1.0, operator_shift=0.0,
                 sampling_mode="uniform", sampling_scale=5.0, batch_size=64, val_eps=1.0, optimizer="rmsprop", lr=1e-4,
                 rmsprop_decay=0.999, momentum=0.0, num_iters=20, sort=0)
DROPIN = [("adam", 0.0), ("sgd", 0.9), ("rmsprop", 0.9)]


def _train(over):
    import neural_svd_amd.drop_in as DI
    import tests.test_box_gpu as TB
    from neural_svd_amd import hip_ops
    TB.H = hip_ops  # (that module's autouse fixture does this for its own tests)
    args, operator, gt, method, (make_batch, val_data, batch_ftn_val, imp_train, imp_val) = \
        TB._build(dict(WELL_ARGS, **over))
    args.eval_freq = args.num_iters // 2
    box = {}
    orig_fused, orig_cap, orig_get = DI._fused_loop_trainer, DI.CapturedPlainStep, DI.get_optimizer

    def spy_fused(*a, **k):
        box["fused"] = orig_fused(*a, **k)
        return box["fused"]

    class SpyStep(orig_cap):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            box["captured"] = self

    def spy_get(*a, **k):
        box["optimizer"] = orig_get(*a, **k)
        return box["optimizer"]

    DI._fused_loop_trainer, DI.CapturedPlainStep, DI.get_optimizer = spy_fused, SpyStep, spy_get
    try:
        torch.manual_seed(123)
        eig, _ = DI.train_operator(args, method, operator, make_batch, val_data, batch_ftn_val, None, None, DEV,
                                   imp_train, imp_val, gt)
    finally:
        DI._fused_loop_trainer, DI.CapturedPlainStep, DI.get_optimizer = orig_fused, orig_cap, orig_get
    return method, eig, box


def _check_torch_state(kind, mu, method, optimizer, steps):
    keys = {"adam": {"step", "exp_avg", "exp_avg_sq"}, "rmsprop": {"step", "square_avg", "momentum_buffer"},
            "sgd": {"momentum_buffer"}}[kind]
    n = 0
    for p in method.parameters():
        if not p.requires_grad:
            continue
        st = optimizer.state[p]
        assert set(st.keys()) == keys, (kind, set(st.keys()))
        for k in keys - {"step"}:
            assert st[k].shape == p.shape and bool(torch.isfinite(st[k]).all()) and float(st[k].abs().max()) > 0, k
        if "step" in keys:
            assert float(st["step"]) == steps
        n += 1
    assert n > 0


@pytest.mark.parametrize("kind,mu", DROPIN)
def test_dropin_fused_loop_takes_the_other_optimisers(kind, mu):
    """args.fused_optimizers: the loop taken is FusedTrainer; after 8 steps optimizer.state carries torch's own keys"""
    from neural_svd_amd.trainer import FusedTrainer
    method, eig, box = _train(dict(num_iters=8, lr=1e-5, optimizer=kind, momentum=mu, fused_optimizers=True))
    tr = box["fused"]
    assert isinstance(tr, FusedTrainer) and "captured" not in box and tr.t == 8
    assert tr.optimizer == kind and tr.momentum == mu
    _check_torch_state(kind, mu, method, box["optimizer"], 8)
    assert len(eig) == 2 and np.isfinite(eig[-1]).all()
    for n, p in method.named_parameters():
        assert torch.isfinite(p).all(), n


@pytest.mark.parametrize("kind,mu", DROPIN)
def test_dropin_captured_loop_takes_the_other_optimisers(kind, mu):
    """fused_loop=False: CapturedPlainStep takes the steps (state in torch.optim's own tensors) and agrees with its
    eager twin - torch.optim itself - at tests/test_box_gpu.py's bound for RMSprop"""
    iters = 8
    res = {}
    for graph in (True, False):
        method, eig, box = _train(dict(num_iters=iters, lr=1e-5, optimizer=kind, momentum=mu, fused_optimizers=True,
                                       fused_loop=False, graph_loop=graph))
        assert box["fused"] is None and ("captured" in box) == graph
        if graph:
            assert box["captured"].steps == iters and box["captured"].graph is not None
            assert box["captured"].state.read().step == iters
        _check_torch_state(kind, mu, method, box["optimizer"], iters)
        res[graph] = {n: p.detach().clone() for n, p in method.named_parameters() if p.requires_grad}, eig[-1]
    upd = iters * 1e-5 / np.sqrt(1.0 - 0.999)
    for n, a in res[True][0].items():
        b = res[False][0][n].double()
        err, bound = float((a.double() - b).norm()), 2e-3 * (float(b.norm()) + upd * np.sqrt(b.numel()))
        print(kind, mu, n, "captured vs eager:", err, "bound", bound)
        assert err <= bound, n
    assert np.isfinite(res[True][1]).all() and np.isfinite(res[False][1]).all()


def test_dropin_routing_without_the_switch_is_unchanged():
    """no args.fused_optimizers: adam takes neither fast loop, as before"""
    method, eig, box = _train(dict(num_iters=6, optimizer="adam", lr=1e-4))
    assert box["fused"] is None and "captured" not in box
    method, eig, box = _train(dict(num_iters=6, optimizer="rmsprop", momentum=0.9, lr=1e-4, fused_optimizers=False))
    assert box["fused"] is None and "captured" not in box
    assert np.isfinite(eig[-1]).all()
