"""Every CDK tower kernel instance and every option of the fused step against the float64 oracle (oracle/nsvd_oracle.py).

The tower and step kernels choose template instances and split counts from the shape (csrc/tower.hip launch_bn_forward /
launch_bn_backward, fwd2_slices, fwd2_slices16; csrc/tower_col.h nsvd_tcol::launch; csrc/cdk_step.hip with
csrc/cdk_narrow.hip). Each row below is derived from that selection code; the case named in it reaches the instance.

fp32 tower (nsvd_tower_forward / _backward). BatchNorm strip <STRIP, NT>: N >= 4096 -> <32, 512>, else B % 256 == 0 ->
<4, 256>, else <8, 256>; rows per thread = B / RG with RG = NT / (STRIP / 4) = 64, 256, 128. S = fwd2_slices(B, d1, d2):
doubled while S < 16, (B / 128)(d2 / 128) S < 256 and d1 % (64 S) == 0; tower_sum_slices_kernel adds 8 slices per pass.

  (B, d0, d1, d2)         BN1 (fwd + bwd)           BN2 (fwd + bwd)           S    reaches
  (384, 128, 256, 128)    <8, 256>, 3 rows/thread   <8, 256>, 3 rows          8    multi-row <8, 256>; K / S = 32
  (640, 256, 4096, 128)   <32, 512>, 10 rows        <8, 256>, 5 rows          16   <32, 512> below B = 1024; 2nd sum pass
  (896, 128, 1024, 256)   <8, 256>, 7 rows          <8, 256>, 7 rows          16   7 rows/thread; 2nd sum pass
  (1024, 128, 256, 4096)  <4, 256>, 4 rows          <32, 512>, 16 rows        1    one slice (256 tiles); d2 > d1
  (1024, 128, 128, 2048)  <4, 256>, 4 rows          <4, 256>, 4 rows          2    K = d1 = 128
  (256, 1024, 128, 256)   <4, 256>, 1 row           <4, 256>, 1 row           4    bottleneck d1 < d0

Mixed-precision tower (16-bit operands; nt = 1 tower per launch). Form "fused": tower_col_kernel<BWD, NI, PI, NBUF> by
B / 128 = 2 -> <2, 2, 3>, 4 -> <4, 4, 2>, 6 -> <6, 3, 2>, 8 -> <8, 4, 2>; forward K = d0, backward K = d2, in stages of
64. Form "strips" (NSVD_TOWER16_FUSED=0): gemm16 + tower_bn16 kernels. S16 = fwd2_slices16(nt, B, d1, d2): doubled while
S < 16, nt (B / 256)(d2 / 128) S < 256 and d1 % (128 S) == 0. BN2 is the fp32 strip above.

  (B, d0, d1, d2)         tower_col (fused form)            S16  BN2
  (768, 128, 256, 256)    <6, 3, 2>: fwd 2 stages, bwd 4    4    <4, 256>, 3 rows
  (768, 384, 1024, 768)   <6, 3, 2>: fwd 6 stages, bwd 12   16   <4, 256>, 3 rows
  (256, 128, 2048, 256)   <2, 2, 3>                         16   <4, 256>, 1 row
  (1024, 128, 256, 8192)  <8, 4, 2>                         1    <32, 512>, 16 rows

Fused step (FusedCdkStep -> nsvd_cdk_step; mixed precision: nt = 2, both towers per launch). The narrow end
(cdk_narrow.hip) runs when mixed and narrow_ok(2, B, d2): d2 <= 1024, d2 / 4 divides 256, 8 % (256 / (d2 / 4)) == 0 -
with d2 % 256 == 0: d2 in {256, 512, 1024}; otherwise the mixed arm runs the fp32 BN2 strip, row_normalize_* and
cdk_sumsq_kernel.

  case                                         arm                                      reaches
  fp32 B 384 [128, 256, 128] l2_sphere seq     fp32 stages, S = 8                       row_normalize sphere; seq masks
  fp32 B 640 [256, 512, 256] step 2, no const  fp32 stages, S = 16, <8, 256> 5 rows     joint masks step 2; L = d2 loss
  bf16 B 768 [128, 512, 768]                   mixed, NOT narrow (d2 = 768), S16 = 8    tower_col <6,3,2> nt = 2; BN2
                                                                                        <4, 256>; cdk_sumsq_kernel
  bf16 B 768 [128, 256, 1024] l2_sphere        mixed narrow, N = 1024 (NTH / (N/4) = 1) narrow sphere branch; S16 = 4
  f16 + GradScaler B 512 [128, 256, 256] sph.  mixed narrow, scaled                     tower_col <4,4,2> f16; sphere

Bounds are those of the existing tests of the same paths (test_tower_gpu.py, test_cdk_step_gpu.py)."""
import pytest
import torch
import torch.nn as nn

from oracle import nsvd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = {"W1": "0.weight", "b1": "0.bias", "g1": "1.weight", "be1": "1.bias", "W2": "3.weight", "b2": "3.bias",
        "g2": "4.weight", "be2": "4.bias"}
GRAD_KEYS = ("W1", "g1", "be1", "W2", "g2", "be2")  # (b1, b2: in front of a BatchNorm, zero in exact arithmetic)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _tower_params(B, d0, d1, d2, seed):
    g = torch.Generator().manual_seed(seed)
    P = dict(W1=torch.randn(d1, d0, generator=g) / d0 ** 0.5, b1=0.1 * torch.randn(d1, generator=g),
             g1=1.0 + 0.3 * torch.randn(d1, generator=g), be1=0.2 * torch.randn(d1, generator=g),
             W2=torch.randn(d2, d1, generator=g) / d1 ** 0.5, b2=0.1 * torch.randn(d2, generator=g),
             g2=1.0 + 0.3 * torch.randn(d2, generator=g), be2=0.2 * torch.randn(d2, generator=g))
    run = dict(rm1=0.1 * torch.randn(d1, generator=g), rv1=1.0 + 0.5 * torch.rand(d1, generator=g),
               rm2=0.1 * torch.randn(d2, generator=g), rv2=1.0 + 0.5 * torch.rand(d2, generator=g))
    x = torch.randn(B, d0, generator=g)
    dz = torch.randn(B, d2, generator=g)
    return P, run, x, dz


def _canary_workspace(B, d0, d1, d2):
    """the tower workspace followed by 4 KiB of 0xA5: nothing may be written past nsvd_tower_workspace_bytes"""
    from neural_svd_amd import hip_ops as H
    nws = H.tower_workspace(B, d0, d1, d2, DEV).numel()
    buf = torch.full((nws + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[:nws]


def _torch_f32_grads(x, P, dz, slope):
    """the yardstick: torch's own float32 modules (library GEMMs, its BatchNorm) on the same weights"""
    d1, d0 = P["W1"].shape
    d2 = P["W2"].shape[0]
    m = nn.Sequential(nn.Linear(d0, d1), nn.BatchNorm1d(d1), nn.LeakyReLU(slope), nn.Linear(d1, d2),
                      nn.BatchNorm1d(d2)).to(DEV).train()
    with torch.no_grad():
        for k, n in KEYS.items():
            dict(m.named_parameters())[n].copy_(P[k])
    (m(x) * dz).sum().backward()
    return {k: dict(m.named_parameters())[n].grad.detach().clone() for k, n in KEYS.items()}


# ---------------------------------------------------------------------------------------------------- 1. fp32 tower
@pytest.mark.parametrize("B,d0,d1,d2", [(384, 128, 256, 128), (640, 256, 4096, 128), (896, 128, 1024, 256),
                                        (1024, 128, 256, 4096), (1024, 128, 128, 2048), (256, 1024, 128, 256)])
def test_fp32_tower_instances_against_the_oracle(B, d0, d1, d2):
    """forward, backward and running statistics of the fp32 tower at every strip instance and slice count (table in
    the module docstring): output to 5e-6 of float64, each gradient within twice torch's own float32 error (at least
    2e-5), the biases in front of a BatchNorm absolute on the W1 gradient's scale, running statistics to 1e-5; the
    workspace canary untouched, a second call bit-identical."""
    from neural_svd_amd import hip_ops as H
    slope = 0.2
    P, run, x, dz = _tower_params(B, d0, d1, d2, 1000 + B + d1 + d2)
    zo, go, (st1, st2) = O.tower_forward_backward(x.double(), {k: v.double() for k, v in P.items()}, dz.double(), slope)
    Pd = {k: v.to(DEV).contiguous() for k, v in {**P, **run}.items()}
    xd, dzd = x.to(DEV), dz.to(DEV)
    buf, ws = _canary_workspace(B, d0, d1, d2)
    z = H.tower_forward(xd, Pd, slope, 1e-5, 0.1, True, ws)
    grads = H.tower_backward(xd, Pd, dzd, slope, ws)
    torch.cuda.synchronize()
    assert bool((buf[ws.numel():] == 0xA5).all()), "a tower kernel wrote past its workspace"
    assert rel(z, zo) < 5e-6, rel(z, zo)
    P_dev = {k: v.to(DEV).contiguous() for k, v in P.items()}
    lib = _torch_f32_grads(xd, P_dev, dzd, slope)
    for k in GRAD_KEYS:
        mine, theirs = rel(grads[k], go[k]), rel(lib[k], go[k])
        assert mine < max(2.0 * theirs, 2e-5), (k, mine, theirs)
    gW1 = float(go["W1"].norm())
    for k in ("b1", "b2"):
        assert float(grads[k].double().abs().max()) < 1e-5 * gW1, (k, float(grads[k].abs().max()), gW1)
    for (rm, rv), (mean, _, unb) in ((("rm1", "rv1"), st1), (("rm2", "rv2"), st2)):
        assert rel(Pd[rm], 0.9 * run[rm].double() + 0.1 * mean) < 1e-5, rm
        assert rel(Pd[rv], 0.9 * run[rv].double() + 0.1 * unb) < 1e-5, rv
    # bit reproducibility (running statistics left alone this time)
    z2 = H.tower_forward(xd, P_dev, slope, 1e-5, 0.1, False, ws)
    g2 = H.tower_backward(xd, P_dev, dzd, slope, ws)
    assert torch.equal(z, z2)
    for k in KEYS:
        assert torch.equal(grads[k], g2[k]), k


# ---------------------------------------------------------------------------------------- 2. mixed-precision tower
@pytest.mark.parametrize("B,d0,d1,d2", [(768, 128, 256, 256), (768, 384, 1024, 768), (256, 128, 2048, 256),
                                        (1024, 128, 256, 8192)])
@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("form", ["fused", "strips"])
def test_mixed_tower_instances_against_the_oracle_with_the_same_rounding(B, d0, d1, d2, half, form, monkeypatch):
    """the mixed-precision tower at B = 768 (tower_col <6, 3, 2>), S16 = 16 and S16 = 1, both forms and both half types,
    against the float64 oracle that restates its roundings, at test_tower_gpu's bounds; the float32 mode beside it
    (different by the operand rounding, and only by that); the canary; a bit-identical second call."""
    from neural_svd_amd import hip_ops as H
    slope = 0.2
    if form == "strips":
        monkeypatch.setenv("NSVD_TOWER16_FUSED", "0")
    assert H.tower_mixed_supported(B, d0, d1, d2)
    fused = H.tower_mixed_fused(B, d0, d1, d2, slope)
    assert fused == (form == "fused")
    P, _, x, dz = _tower_params(B, d0, d1, d2, 2000 + B + d1 + d2)
    zo, go, _ = O.tower_forward_backward(x.double(), {k: v.double() for k, v in P.items()}, dz.double(), slope,
                                         gemm_bf16="fused" if fused else True, half=half)
    flag = 1 | (H.TOWER16_F16 if half == "f16" else 0)
    Pd = {k: v.to(DEV).contiguous() for k, v in P.items()}
    buf, ws = _canary_workspace(B, d0, d1, d2)
    xd, dzd = x.to(DEV), dz.to(DEV)
    res = {}
    for mixed in (True, False):
        z = H.tower_forward(xd, Pd, slope, 1e-5, 0.1, False, ws, gemm_bf16=flag if mixed else 0)
        res[mixed] = (z.clone(), H.tower_backward(xd, Pd, dzd, slope, ws, gemm_bf16=flag if mixed else 0))
    torch.cuda.synchronize()
    assert bool((buf[ws.numel():] == 0xA5).all()), "a tower kernel wrote past its workspace"
    z, grads = res[True]
    assert rel(z, zo) < 2e-4, rel(z, zo)
    for k in GRAD_KEYS:
        assert rel(grads[k], go[k]) < 2e-3, (k, rel(grads[k], go[k]))
    z32, g32 = res[False]
    lo = 1e-4 if half == "bf16" else 1e-5
    assert lo < rel(z, z32) < 2e-2, rel(z, z32)
    assert lo < rel(grads["W2"], g32["W2"]) < 5e-2
    z2 = H.tower_forward(xd, Pd, slope, 1e-5, 0.1, False, ws, gemm_bf16=flag)
    g2 = H.tower_backward(xd, Pd, dzd, slope, ws, gemm_bf16=flag)
    assert torch.equal(z, z2)
    for k in KEYS:
        assert torch.equal(grads[k], g2[k]), k


# ------------------------------------------------------------------------------------------------- 3. fused step
def _build(sizes, mu, seed, mode="l2_ball", sequential=False, step=1, first=True, affine2=False):
    """affine2: the second BatchNorm's weight / bias at 1 + 0.3 randn / 0.2 randn instead of 1 / 0 (with beta2 = 0, an
    identity normalisation and no constant mode, the loss gradient's column sums - beta2's gradient - vanish exactly)"""
    from neural_svd_amd.cdk import HeteroNetwork, NestedLoRAForCDK, get_mlp
    torch.manual_seed(seed)
    model = HeteroNetwork([get_mlp(sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True),
                           get_mlp(sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True)],
                          [nn.Identity(), nn.Identity()], mu=mu, regularize_mode=mode).to(DEV).train()
    if affine2:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for side in "xy":
                bn = model.backbones[side][4]
                bn.weight.copy_(1.0 + 0.3 * torch.randn(bn.weight.shape, generator=g))
                bn.bias.copy_(0.2 * torch.randn(bn.bias.shape, generator=g))
    method = NestedLoRAForCDK(model, neigs=sizes[-1], step=step, sequential=sequential,
                              set_first_mode_const=first).to(DEV)
    return model, method


# mu sets the radius sqrt(mu) against the rows of Z = BN2(..) (row norms about sqrt(d2 (1.13 + 0.3 |z|))). At
# mu = d2 about half the rows lie inside the radius: l2_sphere scales them UP, where l2_ball would leave them - the two
# modes differ. mu = 16: every row outside (l2_ball projects all); mu = 4 d2: every row inside (l2_ball passes all).
# Never a row near the l2_ball radius, where float32 and float64 could take different branches.
STEP_CASES = {
    "fp32-sphere-seq": dict(sizes=[128, 256, 128], B=384, amp=False, mode="l2_sphere", sequential=True, mu=128.0),
    "fp32-step2-noconst": dict(sizes=[256, 512, 256], B=640, amp=False, step=2, first=False, mu=1024.0),
    "bf16-wide-d2": dict(sizes=[128, 512, 768], B=768, amp=True, mu=16.0),
    "bf16-narrow1024-sphere": dict(sizes=[128, 256, 1024], B=768, amp=True, mode="l2_sphere", mu=1024.0),
    "f16-scaler-sphere": dict(sizes=[128, 256, 256], B=512, amp=True, amp_dtype="float16", mode="l2_sphere",
                              mu=256.0),
}


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_fused_step_options_against_the_oracle(name):
    """three FusedCdkStep steps (steps 2 and 3 on the weights - and in mixed precision the 16-bit weight copies - the
    optimiser kernel wrote) against oracle.cdk_train_step with the same options, from the same weights and batches:
    each step's loss terms and total gradient norm (GradScaler: its trajectory too), then every parameter, momentum
    buffer and running statistic. Bounds: fp32 those of test_cdk_step_at_headline_size_against_the_oracle, mixed those
    of the mixed-precision / float16 step tests."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.cdk import FusedCdkStep
    c = dict(mode="l2_ball", sequential=False, step=1, first=True, amp_dtype="bfloat16")
    c.update(STEP_CASES[name])
    sizes, B, amp, half = c["sizes"], c["B"], c["amp"], "f16" if c["amp_dtype"] == "float16" else "bf16"
    mu, lr, mom, max_norm, slope, T, nstep = c["mu"], 5e-3, 0.9, 1.0, 0.2, 10, 3
    model, method = _build(sizes, mu, 11, c["mode"], c["sequential"], c["step"], c["first"], affine2=True)
    ok, why = FusedCdkStep.supported(method, B, amp, c["amp_dtype"])
    assert ok, why
    sd0 = {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(77)
    xs, ys = torch.randn(nstep, B, sizes[0], generator=g), torch.randn(nstep, B, sizes[0], generator=g)
    scaled = amp and half == "f16"
    fs = FusedCdkStep(method, lr=lr, momentum=mom, max_grad_norm=max_norm, t_max=T, batch_size=B, use_amp=amp,
                      amp_dtype=c["amp_dtype"], init_scale=2.0 ** 12, growth_interval=2)
    assert (fs.scaler is not None) == scaled
    omode = ("fused" if H.tower_mixed_fused(B, *sizes, slope) else True) if amp else False
    towers = [{k: sd0[f"backbones.{s}.{n}"].clone() for k, n in KEYS.items()} for s in "xy"]
    bufs = [{k: torch.zeros_like(v) for k, v in t.items()} for t in towers]
    running = [dict(rm1=sd0[f"backbones.{s}.1.running_mean"].clone(), rv1=sd0[f"backbones.{s}.1.running_var"].clone(),
                    rm2=sd0[f"backbones.{s}.4.running_mean"].clone(), rv2=sd0[f"backbones.{s}.4.running_var"].clone())
               for s in "xy"]
    v, M = method.vector_mask.double().cpu(), method.matrix_mask.double().cpu()
    assert torch.equal(v.float(), O.cdk_masks(sizes[-1], c["sequential"], c["step"], c["first"])[0])
    sc = dict(scale=2.0 ** 12, growth_factor=2.0, backoff_factor=0.5, growth_interval=2, growth_tracker=0, steps_ok=0,
              steps_skipped=0) if scaled else None
    tl, tn = (2e-4, 2e-3) if amp else (2e-5, 1e-4)
    for t in range(nstep):
        got = fs.step(xs[t].to(DEV), ys[t].to(DEV)).cpu().double().clone()
        (loss, lop, lmet), total = O.cdk_train_step(xs[t].double(), ys[t].double(), towers, bufs, running, v, M, mu,
                                                    O.cosine_lr(lr, t, T), mom, max_norm, slope, t == 0,
                                                    gemm_bf16=omode, half=half, scaler=sc, mode=c["mode"],
                                                    set_first_mode_const=c["first"])
        for i, want in enumerate((loss, lop, lmet)):
            assert abs(float(got[i]) - float(want)) < tl * max(1.0, abs(float(want))), (t, i, float(got[i]), float(want))
        if scaled:
            st = fs.scaler_state()
            assert (st["scale"], st["growth_tracker"], st["steps_ok"], st["steps_skipped"]) == \
                (sc["scale"], sc["growth_tracker"], sc["steps_ok"], sc["steps_skipped"]), (t, st, sc)
        assert bool(torch.isfinite(total)), "the case is meant to take every step"
        assert abs(float(got[3]) - float(total)) < tn * float(total), (t, float(got[3]), float(total))
    fs.flush_counters()
    torch.cuda.synchronize()
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    for si, s in enumerate("xy"):
        for k, n in KEYS.items():
            got, want, start = sd[f"backbones.{s}.{n}"], towers[si][k], sd0[f"backbones.{s}.{n}"]
            move, d = float((want - start).norm()), float((got - want).norm())
            if amp:
                assert d < 5e-3 * move + 1e-6 * float(want.norm()), (s, k, d, move)
            else:
                assert d < 2e-4 * move + 2e-7 * float(want.norm()), (s, k, d, move)
            bgot, bwant = fs.bufs[si][k].double().cpu(), bufs[si][k]
            if k in ("b1", "b2"):  # zero gradients by construction: rounding noise on both sides
                assert float(bgot.abs().max()) < 1e-5 and float(bwant.abs().max()) < 1e-5, (s, k)
                continue
            assert rel(bgot, bwant) < (5e-3 if amp else 2e-4), (s, k, rel(bgot, bwant))
        for tag, rk in (("1", "1"), ("4", "2")):
            for stat, pre in (("running_mean", "rm"), ("running_var", "rv")):
                got, want = sd[f"backbones.{s}.{tag}.{stat}"], running[si][pre + rk]
                assert rel(got, want) < (2e-3 if amp else 1e-5), (s, tag, stat, rel(got, want))
        assert int(sd[f"backbones.{s}.1.num_batches_tracked"]) == nstep


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_float16_grad_scaler_states_its_width_rule():
    """The GradScaler needs the fused narrow end (d2 in FusedCdkStep.SCALER_WIDTHS). float16 at d2 = 768 with the
    default scaler is refused up front, naming that rule (not a workspace error about multiples of 128); with
    grad_scaler=False it runs - the mixed arm without the narrow end, in float16 - and matches the oracle."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.cdk import FusedCdkStep
    sizes, B, mu, slope = [128, 256, 768], 256, 16.0, 0.2
    assert sizes[-1] not in FusedCdkStep.SCALER_WIDTHS and H.tower_mixed_supported(B, *sizes)
    model, method = _build(sizes, mu, 3)
    ok, why = FusedCdkStep.supported(method, B, True, "float16")
    assert not ok and "GradScaler" in why and "768" in why, why
    assert FusedCdkStep.supported(method, B, True, "float16", grad_scaler=False)[0]
    assert FusedCdkStep.supported(method, B, True, "bfloat16")[0]
    for kw in ({}, dict(grad_scaler=True)):
        with pytest.raises(H.NsvdError, match="GradScaler needs the towers' output width"):
            FusedCdkStep(method, lr=1e-3, batch_size=B, use_amp=True, amp_dtype="float16", **kw)
    sd0 = {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}
    fs = FusedCdkStep(method, lr=5e-3, momentum=0.9, max_grad_norm=1.0, batch_size=B, use_amp=True,
                      amp_dtype="float16", grad_scaler=False)
    assert fs.scaler is None
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(B, sizes[0], generator=g), torch.randn(B, sizes[0], generator=g)
    got = fs.step(x.to(DEV), y.to(DEV)).cpu().double()
    towers = [{k: sd0[f"backbones.{s}.{n}"].clone() for k, n in KEYS.items()} for s in "xy"]
    bufs = [{k: torch.zeros_like(v) for k, v in t.items()} for t in towers]
    running = [dict(rm1=sd0[f"backbones.{s}.1.running_mean"].clone(), rv1=sd0[f"backbones.{s}.1.running_var"].clone(),
                    rm2=sd0[f"backbones.{s}.4.running_mean"].clone(), rv2=sd0[f"backbones.{s}.4.running_var"].clone())
               for s in "xy"]
    v, M = method.vector_mask.double().cpu(), method.matrix_mask.double().cpu()
    omode = "fused" if H.tower_mixed_fused(B, *sizes, slope) else True
    (loss, _, _), total = O.cdk_train_step(x.double(), y.double(), towers, bufs, running, v, M, mu, 5e-3, 0.9, 1.0,
                                           slope, True, gemm_bf16=omode, half="f16")
    assert abs(float(got[0]) - float(loss)) < 2e-4 * max(1.0, abs(float(loss))), (float(got[0]), float(loss))
    assert abs(float(got[3]) - float(total)) < 2e-3 * float(total), (float(got[3]), float(total))
