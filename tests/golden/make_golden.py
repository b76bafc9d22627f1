#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by IMPORTING the reference.

Runs only in the build container (needs /root/reference); the GPU box and the
test-suite never run it, they only read the committed ``*.npz`` files.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

What it does: pre-seeds ``sys.modules`` with empty stand-ins for the optional
third-party modules the reference imports at module scope but never uses on the
NestedLoRA/PDE hot path (torch_ema, uncertainties, toml, configargparse,
termplotlib, tensorboardX, classy_vision), imports the reference's own
``get_problem`` / ``get_wavefunctions`` / ``get_dataloader`` / ``get_evd_method``
/ ``get_optimizer`` / ``compute_spectrum_evd`` and records inputs + outputs.
No reference source text is stored: fixtures are arrays only.

Every case is produced twice: float64 (truth) and float32 (reference behaviour).
"""
import os
import sys
import types
import argparse

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Dummy:
        def __init__(self, *a, **k):
            pass

    mod("torch_ema", ExponentialMovingAverage=_Dummy)
    mod("uncertainties", ufloat=lambda *a, **k: None, unumpy=types.ModuleType("unumpy"))
    sys.modules["uncertainties.unumpy"] = sys.modules["uncertainties"].unumpy
    mod("toml", loads=lambda s: {}, load=lambda f: {})
    mod("configargparse", ArgumentParser=argparse.ArgumentParser)
    mod("termplotlib", figure=_Dummy)
    mod("tensorboardX", SummaryWriter=_Dummy)
    cv = mod("classy_vision")
    cvg = mod("classy_vision.generic")
    cvd = mod("classy_vision.generic.distributed_util", is_distributed_training_run=lambda: False,
              convert_to_distributed_tensor=lambda t: (t, None), convert_to_normal_tensor=lambda t, d: t)
    cv.generic = cvg
    cvg.distributed_util = cvd


_install_stubs()
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from methods.nestedlora import (  # noqa: E402
    NestedLoRALossFunctionEVD,
    get_joint_nesting_masks,
    get_sequential_nesting_masks,
    NestedLoRA,
)
from methods.general import get_evd_method  # noqa: E402
from methods.spectrum import compute_spectrum_evd  # noqa: E402
from examples.operator.pde.problems import get_problem  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402
from examples.operator.pde.main_pde import get_dataloader  # noqa: E402
from examples.utils import get_optimizer  # noqa: E402
from examples.operator.pde.schrodinger.ground_truths import Hydrogen2D, HarmonicOscillator  # noqa: E402
from tools.generic import Namespace  # noqa: E402


def np64(t):
    return t.detach().cpu().double().numpy().copy()


def make_args(**over):
    a = argparse.Namespace(
        seed=0,
        # model
        ndim=2, n_particles=1, neigs=4, mlp_hidden_dims="32,32", nonlinearity="softplus",
        parallel=1, weight_normalization=0,
        use_fourier_feature=True, fourier_mapping_size=16, fourier_scale=0.1,
        fourier_deterministic=False, fourier_append_raw=False,
        apply_boundary=0, boundary_mode="dir_box_sqrt", lim=5.0,
        apply_exp_mask=0, exp_mask_init_scale=10.0, hard_mul_const=1.0,
        # problem
        problem="sch", potential_type="hydrogen", charge=1.0, laplacian_eps=0.01,
        operator_scale=100.0, operator_shift=0.0,
        # sampler
        sampling_mode="gaussian", sampling_scale=16.0, batch_size=24, val_eps=0.5,
        # optimiser
        optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0, num_iters=100,
        sort=0,
    )
    seq = over.pop("sequential", 1)
    step = over.pop("step", 1)
    for k, v in over.items():
        setattr(a, k, v)
    a.loss = Namespace(dict(name="neuralsvd", neuralsvd=dict(step=step, sequential=seq)))
    return a


# --------------------------------------------------------------------------- masks
def golden_masks(out):
    for L in (1, 4, 16, 33):
        v, M = get_sequential_nesting_masks(L)
        out[f"seq_L{L}_v"] = v.numpy()
        out[f"seq_L{L}_M"] = M.numpy()
    for (L, step) in ((4, 1), (16, 1), (10, 4), (16, 4), (7, 3), (5, 7)):
        m = NestedLoRA(model=None, neigs=L, step=step, sequential=False)
        out[f"joint_L{L}_s{step}_v"] = m.vector_mask.numpy()
        out[f"joint_L{L}_s{step}_M"] = m.matrix_mask.numpy()


# --------------------------------------------------------------------------- loss only
def golden_loss(out):
    g = torch.Generator().manual_seed(1234)
    cases = dict(
        a=dict(B=12, L=5, seq=True, step=1),
        b=dict(B=13, L=5, seq=False, step=1),   # odd B: torch.chunk gives 7 + 6
        c=dict(B=64, L=16, seq=False, step=1),
        d=dict(B=10, L=7, seq=False, step=3),
        e=dict(B=2, L=1, seq=True, step=1),
        f=dict(B=256, L=64, seq=True, step=1),
    )
    for name, c in cases.items():
        B, L = c["B"], c["L"]
        f64 = torch.randn(B, L, generator=g, dtype=torch.float64)
        Tf64 = torch.randn(B, L, generator=g, dtype=torch.float64) * 3.0
        m = NestedLoRA(model=None, neigs=L, step=c["step"], sequential=c["seq"])
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            f = f64.to(dt).clone().requires_grad_(True)
            Tf = Tf64.to(dt).clone().requires_grad_(True)
            f1, f2 = torch.chunk(f, 2)
            loss = NestedLoRALossFunctionEVD.apply(f, Tf, f1, f2, m.vector_mask.to(dt), m.matrix_mask.to(dt))
            (loss * 1.0).backward()
            p = f"loss_{name}_{tag}_"
            out[p + "loss"] = np64(loss)
            out[p + "grad_f"] = np64(f.grad)
            assert Tf.grad is None
            f1d, f2d = torch.chunk(f.detach(), 2)
            out[p + "lam1"] = np64(f1d.T @ f1d / f1d.shape[0])
            out[p + "lam2"] = np64(f2d.T @ f2d / f2d.shape[0])
        p = f"loss_{name}_"
        out[p + "f"] = f64.numpy()
        out[p + "Tf"] = Tf64.numpy()
        out[p + "v"] = m.vector_mask.numpy()
        out[p + "M"] = m.matrix_mask.numpy()
        out[p + "cfg"] = np.array([B, L, int(c["seq"]), c["step"]])


def golden_loss_indep(out):
    """NestedLoRALossFunctionEVD.apply with f1, f2 that are NOT chunks of f (the lower seam of
    methods/nestedlora.py:70-111; what compute_loss_kernel(split_batch=True) passes, :239-244): gradients to f, f1
    and f2 separately"""
    g = torch.Generator().manual_seed(4321)
    cases = dict(
        a=dict(B=12, B1=12, B2=12, L=5, seq=True, step=1, f1_is_f=True),    # split_batch: f1 IS f, f2 another batch
        b=dict(B=16, B1=8, B2=8, L=6, seq=False, step=1, f1_is_f=False),    # three independent tensors
        c=dict(B=9, B1=7, B2=4, L=5, seq=False, step=2, f1_is_f=False),     # unequal halves, B1 > B2
        d=dict(B=20, B1=6, B2=11, L=7, seq=True, step=1, f1_is_f=False),    # B1 < B2
        e=dict(B=64, B1=64, B2=64, L=16, seq=False, step=1, f1_is_f=True),
        f=dict(B=3, B1=1, B2=2, L=1, seq=True, step=1, f1_is_f=False),
    )
    for name, c in cases.items():
        B, B1, B2, L = c["B"], c["B1"], c["B2"], c["L"]
        f64 = torch.randn(B, L, generator=g, dtype=torch.float64)
        Tf64 = torch.randn(B, L, generator=g, dtype=torch.float64) * 3.0
        f1_64 = f64 if c["f1_is_f"] else torch.randn(B1, L, generator=g, dtype=torch.float64)
        f2_64 = torch.randn(B2, L, generator=g, dtype=torch.float64)
        m = NestedLoRA(model=None, neigs=L, step=c["step"], sequential=c["seq"])
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            f = f64.to(dt).clone().requires_grad_(True)
            Tf = Tf64.to(dt).clone().requires_grad_(True)
            f1 = f if c["f1_is_f"] else f1_64.to(dt).clone().requires_grad_(True)
            f2 = f2_64.to(dt).clone().requires_grad_(True)
            loss = NestedLoRALossFunctionEVD.apply(f, Tf, f1, f2, m.vector_mask.to(dt), m.matrix_mask.to(dt))
            (loss * 1.5).backward()  # (a grad_output that is not 1)
            p = f"indep_{name}_{tag}_"
            out[p + "loss"] = np64(loss)
            out[p + "grad_f"] = np64(f.grad)  # f1 is f: the operator and the metric gradients summed by autograd
            if not c["f1_is_f"]:
                out[p + "grad_f1"] = np64(f1.grad)
            out[p + "grad_f2"] = np64(f2.grad)
            assert Tf.grad is None
        p = f"indep_{name}_"
        out[p + "f"] = f64.numpy()
        out[p + "Tf"] = Tf64.numpy()
        if not c["f1_is_f"]:
            out[p + "f1"] = f1_64.numpy()
        out[p + "f2"] = f2_64.numpy()
        out[p + "v"] = m.vector_mask.numpy()
        out[p + "M"] = m.matrix_mask.numpy()
        out[p + "cfg"] = np.array([B, B1, B2, L, int(c["seq"]), c["step"], int(c["f1_is_f"])])


# --------------------------------------------------------------------------- full model
def build(args, dtype):
    torch.manual_seed(args.seed)
    operator, gt = get_problem(args, torch.device("cpu"))
    model = get_wavefunctions(args)
    make_batch, val_data, batch_ftn_val, imp_train, imp_val = get_dataloader(args, torch.device("cpu"))
    method = get_evd_method(args, "neuralsvd", model)
    method = method.to(dtype)
    return operator, gt, method, make_batch, val_data, batch_ftn_val, imp_train, imp_val


def importance_for(args, dtype):
    # the reference builds its MultivariateNormal in float32; for the float64 truth
    # we rebuild the same density in float64
    from torch.distributions import MultivariateNormal
    d = args.n_particles * args.ndim
    mvn = MultivariateNormal(loc=torch.zeros(d, dtype=dtype),
                             covariance_matrix=args.sampling_scale ** 2 * torch.eye(d, dtype=dtype))
    return lambda x: mvn.log_prob(x.view(x.shape[0], -1)).exp().view(-1, 1)


def golden_model(out, name, nsteps=2, grid=True, store_params=True, sample_stride=None, **over):
    args64 = make_args(**over)
    # draw x once (float32, like the reference's sampler), reuse for both dtypes
    torch.manual_seed(args64.seed + 1000)
    xs = [args64.sampling_scale * torch.randn((args64.batch_size, 1, args64.ndim)) for _ in range(nsteps)]
    out[f"{name}_x"] = np.stack([x.reshape(x.shape[0], -1).numpy() for x in xs])
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        args = make_args(**over)
        operator, gt, method, _, val_data, batch_ftn_val, _, imp_val = build(args, dtype)
        imp_train = importance_for(args, dtype)
        p = f"{name}_{tag}_"
        names = [n for n, _ in method.named_parameters()]
        if tag == "f64":
            out[f"{name}_param_names"] = np.array(names)
            out[f"{name}_gt"] = np.asarray(gt, dtype=np.float64)
            out[f"{name}_v"] = method.vector_mask.numpy()
            out[f"{name}_M"] = method.matrix_mask.numpy()
            if store_params:
                # parameters are created in float32 by the reference; both dtypes start from the same values
                for n, t in method.named_parameters():
                    out[f"{name}_param0_{n}"] = t.detach().float().numpy()
        optimizer = get_optimizer(args, method)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, args.num_iters)
        for it in range(nsteps):
            method.train()
            optimizer.zero_grad()
            x = xs[it].to(dtype)
            x = x.reshape(x.shape[0], -1)
            loss, aux = method.compute_loss_operator(operator, x, importance=imp_train)
            loss.backward()
            out[p + f"step{it}_loss"] = np64(loss)
            out[p + f"step{it}_f"] = np64(aux["f"])
            out[p + f"step{it}_Tf"] = np64(aux["Tf"])
            for n, t in method.named_parameters():
                if t.grad is None:
                    continue
                g = np64(t.grad)
                if sample_stride is None:
                    out[p + f"step{it}_grad_{n}"] = g
                else:
                    out[p + f"step{it}_gradnorm_{n}"] = np.array(np.linalg.norm(g))
                    out[p + f"step{it}_gradsample_{n}"] = g.reshape(-1)[::sample_stride]
            optimizer.step()
            scheduler.step()
            if sample_stride is None:
                for n, t in method.named_parameters():
                    out[p + f"step{it}_param_{n}"] = np64(t)
        if grid and batch_ftn_val is not None:
            method.eval()
            with torch.no_grad():
                vd = val_data.to(dtype)
                bs = args.batch_size

                def loader():
                    for i in range(int(np.ceil(len(vd) / float(bs)))):
                        yield vd[i * bs:min((i + 1) * bs, len(vd))], 0.

                imp_val_d = lambda x: imp_val(x).to(dtype)  # noqa: E731
                res = compute_spectrum_evd(method, dataloader=loader(), operator=operator,
                                           importance_train=imp_train, importance_val=imp_val_d,
                                           normalize=True, set_first_mode_const=False, device=torch.device("cpu"))
            out[p + "spec_eigvals"] = np.asarray(res["eigvals"], dtype=np.float64)
            out[p + "spec_norms"] = np.asarray(res["norms"], dtype=np.float64)
            out[p + "spec_quad"] = np.asarray(res["quad"], dtype=np.float64)
            out[p + "spec_cov_normalized"] = np.asarray(res["cov"], dtype=np.float64)
            if tag == "f64":
                out[f"{name}_val_data"] = val_data.numpy()
    cfg = {k: v for k, v in vars(make_args(**over)).items() if k != "loss"}
    cfg["sequential"] = int(over.get("sequential", 1))
    cfg["step"] = int(over.get("step", 1))
    out[f"{name}_cfg"] = np.array(repr(cfg))


def golden_debug_model(out):
    """RNG-free model: ParallelMLP(debug=True) + deterministic Fourier map (reference
    examples/models/mlp.py:190-193, examples/utils.py:106-113)."""
    from examples.models.mlp import ParallelMLP
    from examples.utils import GaussianFourierFeatureTransform
    fm = GaussianFourierFeatureTransform(input_dim=2, mapping_size=3, scale=0.25, deterministic=True)
    mlp = ParallelMLP(input_dim=2, mlp_hidden_dims=[8, 8], output_dim=1, num_copies=3, nonlinearity="softplus",
                      bias=True, feature_map=fm, debug=True)
    x = torch.tensor([[0.1, -0.2], [1.5, 0.3], [-0.7, 0.9], [2.0, -1.0], [0.0, 0.0]])
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        y = mlp.to(dtype)(x.to(dtype))
        out[f"debug_{tag}_y"] = np64(y)
    out["debug_x"] = x.numpy()
    out["debug_B"] = fm._B.detach().float().numpy()


def golden_cdk(out):
    """NestedLoRALossFunctionForCDK (methods/nestedlora.py:270-332) + NestedLoRAForCDK masks (:335-378)."""
    from methods.nestedlora import NestedLoRALossFunctionForCDK, NestedLoRAForCDK
    g = torch.Generator().manual_seed(4321)
    cases = dict(
        a=dict(B=9, L=5, seq=False, step=1, first=True, bw=False),
        b=dict(B=16, L=8, seq=True, step=1, first=True, bw=True),
        c=dict(B=12, L=6, seq=False, step=4, first=False, bw=False),
        d=dict(B=70, L=33, seq=False, step=1, first=True, bw=False),
        e=dict(B=64, L=512, seq=False, step=1, first=True, bw=False),
    )
    for name, c in cases.items():
        B, L = c["B"], c["L"]
        f64 = torch.randn(B, L, generator=g, dtype=torch.float64) * 0.5
        g64 = torch.randn(B, L, generator=g, dtype=torch.float64) * 0.5
        bw64 = (torch.rand(B, 1, generator=g, dtype=torch.float64) + 0.5) if c["bw"] else None
        m = NestedLoRAForCDK(model=None, neigs=L, step=c["step"], sequential=c["seq"], set_first_mode_const=c["first"])
        p = f"cdk_{name}_"
        out[p + "f"], out[p + "g"] = f64.numpy(), g64.numpy()
        if bw64 is not None:
            out[p + "bw"] = bw64.numpy()
        out[p + "v"], out[p + "M"] = m.vector_mask.numpy(), m.matrix_mask.numpy()
        out[p + "cfg"] = np.array([B, L, int(c["seq"]), c["step"], int(c["first"]), int(c["bw"])])
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            f = f64.to(dt).clone().requires_grad_(True)
            gg = g64.to(dt).clone().requires_grad_(True)
            bw = None if bw64 is None else bw64.to(dt)
            loss, lop, lmet, rj, ri = NestedLoRALossFunctionForCDK.apply(
                f, gg, m.vector_mask.to(dt), m.matrix_mask.to(dt), c["first"], bw)
            loss.backward()
            q = p + tag + "_"
            out[q + "loss"] = np.array([float(loss), float(lop), float(lmet)])
            out[q + "rs_joint"], out[q + "rs_indep"] = np64(rj), np64(ri)
            out[q + "grad_f"], out[q + "grad_g"] = np64(f.grad), np64(gg.grad)


def golden_svd(out):
    """NestedLoRALossFunctionSVD (methods/nestedlora.py:114-164): loss and gradients w.r.t. f and g. The reference has
    no caller for it (both compute_loss_* raise for evd=False); the Function itself is complete."""
    from methods.nestedlora import NestedLoRA, NestedLoRALossFunctionSVD
    g = torch.Generator().manual_seed(777)
    cases = dict(a=dict(B=8, L=4, seq=True, step=1), b=dict(B=12, L=6, seq=False, step=1),
                 c=dict(B=64, L=16, seq=False, step=4), d=dict(B=33, L=7, seq=True, step=1),
                 e=dict(B=256, L=64, seq=False, step=1))
    for name, c in cases.items():
        B, L = c["B"], c["L"]
        t = [torch.randn(B, L, generator=g, dtype=torch.float64) * s for s in (0.5, 2.0, 0.5, 2.0)]
        m = NestedLoRA(model=None, neigs=L, step=c["step"], sequential=c["seq"])
        p = f"svd_{name}_"
        for k, v in zip(("f", "Tg", "g", "Tadjf"), t):
            out[p + k] = v.numpy()
        out[p + "v"], out[p + "M"] = m.vector_mask.numpy(), m.matrix_mask.numpy()
        out[p + "cfg"] = np.array([B, L, int(c["seq"]), c["step"]])
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            f, Tg, gg, Ta = [x.to(dt).clone() for x in t]
            f.requires_grad_(True)
            gg.requires_grad_(True)
            loss = NestedLoRALossFunctionSVD.apply(f, Tg, gg, Ta, m.vector_mask.to(dt), m.matrix_mask.to(dt))
            loss.backward()
            q = p + tag + "_"
            out[q + "loss"] = np.array([float(loss)])
            out[q + "grad_f"], out[q + "grad_g"] = np64(f.grad), np64(gg.grad)


def golden_normalize(out):
    """normalize(z, r_up, mode) of examples/models/siam.py:170-183 ('l2_ball', 'l2_sphere') and its autograd gradient
    for a given upstream gradient; rows straddle the radius, one row is exactly zero."""
    from examples.models.siam import normalize
    g = torch.Generator().manual_seed(99)
    for name, (B, L, r) in dict(a=(7, 5, 1.5), b=(12, 512, 4.0), c=(33, 30, 0.7), d=(8, 128, 16.0)).items():
        z64 = torch.randn(B, L, generator=g, dtype=torch.float64) * (2.0 * r / np.sqrt(L)) * \
            (0.25 + 1.5 * torch.rand(B, 1, generator=g, dtype=torch.float64))
        z64[0] = 0.0
        d64 = torch.randn(B, L, generator=g, dtype=torch.float64)
        p = f"norm_{name}_"
        out[p + "z"], out[p + "dout"], out[p + "cfg"] = z64.numpy(), d64.numpy(), np.array([B, L, r])
        for mode in ("l2_ball", "l2_sphere"):
            for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                if tag == "f32" and B * L > 2000:
                    continue  # the float32 yardstick only for the small cases (fixture size)
                z = z64.to(dt).clone().requires_grad_(True)
                y = normalize(z, r, mode)
                y.backward(d64.to(dt))
                out[p + f"{mode}_{tag}_out"], out[p + f"{mode}_{tag}_dz"] = np64(y), np64(z.grad)


def gaussian_kernel_op_factory(ell):
    """A toy `get_approx_kernel_op` for NestedLoRA.compute_loss_kernel (the reference ships none): the Gaussian
    kernel k(x, y) = exp(-|x - y|^2 / (2 ell^2)) applied by Monte-Carlo quadrature on the reference batch,
    Kf(x) = (1 / B_ref) sum_j k(x, x_ref_j) f(x_ref_j), f evaluated through the method itself."""
    def get_approx_kernel_op(x_ref):
        def op(method, x, importance=None):
            f = method(x)
            with torch.no_grad():
                f_ref = method(x_ref)
                Kmat = torch.exp(-torch.cdist(x, x_ref) ** 2 / (2.0 * ell ** 2))
                Kf = Kmat @ f_ref / x_ref.shape[0]
            return Kf, f
        return op
    return get_approx_kernel_op


def golden_kernel_loss(out):
    """NestedLoRA.compute_loss_kernel (methods/nestedlora.py:230-252), both split_batch modes, on the reference's own
    WaveFunctions model (plain model evaluation: no importance, no stencil) with the toy Gaussian-kernel operator
    above: loss, f, Kf and every parameter gradient, float64 and float32."""
    ell = 1.5
    cases = dict(
        ka=dict(neigs=4, mlp_hidden_dims="32,32", fourier_mapping_size=16, fourier_scale=0.3, batch_size=24,
                sequential=1, seed=21),
        kb=dict(neigs=4, mlp_hidden_dims="128,128,128", fourier_mapping_size=64, fourier_scale=0.3, batch_size=64,
                sequential=0, step=1, apply_exp_mask=1, exp_mask_init_scale=3.0, seed=22),
        kc=dict(neigs=5, mlp_hidden_dims="12,20", fourier_mapping_size=5, fourier_scale=0.3, batch_size=33,
                sequential=0, step=2, seed=23),
    )
    for name, over in cases.items():
        args0 = make_args(**dict(over))
        torch.manual_seed(args0.seed + 500)
        x32 = 2.0 * torch.randn(args0.batch_size, args0.ndim)
        out[f"{name}_x"] = x32.numpy()
        out[f"{name}_ell"] = np.array(ell)
        big = "128" in over["mlp_hidden_dims"]
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            args = make_args(**dict(over))
            _, _, method, *_ = build(args, dtype)
            if tag == "f64":
                out[f"{name}_param_names"] = np.array([n for n, _ in method.named_parameters()])
                out[f"{name}_v"], out[f"{name}_M"] = method.vector_mask.numpy(), method.matrix_mask.numpy()
                if not big:  # the H=128 case is rebuilt from its seed (same recipe as the cfg1 fixture)
                    for n, t in method.named_parameters():
                        out[f"{name}_param0_{n}"] = t.detach().float().numpy()
            x = x32.to(dtype)
            for split in (False, True):
                method.zero_grad()
                loss, aux = method.compute_loss_kernel(gaussian_kernel_op_factory(ell), x, None, split_batch=split)
                loss.backward()
                q = f"{name}_{tag}_split{int(split)}_"
                out[q + "loss"], out[q + "f"], out[q + "Kf"] = np64(loss), np64(aux["f"]), np64(aux["Tf"])
                for n, t in method.named_parameters():
                    if t.grad is None:
                        continue
                    g = np64(t.grad)
                    if big and g.size > 4096:
                        out[q + f"gradnorm_{n}"] = np.array(np.linalg.norm(g))
                        out[q + f"gradsample_{n}"] = g.reshape(-1)[::61]
                    else:
                        out[q + f"grad_{n}"] = g
        cfg = {k: v for k, v in vars(make_args(**dict(over))).items() if k != "loss"}
        cfg["sequential"], cfg["step"] = int(over.get("sequential", 1)), int(over.get("step", 1))
        out[f"{name}_cfg"] = np.array(repr(cfg))


def golden_tower(out):
    """The CDK script's tower (main_sketchy.py:107-116): get_mlp(sizes=[d0, d1, d2], bias=True, nonlinearity='lrelu0.2',
    use_bn=True) of examples/models/mlp.py:129-164 in training mode: output, autograd gradients of sum(dz * z) and the
    BatchNorm running statistics after the step, float64 and float32. Case tb (multiples of 128: what the HIP tower
    kernels take) stores no parameters: torch.manual_seed(seed) + the same constructor calls reproduce them."""
    from examples.models.mlp import get_mlp
    for name, (sizes, B, slope, seed) in dict(ta=([8, 12, 6], 10, 0.2, 31), tb=([128, 256, 128], 128, 0.2, 32),
                                              tc=([16, 24, 8], 20, 0.0, 33)).items():
        g = torch.Generator().manual_seed(1000 + seed)
        x64 = torch.randn(B, sizes[0], generator=g, dtype=torch.float64)
        dz64 = torch.randn(B, sizes[2], generator=g, dtype=torch.float64)
        out[f"{name}_x"], out[f"{name}_dz"] = x64.numpy(), dz64.numpy()
        out[f"{name}_cfg"] = np.array([B, sizes[0], sizes[1], sizes[2], seed])
        out[f"{name}_slope"] = np.array(slope)
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            torch.manual_seed(seed)
            m = get_mlp(sizes=sizes, bias=True, nonlinearity="relu" if slope == 0.0 else f"lrelu{slope}", use_bn=True)
            with torch.no_grad():  # non-trivial BatchNorm affine parameters (the constructor's are 1 and 0)
                gg = torch.Generator().manual_seed(2000 + seed)
                for k in (1, 4):
                    m[k].weight.copy_(1.0 + 0.3 * torch.randn(m[k].weight.shape, generator=gg))
                    m[k].bias.copy_(0.2 * torch.randn(m[k].bias.shape, generator=gg))
            if tag == "f64" and name != "tb":
                for k, v in m.state_dict().items():
                    out[f"{name}_param0_{k}"] = v.detach().double().numpy()
            m = m.to(dt).train()
            z = m(x64.to(dt))
            (z * dz64.to(dt)).sum().backward()
            q = f"{name}_{tag}_"
            out[q + "z"] = np64(z)
            for k, v in m.named_parameters():
                gr = np64(v.grad)
                if name == "tb" and tag == "f32":
                    out[q + f"gradnorm_{k}"] = np.array(np.linalg.norm(gr))
                else:
                    out[q + f"grad_{k}"] = gr
            for k in (1, 4):
                out[q + f"running_mean_{k}"] = np64(m[k].running_mean)
                out[q + f"running_var_{k}"] = np64(m[k].running_var)


def golden_cdk_step(out):
    """The Sketchy training step (examples/cdk/sketchy/main_sketchy.py:180-212 as configured by scripts/exps/sketchy.sh:
    sgd momentum 0.9, --clip_grad_norm (max norm 1), --use_lr_scheduler = CosineAnnealingLR, AMP off here): HeteroNetwork
    of two get_mlp towers with Identity projectors (main_sketchy.py:107-116, models/siam.py:132-166), l2_ball
    normalisation, NestedLoRAForCDK loss, clip_grad_norm_, SGD step, scheduler step - three steps on fixed inputs, float64
    and float32. Stored: inputs, masks, per-step loss triple and total gradient norm, the parameters / momentum buffers /
    BatchNorm running statistics after the last step (case sb: every 5th element + norms; its initial weights come from
    torch.manual_seed(seed) + the same constructor calls)."""
    from examples.models.mlp import get_mlp
    from examples.models.siam import HeteroNetwork
    from methods.nestedlora import NestedLoRAForCDK
    cases = dict(sa=dict(sizes=[8, 12, 6], B=10, mu=4.0, lr=5e-2, seed=41, T=10),
                 sb=dict(sizes=[128, 256, 128], B=128, mu=16.0, lr=5e-3, seed=42, T=10))
    NSTEP = 3
    for name, c in cases.items():
        sizes, B, L = c["sizes"], c["B"], c["sizes"][-1]
        g = torch.Generator().manual_seed(3000 + c["seed"])
        xs = torch.randn(NSTEP, B, sizes[0], generator=g, dtype=torch.float64)
        ys = torch.randn(NSTEP, B, sizes[0], generator=g, dtype=torch.float64)
        if name == "sa":  # (sb: the two randn calls above on torch.Generator().manual_seed(3000 + seed) reproduce them)
            out[f"{name}_x"], out[f"{name}_y"] = xs.numpy(), ys.numpy()
        out[f"{name}_cfg"] = np.array([B, sizes[0], sizes[1], sizes[2], c["seed"], NSTEP, c["T"]])
        out[f"{name}_hyper"] = np.array([c["mu"], c["lr"], 0.9, 1.0, 0.2])  # mu, lr, momentum, max_norm, slope
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            torch.manual_seed(c["seed"])
            model = HeteroNetwork(backbones=[get_mlp(sizes=sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True),
                                             get_mlp(sizes=sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True)],
                                  projectors=[nn.Identity(), nn.Identity()], mu=c["mu"], regularize_mode="l2_ball")
            if tag == "f64" and name == "sa":
                for k, v in model.state_dict().items():
                    out[f"{name}_param0_{k}"] = v.detach().double().numpy()
            model = model.to(dt).train()
            method = NestedLoRAForCDK(model, neigs=L, step=1, sequential=False, set_first_mode_const=True)
            if tag == "f64":
                out[f"{name}_v"], out[f"{name}_M"] = method.vector_mask.numpy(), method.matrix_mask.numpy()
            method.vector_mask, method.matrix_mask = method.vector_mask.to(dt), method.matrix_mask.to(dt)
            opt = torch.optim.SGD(model.parameters(), lr=c["lr"], momentum=0.9, weight_decay=0.0)
            sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, c["T"])
            losses, norms = [], []
            for t in range(NSTEP):
                opt.zero_grad()
                _, fx, _, fy = method(xs[t].to(dt), ys[t].to(dt))
                loss, lop, lmet, rj, ri = method.compute_loss(fx, fy)
                loss.backward()
                total_norm = nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
                opt.step()
                sched.step()
                losses.append([float(loss), float(lop), float(lmet)])
                norms.append(float(total_norm))
            q = f"{name}_{tag}_"
            out[q + "loss"], out[q + "total_norm"] = np.array(losses), np.array(norms)
            sd = model.state_dict()
            for k, v in sd.items():
                if "num_batches" in k:
                    continue
                a = np64(v)
                if name == "sb":
                    out[q + f"pnorm_{k}"] = np.array(np.linalg.norm(a))
                    a = a.reshape(-1)[::5]
                    if tag == "f32":
                        continue
                out[q + f"param_{k}"] = a
            for k, prm in model.named_parameters():
                a = np64(opt.state[prm]["momentum_buffer"])
                if name == "sb":
                    out[q + f"bufnorm_{k}"] = np.array(np.linalg.norm(a))
                    continue
                out[q + f"buf_{k}"] = a


def golden_cdk_step_opts(out):
    """The Sketchy training step of golden_cdk_step with the options it leaves at their sketchy.sh values: case oa -
    regularize_mode='l2_sphere' (models/siam.py:178-180) with sequential nesting masks (methods/nestedlora.py:348-349);
    case ob - 'l2_ball' with joint masks at step = 2 and set_first_mode_const=False (:350-358, --neuralsvd.step /
    --neuralsvd.sequential). Two SGD steps each at a tiny shape, float64 only (the oracle is held to it at float64
    precision). Stored: initial parameters and running statistics, inputs, masks, per-step loss triple and total gradient
    norm, and every parameter / momentum buffer / running statistic after the last step."""
    from examples.models.mlp import get_mlp
    from examples.models.siam import HeteroNetwork
    from methods.nestedlora import NestedLoRAForCDK
    cases = dict(oa=dict(sizes=[8, 12, 6], B=10, mu=4.0, lr=5e-2, seed=43, T=10, mode="l2_sphere", seq=True, step=1,
                         first=True),
                 ob=dict(sizes=[8, 12, 6], B=10, mu=4.0, lr=5e-2, seed=44, T=10, mode="l2_ball", seq=False, step=2,
                         first=False))
    NSTEP = 2
    for name, c in cases.items():
        sizes, B, L = c["sizes"], c["B"], c["sizes"][-1]
        g = torch.Generator().manual_seed(3000 + c["seed"])
        xs = torch.randn(NSTEP, B, sizes[0], generator=g, dtype=torch.float64)
        ys = torch.randn(NSTEP, B, sizes[0], generator=g, dtype=torch.float64)
        out[f"{name}_x"], out[f"{name}_y"] = xs.numpy(), ys.numpy()
        out[f"{name}_cfg"] = np.array([B, sizes[0], sizes[1], sizes[2], c["seed"], NSTEP, c["T"]])
        out[f"{name}_hyper"] = np.array([c["mu"], c["lr"], 0.9, 1.0, 0.2])  # mu, lr, momentum, max_norm, slope
        # mode (1 = l2_sphere), sequential, step, set_first_mode_const
        out[f"{name}_opts"] = np.array([int(c["mode"] == "l2_sphere"), int(c["seq"]), c["step"], int(c["first"])])
        torch.manual_seed(c["seed"])
        model = HeteroNetwork(backbones=[get_mlp(sizes=sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True),
                                         get_mlp(sizes=sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True)],
                              projectors=[nn.Identity(), nn.Identity()], mu=c["mu"], regularize_mode=c["mode"])
        for k, v in model.state_dict().items():
            if "num_batches" not in k:
                out[f"{name}_param0_{k}"] = v.detach().double().numpy()
        model = model.double().train()
        method = NestedLoRAForCDK(model, neigs=L, step=c["step"], sequential=c["seq"], set_first_mode_const=c["first"])
        out[f"{name}_v"], out[f"{name}_M"] = np64(method.vector_mask), np64(method.matrix_mask)
        method.vector_mask, method.matrix_mask = method.vector_mask.double(), method.matrix_mask.double()
        opt = torch.optim.SGD(model.parameters(), lr=c["lr"], momentum=0.9, weight_decay=0.0)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, c["T"])
        losses, norms = [], []
        for t in range(NSTEP):
            opt.zero_grad()
            _, fx, _, fy = method(xs[t], ys[t])
            loss, lop, lmet, rj, ri = method.compute_loss(fx, fy)
            loss.backward()
            total_norm = nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
            opt.step()
            sched.step()
            losses.append([float(loss), float(lop), float(lmet)])
            norms.append(float(total_norm))
        q = f"{name}_f64_"
        out[q + "loss"], out[q + "total_norm"] = np.array(losses), np.array(norms)
        for k, v in model.state_dict().items():
            if "num_batches" not in k:
                out[q + f"param_{k}"] = np64(v)
        for k, prm in model.named_parameters():
            out[q + f"buf_{k}"] = np64(opt.state[prm]["momentum_buffer"])


def golden_amp(out):
    """The reference's AMP branch (on by default in the Sketchy script: examples/cdk/sketchy/main_sketchy.py:161,182,
    194-208) run HERE, on the CPU: torch.cuda.amp.autocast disables itself without a CUDA device, so the same modules run
    under torch.autocast("cpu", dtype=torch.float16) - Linear / BatchNorm / LeakyReLU outputs are float16 tensors, the
    masters float32, as under CUDA autocast - with torch.amp.GradScaler("cpu") in GradScaler's place. Not the CUDA kernels'
    bits (accumulation orders differ), but the reference's own code and torch's own autocast / GradScaler semantics.
      amp_tower_*: get_mlp([128, 256, 256], lrelu0.2, BatchNorm) forward + backward of sum(dz * z) on 256 rows.
      amp_step_*:  eight iterations of the loop body of main_sketchy.py:180-212 (sgd momentum 0.9, clip_grad_norm 1,
                   CosineAnnealingLR(T_max = 6) stepped EVERY iteration as the script does) from torch's default loss scale
                   of 2^16 with growth_interval = 2 (the scale doubles every second iteration up to 2^20; nothing
                   overflows - under autocast the reference's LOSS runs in float16 as well, so its overflow threshold,
                   between 2^20 and 2^21 here, is not that of a build whose loss is float32: skip patterns beyond it are
                   not comparable): per iteration the loss, the unscaled total norm, the scale after update(); the
                   parameters after the last one. Initial weights: torch.manual_seed(seed) + the constructor calls."""
    from examples.models.mlp import get_mlp
    from examples.models.siam import HeteroNetwork
    from methods.nestedlora import NestedLoRAForCDK
    sizes, B, slope = [128, 256, 256], 256, 0.2
    # ---- tower
    seed = 51
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(B, sizes[0], generator=g)
    dz = torch.randn(B, sizes[2], generator=g)
    out["amp_tower_cfg"] = np.array([B, sizes[0], sizes[1], sizes[2], seed])
    out["amp_tower_x"], out["amp_tower_dz"] = x.numpy(), dz.numpy()
    for tag in ("f16", "f64"):
        torch.manual_seed(seed)
        m = get_mlp(sizes=sizes, bias=True, nonlinearity=f"lrelu{slope}", use_bn=True)
        with torch.no_grad():
            gg = torch.Generator().manual_seed(2000 + seed)
            for k in (1, 4):
                m[k].weight.copy_(1.0 + 0.3 * torch.randn(m[k].weight.shape, generator=gg))
                m[k].bias.copy_(0.2 * torch.randn(m[k].bias.shape, generator=gg))
        if tag == "f16":
            for k, v in m.state_dict().items():
                if "num_batches" not in k:
                    out[f"amp_tower_param0_{k}"] = v.detach().numpy().copy()
            m = m.train()
            with torch.autocast("cpu", dtype=torch.float16):
                z = m(x)
            assert z.dtype == torch.float16
            (z.float() * dz).sum().backward()
        else:
            m = m.double().train()
            z = m(x.double())
            (z * dz.double()).sum().backward()
        q = f"amp_tower_{tag}_"
        out[q + "z"] = np64(z)
        for k, v in m.named_parameters():
            out[q + f"grad_{k}"] = np64(v.grad)
    # ---- training iterations with the GradScaler
    seed, mu, lr, T, nstep = 11, 16.0, 5e-3, 6, 8
    g = torch.Generator().manual_seed(77)
    xs = torch.randn(nstep, B, sizes[0], generator=g)
    ys = torch.randn(nstep, B, sizes[0], generator=g)
    out["amp_step_cfg"] = np.array([B, sizes[0], sizes[1], sizes[2], seed, nstep, T])
    out["amp_step_hyper"] = np.array([mu, lr, 0.9, 1.0, slope, 2.0 ** 16, 2.0])  # .. init scale, growth interval
    torch.manual_seed(seed)
    model = HeteroNetwork(backbones=[get_mlp(sizes=sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True),
                                     get_mlp(sizes=sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True)],
                          projectors=[nn.Identity(), nn.Identity()], mu=mu, regularize_mode="l2_ball").train()
    method = NestedLoRAForCDK(model, neigs=sizes[-1], step=1, sequential=False, set_first_mode_const=True)
    opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0 ** 16, growth_interval=2)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rows = []
    for t in range(nstep):
        opt.zero_grad()
        with torch.autocast("cpu", dtype=torch.float16):
            _, fx, _, fy = method(xs[t], ys[t])
            loss, lop, lmet, rj, ri = method.compute_loss(fx, fy)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        total_norm = nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        scaler.step(opt)
        scaler.update()
        sched.step()
        rows.append([float(loss), float(total_norm), float(scaler.get_scale())])
    out["amp_step_rows"] = np.array(rows)  # loss | unscaled total norm (inf / nan: skipped) | scale after update()
    for k, v in model.state_dict().items():
        if "num_batches" in k:
            continue
        out[f"amp_step_param_{k}"] = v.detach().numpy()[..., ::3].copy() if v.dim() == 2 else v.detach().numpy().copy()
        out[f"amp_step_move_{k}"] = np.array(float((v.detach() - sd0[k]).double().norm()))


def golden_ground_truth(out):
    out["gt_hydrogen2d_64"] = Hydrogen2D(charge=1.0).get_eigvals(64)
    out["gt_hydrogen2d_z2_9"] = Hydrogen2D(charge=2.0).get_eigvals(9)
    for n in (1, 6, 16, 32, 55):
        out[f"gt_oscillator_{n}"] = HarmonicOscillator(k=1.0, ndim=2).get_eigvals(n)


# the cases of tests/test_checkpoint_interchange.py
CHECKPOINT_CASES = [dict(neigs=4, mlp_hidden_dims="32,32", fourier_mapping_size=16),
                    dict(neigs=3, mlp_hidden_dims="128,128,128", fourier_mapping_size=64,
                         potential_type="harmonic_oscillator", apply_exp_mask=1, exp_mask_init_scale=10.0,
                         sequential=0)]


def golden_checkpoint(out):
    """what a reference checkpoint holds (examples/operator/__init__.py:139-145): per case the reference method's
    state_dict keys in order with their shapes and dtypes, the number of its trainable tensors, its optimiser's
    param_groups, and the values of one state_dict drawn under torch.manual_seed(5)"""
    import json
    for i, over in enumerate(CHECKPOINT_CASES):
        args = make_args(**dict(over))
        torch.manual_seed(5)
        ref = get_evd_method(args, "neuralsvd", get_wavefunctions(args))
        sd = ref.state_dict()
        opt = get_optimizer(args, ref)
        meta = dict(keys=list(sd.keys()), shapes=[list(t.shape) for t in sd.values()],
                    dtypes=[str(t.dtype) for t in sd.values()],
                    n_trainable=sum(1 for p in ref.parameters() if p.requires_grad),
                    optimizer=type(opt).__name__, param_groups=opt.state_dict()["param_groups"])
        out[f"case{i}_meta"] = np.array(json.dumps(meta))
        for k, t in sd.items():
            out[f"case{i}_sd.{k}"] = t.detach().numpy().copy()


def main():
    torch.set_num_threads(8)
    if len(sys.argv) > 1 and sys.argv[1] == "checkpoint":
        o = {}
        golden_checkpoint(o)
        np.savez_compressed(os.path.join(HERE, "checkpoint.npz"), **o)
        print("checkpoint", os.path.getsize(os.path.join(HERE, "checkpoint.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "normalize":
        o = {}
        golden_normalize(o)
        np.savez_compressed(os.path.join(HERE, "normalize.npz"), **o)
        print("normalize", os.path.getsize(os.path.join(HERE, "normalize.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "cdk_step":
        o = {}
        golden_cdk_step(o)
        np.savez_compressed(os.path.join(HERE, "cdk_step.npz"), **o)
        print("cdk_step", os.path.getsize(os.path.join(HERE, "cdk_step.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "cdk_step_opts":
        o = {}
        golden_cdk_step_opts(o)
        np.savez_compressed(os.path.join(HERE, "cdk_step_opts.npz"), **o)
        print("cdk_step_opts", os.path.getsize(os.path.join(HERE, "cdk_step_opts.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "tower":
        o = {}
        golden_tower(o)
        np.savez_compressed(os.path.join(HERE, "tower.npz"), **o)
        print("tower", os.path.getsize(os.path.join(HERE, "tower.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "kernel_loss":
        o = {}
        golden_kernel_loss(o)
        np.savez_compressed(os.path.join(HERE, "kernel_loss.npz"), **o)
        print("kernel_loss", os.path.getsize(os.path.join(HERE, "kernel_loss.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "amp":
        o = {}
        golden_amp(o)
        np.savez_compressed(os.path.join(HERE, "amp.npz"), **o)
        print("amp", os.path.getsize(os.path.join(HERE, "amp.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "loss_indep":
        o = {}
        golden_loss_indep(o)
        np.savez_compressed(os.path.join(HERE, "evd_loss_indep.npz"), **o)
        print("evd_loss_indep", os.path.getsize(os.path.join(HERE, "evd_loss_indep.npz")) // 1024, "KiB")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "svd":  # only the fixture added last (the others stay byte-identical)
        o = {}
        golden_svd(o)
        np.savez_compressed(os.path.join(HERE, "svd_loss.npz"), **o)
        print("svd_loss", os.path.getsize(os.path.join(HERE, "svd_loss.npz")) // 1024, "KiB")
        return
    o = {}
    golden_checkpoint(o)
    np.savez_compressed(os.path.join(HERE, "checkpoint.npz"), **o)
    o = {}
    golden_cdk_step(o)
    np.savez_compressed(os.path.join(HERE, "cdk_step.npz"), **o)
    o = {}
    golden_cdk_step_opts(o)
    np.savez_compressed(os.path.join(HERE, "cdk_step_opts.npz"), **o)
    o = {}
    golden_tower(o)
    np.savez_compressed(os.path.join(HERE, "tower.npz"), **o)
    o = {}
    golden_kernel_loss(o)
    np.savez_compressed(os.path.join(HERE, "kernel_loss.npz"), **o)
    o = {}
    golden_svd(o)
    np.savez_compressed(os.path.join(HERE, "svd_loss.npz"), **o)
    o = {}
    golden_normalize(o)
    np.savez_compressed(os.path.join(HERE, "normalize.npz"), **o)
    o = {}
    golden_masks(o)
    np.savez_compressed(os.path.join(HERE, "masks.npz"), **o)

    o = {}
    golden_loss(o)
    np.savez_compressed(os.path.join(HERE, "evd_loss.npz"), **o)

    o = {}
    golden_loss_indep(o)
    np.savez_compressed(os.path.join(HERE, "evd_loss_indep.npz"), **o)
    o = {}
    golden_amp(o)
    np.savez_compressed(os.path.join(HERE, "amp.npz"), **o)

    o = {}
    golden_ground_truth(o)
    golden_debug_model(o)
    np.savez_compressed(os.path.join(HERE, "misc.npz"), **o)

    o = {}
    golden_cdk(o)
    np.savez_compressed(os.path.join(HERE, "cdk_loss.npz"), **o)

    # small seeded models (fit the MFMA fast path: H=32 blocks) -----------------
    o = {}
    golden_model(o, "hyd_small", potential_type="hydrogen", neigs=4, mlp_hidden_dims="32,32",
                 fourier_mapping_size=16, fourier_scale=0.1, sampling_scale=16.0, batch_size=24,
                 operator_scale=100.0, operator_shift=0.0, lim=5.0, val_eps=0.5, sequential=1)
    golden_model(o, "osc_small", potential_type="harmonic_oscillator", neigs=5, mlp_hidden_dims="32,32,32",
                 fourier_mapping_size=16, fourier_scale=1.0, sampling_scale=4.0, batch_size=32,
                 operator_scale=1.0, operator_shift=16.0, apply_exp_mask=1, exp_mask_init_scale=10.0,
                 lim=5.0, val_eps=0.5, sequential=0)
    # ragged shapes: generic path (H not multiple of 32, odd B, odd m, step>1 joint)
    golden_model(o, "hyd_ragged", potential_type="hydrogen", neigs=3, mlp_hidden_dims="12,20",
                 fourier_mapping_size=5, fourier_scale=0.1, sampling_scale=16.0, batch_size=11,
                 operator_scale=100.0, operator_shift=0.0, lim=2.0, val_eps=0.5, sequential=0, step=2)
    np.savez_compressed(os.path.join(HERE, "model_small.npz"), **o)

    # medium: H=128x3 (the headline hidden sizes) at reduced L/B/m --------------
    o = {}
    golden_model(o, "hyd_med", nsteps=1, grid=False, store_params=False, sample_stride=997,
                 potential_type="hydrogen", neigs=4, mlp_hidden_dims="128,128,128",
                 fourier_mapping_size=64, fourier_scale=0.1, sampling_scale=16.0, batch_size=64,
                 operator_scale=100.0, operator_shift=0.0, sequential=0, seed=3)
    # cfg1-shaped (hydrogen L=16 B=128 seq, m=1024): outputs only, params from the seed recipe
    golden_model(o, "cfg1", nsteps=1, grid=False, store_params=False, sample_stride=9973,
                 potential_type="hydrogen", neigs=16, mlp_hidden_dims="128,128,128",
                 fourier_mapping_size=1024, fourier_scale=0.1, sampling_scale=16.0, batch_size=128,
                 operator_scale=100.0, operator_shift=0.0, sequential=1, seed=0)
    np.savez_compressed(os.path.join(HERE, "model_headline.npz"), **o)
    # exact-Laplacian mode (laplacian_eps = 0: VectorizedLaplacian.exact_laplacian, diff_ops.py:54-61,64-111) ----
    o = {}
    golden_model(o, "hyd_exact", nsteps=1, grid=False, store_params=True, sample_stride=13, laplacian_eps=0.0,
                 potential_type="hydrogen", neigs=3, mlp_hidden_dims="128,128", fourier_mapping_size=64,
                 fourier_scale=0.1, sampling_scale=16.0, batch_size=32, operator_scale=100.0, operator_shift=0.0,
                 sequential=0, seed=7)
    golden_model(o, "osc_exact", nsteps=1, grid=False, store_params=True, sample_stride=13, laplacian_eps=0.0,
                 potential_type="harmonic_oscillator", neigs=2, mlp_hidden_dims="128,128,128",
                 fourier_mapping_size=64, fourier_scale=1.0, sampling_scale=4.0, batch_size=32, operator_scale=1.0,
                 operator_shift=16.0, apply_exp_mask=1, exp_mask_init_scale=10.0, sequential=1, seed=8)
    golden_model(o, "osc_exact_small", nsteps=1, grid=False, store_params=True, laplacian_eps=0.0,
                 potential_type="harmonic_oscillator", neigs=3, mlp_hidden_dims="12,9", fourier_mapping_size=5,
                 fourier_scale=1.0, sampling_scale=4.0, batch_size=7, operator_scale=1.0, operator_shift=16.0,
                 apply_exp_mask=1, exp_mask_init_scale=10.0, sequential=0, seed=9)
    np.savez_compressed(os.path.join(HERE, "model_exact.npz"), **o)
    for fn in ("tower", "kernel_loss", "masks", "evd_loss", "evd_loss_indep", "amp", "cdk_loss", "svd_loss", "normalize", "misc", "model_small", "model_headline", "model_exact"):
        p = os.path.join(HERE, fn + ".npz")
        print(fn, os.path.getsize(p) // 1024, "KiB")


if __name__ == "__main__":
    main()
