#!/usr/bin/env python3
"""Generate tests/golden/kernel_svd.npz by IMPORTING the reference's NestedLoRALossFunctionSVD (methods/nestedlora.py)
and get_wavefunctions.

Needs the reference checkout (imported the way make_golden.py does); the test-suite never runs this, it only reads the
committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kernel_svd.py

The kernel SVD step on a cross-domain Gaussian kernel, 64 rows a side: two reference models (f seeded with `seed`, g with
`seed + 1`), x ~ N(0, sigma_x^2 I), y ~ N(0, sigma_y^2 I) with sigma_x = 1 != sigma_y = 0.5, the kernel matrix from this
script's own float64 formula K = exp(-|x_i - y_j|^2 / (2 ell^2)), Tg = K g / B2 and Tadjf = K^T f / B1 (no gradient),
the reference's Function on (f, Tg, g, Tadjf) and loss.backward() into both models. Stored per case: the float64 run's
loss, f, g, Tg, Tadjf and every parameter gradient (above 4096 elements: norm plus every 61st element, as
kernel_loss.npz stores them), and the float32 run's distance from float64, quantity by quantity (`<case>_f32err_<key>`:
relative 2-norm distance, for the loss the absolute difference). No reference source text is stored: arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)

from methods.nestedlora import NestedLoRA, NestedLoRALossFunctionSVD  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402

B, SIGMA_X, SIGMA_Y = 64, 1.0, 0.5
CASES = dict(
    sa=dict(ndim=1, neigs=3, mlp_hidden_dims="32,32", fourier_mapping_size=16, sequential=0, step=1, seed=31),
    sb=dict(ndim=3, neigs=6, mlp_hidden_dims="32,32", fourier_mapping_size=16, sequential=1, step=1, seed=32),
    sc=dict(ndim=16, neigs=8, mlp_hidden_dims="128,128", fourier_mapping_size=64, sequential=0, step=2, seed=33),
)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def run(name, over, dtype):
    args = G.make_args(fourier_scale=0.3, batch_size=B, **dict(over))
    torch.manual_seed(args.seed)
    model_f = get_wavefunctions(args).to(dtype)
    torch.manual_seed(args.seed + 1)
    model_g = get_wavefunctions(args).to(dtype)
    torch.manual_seed(args.seed + 500)
    x32 = SIGMA_X * torch.randn(B, args.ndim)
    y32 = SIGMA_Y * torch.randn(B, args.ndim)
    ell = 1.5 * float(args.ndim) ** 0.5
    x, y = x32.to(dtype), y32.to(dtype)
    m = NestedLoRA(model=None, neigs=args.neigs, step=over["step"], sequential=bool(over["sequential"]))
    f, g = model_f(x), model_g(y)
    with torch.no_grad():
        K = torch.exp(-((x[:, None, :] - y[None, :, :]) ** 2).sum(-1) / (2.0 * ell ** 2))
        Tg, Tadjf = K @ g / B, K.T @ f / B
    loss = NestedLoRALossFunctionSVD.apply(f, Tg, g, Tadjf, m.vector_mask.to(dtype), m.matrix_mask.to(dtype))
    loss.backward()
    q = dict(loss=G.np64(loss), f=G.np64(f), g=G.np64(g), Tg=G.np64(Tg), Tadjf=G.np64(Tadjf))
    for side, model in (("f", model_f), ("g", model_g)):
        for n, t in model.named_parameters():
            if t.grad is not None:
                q[f"grad_{side}.{n}"] = G.np64(t.grad)
    cfg = {k: v for k, v in vars(args).items() if k != "loss"}
    cfg["sequential"], cfg["step"] = int(over["sequential"]), int(over["step"])
    meta = dict(x=x32.numpy(), y=y32.numpy(), ell=np.array(ell), sigma=np.array([SIGMA_X, SIGMA_Y]),
                v=m.vector_mask.numpy(), M=m.matrix_mask.numpy(), cfg=np.array(repr(cfg)))
    return q, meta


def main():
    out = {}
    for name, over in CASES.items():
        q64, meta = run(name, over, torch.float64)
        q32, _ = run(name, over, torch.float32)
        for k, v in meta.items():
            out[f"{name}_{k}"] = v
        for k, v in q64.items():
            err = abs(float(q32[k]) - float(v)) if k == "loss" else rel(q32[k], v)
            out[f"{name}_f32err_{k}"] = np.array(err)
            if k.startswith("grad_") and v.size > 4096:
                out[f"{name}_f64_gradnorm_{k[5:]}"] = np.array(np.linalg.norm(v))
                out[f"{name}_f64_gradsample_{k[5:]}"] = v.reshape(-1)[::61]
            else:
                out[f"{name}_f64_{k}"] = v
        print(name, "loss", float(q64["loss"]), "f32 errors:",
              " ".join(f"{k} {float(out[f'{name}_f32err_{k}']):.1e}" for k in q64))
    path = os.path.join(HERE, "kernel_svd.npz")
    np.savez_compressed(path, **out)
    print("kernel_svd", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
