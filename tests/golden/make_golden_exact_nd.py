#!/usr/bin/env python3
"""Generate tests/golden/exact_nd.npz by IMPORTING the reference: its exact-Laplacian mode (laplacian_eps <= 0:
VectorizedLaplacian.exact_laplacian, examples/operator/pde/diff_ops.py:54-61) above four input dimensions - the cosine
Schroedinger problem at ndim 5 and the H2 molecule at ndim 3 (D = 6).

Runs only where the reference checkout that make_golden.py imports is present; the test-suite never runs it, it only
reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_exact_nd.py

Per case, in float64 and in float32: ONE evaluation of the reference's compute_loss_operator + backward on the same
batch and the same float32 initial weights, recording x, f, Tf, the loss and every parameter gradient. Both cases: neigs
3, batch 8, hidden (16, 16), mapping size 8, laplacian_eps 0. The batches are plain draws of the case's sampler, from the
first seed at which no row is within 0.1 of a nucleus or a coalescence point (asserted below; the exact mode has no
stencil that could straddle one). No reference source text is stored: arrays and reprs only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)
import make_golden_box as GB  # noqa: E402
import make_golden_highdim as GH  # noqa: E402

SMALL = dict(batch_size=8, neigs=3, laplacian_eps=0.0)
CASES = dict(
    cos_5d=dict(GH.CASES["cos_5d"], **SMALL),
    h2_3d=dict(GH.CASES["h2_3d"], **SMALL),
)


def draw_x(args, mol):
    shape = (args.batch_size, args.n_particles, args.ndim)
    for seed in range(args.seed + 4000, args.seed + 4100):
        torch.manual_seed(seed)
        if args.sampling_mode == "uniform":
            x = args.sampling_scale * (2 * torch.rand(shape) - 1)
        else:
            x = args.sampling_scale * torch.randn(shape)
        x = x.reshape(args.batch_size, -1).clone()
        if mol is None:
            return x, seed
        en, ee = GH.min_distances(x, mol, args.n_particles)
        if float(en.min()) > 0.1 and float(ee.min()) > 0.1:
            return x, seed
    raise AssertionError("no clear batch")


def run_case(out, name, case):
    args = G.make_args(**case)
    operator, gt, method0, mol = GH.build(args)
    x, seed = draw_x(args, mol)
    out[f"{name}_x"] = x.numpy()[None]
    out[f"{name}_x_seed"] = np.array(seed)
    assert out[f"{name}_x"].dtype == np.float32
    out[f"{name}_param_names"] = np.array([n for n, t in method0.named_parameters() if t.requires_grad])
    for n, t in method0.named_parameters():
        if t.requires_grad:
            out[f"{name}_param0_{n}"] = t.detach().float().numpy()
        elif n.endswith("feature_map._B"):
            out[f"{name}_fourier_B"] = t.detach().float().numpy()
    out[f"{name}_cfg"] = np.array(repr({k: v for k, v in vars(args).items() if k != "loss"}))
    if mol is not None:
        out[f"{name}_mol_coords"] = mol.coords.numpy()
        out[f"{name}_mol_charges"] = mol.charges.numpy()
    state = {k: v.detach().clone() for k, v in method0.state_dict().items()}
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        operator, gt, method, mol = GH.build(G.make_args(**case))
        method.load_state_dict(state)
        method = method.to(dtype)
        method.train()
        loss, aux = method.compute_loss_operator(operator, x.to(dtype), importance=GB.importance_for(args, dtype))
        loss.backward()
        assert bool(torch.isfinite(aux["f"]).all()) and bool(torch.isfinite(aux["Tf"]).all())
        p = f"{name}_{tag}_step0_"
        out[p + "loss"] = G.np64(loss)
        out[p + "f"] = G.np64(aux["f"])
        out[p + "Tf"] = G.np64(aux["Tf"])
        for n, t in method.named_parameters():
            if t.requires_grad:
                out[p + f"grad_{n}"] = G.np64(t.grad)


def main():
    out = {}
    for name, case in CASES.items():
        run_case(out, name, case)
    path = os.path.join(HERE, "exact_nd.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
