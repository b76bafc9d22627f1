#!/usr/bin/env python3
"""Generate tests/golden/spin.npz by IMPORTING the reference's SpIN (methods/spin.py) and get_wavefunctions.

Needs the reference checkout (imported the way make_golden.py does); the test-suite never runs this, it only reads the
committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spin.py

Per case of tests/_spin_oracle.py:CASES and both split_batch modes: NSTEPS steps of the reference's loop body
(compute_loss_kernel, backward, a plain SGD update) on a DENSE DIFFERENTIABLE Gaussian-kernel operator
op(model, x) = (k(x, x_ref) @ model(x_ref) / B2, model(x)), in float64 (stored) and again in float32 (stored as its error
against the float64 run, quantity by quantity: the tests' tolerance is max(1e-4, 4 x that error)). Tensors above
SAMPLE_ABOVE elements are stored as a strided sample (_spin_oracle.sample). A case is admitted only if
cond(sigma_avg + 1e-3 I) <= COND_MAX at every recorded step: asserted here, so that no test passes on noise.
No reference source text is stored: fixtures are arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)
import _spin_oracle as S  # noqa: E402

from methods.spin import SpIN  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402


def dense_kernel_op_factory(ell):
    def get_approx_kernel_op(x_ref):
        def op(model, x, importance=None):
            Kmat = torch.exp(-torch.cdist(x, x_ref) ** 2 / (2.0 * ell ** 2))
            return Kmat @ model(x_ref) / x_ref.shape[0], model(x)
        return op
    return get_approx_kernel_op


def build(name, dtype):
    cs = S.CASES[name]
    args = G.make_args(ndim=cs["D"], neigs=cs["L"], mlp_hidden_dims=",".join(str(h) for h in cs["hidden"]),
                       fourier_mapping_size=cs["m"], fourier_scale=S.FOURIER_SCALE, seed=S.case_seed(name),
                       hard_mul_const=S.case_c(name))
    torch.manual_seed(args.seed)
    model = get_wavefunctions(args)
    return SpIN(model, cs["L"], cs["decay"], use_vmap=True).to(dtype)


def trainable(method):
    named = dict(method.model.named_parameters())
    n = len([k for k in named if k.startswith("base.ws.")])
    return [f"base.ws.{i}" for i in range(n)] + [f"base.bs.{i}" for i in range(n)], named


def run_case(out, name):
    cs = S.CASES[name]
    torch.manual_seed(S.case_seed(name) + 1000)
    xs = S.X_SCALE * torch.randn(S.NSTEPS, cs["B"], cs["D"])
    out[f"{name}_x"] = xs.numpy()
    m0 = build(name, torch.float32)
    names, named = trainable(m0)
    n = len(names) // 2
    if sum(named[k].numel() for k in names) <= S.STORE_PARAMS_UP_TO:
        out[f"{name}_fB"] = named["base.feature_map._B"].detach().numpy().copy()
        for i in range(n):
            out[f"{name}_w{i}"] = named[names[i]].detach().numpy().copy()
            out[f"{name}_b{i}"] = named[names[n + i]].detach().numpy().copy()
    else:  # rebuilt from the seed by the tests: the recipe must reproduce the reference's draw
        fB, ws, bs = S.init_params(cs["L"], cs["D"], cs["m"], cs["hidden"], S.case_seed(name))
        assert torch.equal(fB, named["base.feature_map._B"].detach())
        for i in range(n):
            assert torch.equal(ws[i], named[names[i]].detach()) and torch.equal(bs[i], named[names[n + i]].detach())
    worst = 0.0
    for split in (False, True):
        rec = {}
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            method = build(name, dtype)
            names, named = trainable(method)
            for it in range(S.NSTEPS):
                method.zero_grad()
                x = xs[it].to(dtype)
                loss, aux = method.compute_loss_kernel(dense_kernel_op_factory(S.ELL), x, None, split_batch=split)
                term2 = [named[k].grad.detach().clone() for k in names]
                loss.backward()
                q = dict(loss=loss, eigvals=aux["eigvals"], sigma_avg=method.sigma_avg, chol=method.chol, phi=aux["f"],
                         Kphi=aux["Tf"])
                for i, k in enumerate(names):
                    q[f"term2_{i}"] = term2[i]
                    q[f"grad_{i}"] = named[k].grad
                rec[(tag, it)] = {k: S.sample(v.detach().double()).clone() for k, v in q.items()}
                if tag == "f64":
                    cond = float(torch.linalg.cond(method.sigma_avg.detach() + 1e-3 * torch.eye(cs["L"], dtype=dtype)))
                    assert cond <= S.COND_MAX, (name, split, it, cond)
                    rec[(tag, it)]["cond"] = torch.tensor([cond], dtype=torch.float64)
                with torch.no_grad():
                    for k in names:
                        named[k] -= S.LR * named[k].grad
            if tag == "f64" and name == "t3":
                for i, k in enumerate(names):
                    out[f"{name}_s{int(split)}_javg_{i}"] = G.np64(method.j_avg[k.replace(".", "_")])
        for it in range(S.NSTEPS):
            p = f"{name}_s{int(split)}_k{it}_"
            r64, r32 = rec[("f64", it)], rec[("f32", it)]
            keys = S.quantity_names(len(names))
            errs = [S.rel_err(r32[k], r64[k]) for k in keys]
            out[p + "vals"] = torch.cat([r64[k].reshape(-1) for k in keys]).numpy()
            out[p + "sizes"] = np.array([r64[k].numel() for k in keys], dtype=np.int32)
            out[p + "err32"] = np.array(errs)
            out[p + "cond"] = r64["cond"].numpy()[0]
            worst = max([worst] + [e for k, e in zip(keys, errs) if k.startswith(("term2", "grad"))])
    print(f"{name}: worst float32 gradient error {worst:.2e}")


def main():
    out = {}
    for name in S.CASES:
        run_case(out, name)
    path = os.path.join(HERE, "spin.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
