#!/usr/bin/env python3
"""Generate tests/golden/spinx.npz by IMPORTING the reference's SpINx (methods/spinx.py) and get_wavefunctions.

Needs the reference checkout (imported the way make_golden.py does); the test-suite never runs this, it only reads the
committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spinx.py

The reference's SpINx._compute_loss assigns plain tensors to ``sigma_avg`` and ``chol``, which its constructor registers
as nn.Parameter, and raises. The intent is SpIN's ``.data`` update; here the two names are deleted from the method's
``_parameters`` and set as plain zero tensors, after which the reference's own compute_loss_kernel, _compute_loss and
backward run unmodified. No reference code is restated.

Per case of tests/_spinx_oracle.py:CASES and both split_batch modes, on a DENSE DIFFERENTIABLE Gaussian-kernel operator
op(model, x) = (k(x, x_ref) @ model(x_ref) / B2, model(x)): NSTEPS steps of the reference's loop body
(compute_loss_kernel, backward, plain SGD) with unit weights, one more step with nonuniform_weights, then
update_weights_kernel's recipe on the last batch: the reference's jac_model_params on its SpINxLossFunctionKernel and its
own _update_weights, with the two keys that never train (the frozen Fourier matrix and trace_weights) dropped from the
Jacobian dictionary. Everything in float64 (stored) and again in float32 (stored as its error against the float64 run,
quantity by quantity: the tests' tolerance is max(1e-4, 4 x that error)). Tensors above SAMPLE_ABOVE elements are stored
as a strided sample. A case is admitted only if cond(sigma_batch + 1e-3 I) <= COND_MAX at every recorded step.
Fixtures are arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)
from tests import _spinx_oracle as X  # noqa: E402

from methods.spin import jac_model_params  # noqa: E402
from methods.spinx import SpINx, SpINxLossFunctionKernel  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402
from make_golden_spin import dense_kernel_op_factory, trainable  # noqa: E402

FROZEN = ("model.base.feature_map._B", "spinx_loss_ftn.trace_weights")


def build(name, dtype):
    cs = X.CASES[name]
    args = G.make_args(ndim=cs["D"], neigs=cs["L"], mlp_hidden_dims=",".join(str(h) for h in cs["hidden"]),
                       fourier_mapping_size=cs["m"], fourier_scale=X.FOURIER_SCALE, seed=X.case_seed(name),
                       hard_mul_const=X.case_c(name))
    torch.manual_seed(args.seed)
    model = get_wavefunctions(args)
    method = SpINx(model, cs["L"], cs["decay"]).to(dtype)
    for key in ("sigma_avg", "chol"):  # the registration workaround (see the docstring)
        del method._parameters[key]
        setattr(method, key, torch.zeros(cs["L"], cs["L"], dtype=dtype))
    method.weights = method.weights.to(dtype)
    return method


def run_case(out, name):
    cs = X.CASES[name]
    L = cs["L"]
    torch.manual_seed(X.case_seed(name) + 1000)
    xs = X.X_SCALE * torch.randn(X.NSTEPS + 1, cs["B"], cs["D"])
    out[f"{name}_x"] = xs.numpy()
    m0 = build(name, torch.float32)
    names, named = trainable(m0)
    n = len(names) // 2
    if sum(named[k].numel() for k in names) <= X.STORE_PARAMS_UP_TO:
        out[f"{name}_fB"] = named["base.feature_map._B"].detach().numpy().copy()
        for i in range(n):
            out[f"{name}_w{i}"] = named[names[i]].detach().numpy().copy()
            out[f"{name}_b{i}"] = named[names[n + i]].detach().numpy().copy()
    else:  # rebuilt from the seed by the tests: the recipe must reproduce the reference's draw
        fB, ws, bs = X.init_params(L, cs["D"], cs["m"], cs["hidden"], X.case_seed(name))
        assert torch.equal(fB, named["base.feature_map._B"].detach())
        for i in range(n):
            assert torch.equal(ws[i], named[names[i]].detach()) and torch.equal(bs[i], named[names[n + i]].detach())
    worst, worst_cond = 0.0, 0.0
    for split in (False, True):
        rec, wts = {}, {}
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            method = build(name, dtype)
            names, named = trainable(method)
            op = dense_kernel_op_factory(X.ELL)
            for it in range(X.NSTEPS + 1):
                if it == X.NSTEPS:
                    method.weights = X.nonuniform_weights(L).to(dtype)
                method.zero_grad()
                x = xs[it].to(dtype)
                loss, aux = method.compute_loss_kernel(op, x, None, split_batch=split)
                loss.backward()
                q = dict(loss=loss, phi=aux["f"], Kphi=aux["Tf"], sigma_avg=method.sigma_avg, chol=method.chol)
                for i, k in enumerate(names):
                    q[f"grad_{i}"] = named[k].grad
                rec[(tag, it)] = {k: X.sample(v.detach().double()).clone() for k, v in q.items()}
                if tag == "f64":
                    with torch.no_grad():
                        phi_all = method.model(x)
                        sig = phi_all.T @ phi_all / len(x)
                    cond = float(torch.linalg.cond(sig + 1e-3 * torch.eye(L, dtype=dtype)))
                    assert cond <= X.COND_MAX, (name, split, it, cond)
                    worst_cond = max(worst_cond, cond)
                    rec[(tag, it)]["cond"] = torch.tensor([cond], dtype=torch.float64)
                with torch.no_grad():
                    for k in names:
                        named[k] -= X.LR * named[k].grad
            method.zero_grad()
            jac = jac_model_params(SpINxLossFunctionKernel(method.model, L, op, None, split), xs[X.NSTEPS].to(dtype),
                                   use_vmap=False)
            assert all(k in jac for k in FROZEN)
            # (_update_weights accumulates into a float32 vector whatever the Jacobians' dtype: the float64 run's
            # weights carry that rounding, ~1e-7)
            method._update_weights({k: v.detach() for k, v in jac.items() if k not in FROZEN})
            wts[tag] = method.weights.double().clone()
        for it in range(X.NSTEPS + 1):
            p = f"{name}_s{int(split)}_k{it}_"
            r64, r32 = rec[("f64", it)], rec[("f32", it)]
            keys = X.quantity_names(len(names))
            errs = [X.rel_err(r32[k], r64[k]) for k in keys]
            out[p + "vals"] = torch.cat([r64[k].reshape(-1) for k in keys]).numpy()
            out[p + "sizes"] = np.array([r64[k].numel() for k in keys], dtype=np.int32)
            out[p + "err32"] = np.array(errs)
            out[p + "cond"] = r64["cond"].numpy()[0]
            worst = max([worst] + [e for k, e in zip(keys, errs) if k.startswith("grad")])
        out[f"{name}_s{int(split)}_weights"] = wts["f64"].numpy()
        out[f"{name}_s{int(split)}_weights_err32"] = np.array(X.rel_err(wts["f32"], wts["f64"]))
    print(f"{name}: worst float32 gradient error {worst:.2e}, worst cond {worst_cond:.1e}")


def main():
    out = {}
    for name in X.CASES:
        run_case(out, name)
    path = os.path.join(HERE, "spinx.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
