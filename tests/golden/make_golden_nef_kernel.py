#!/usr/bin/env python3
"""Generate tests/golden/nef_kernel.npz by IMPORTING the reference's NeuralEigenfunctions (methods/neuralef.py), its
BatchL2NormalizedFunctions (methods/utils.py) and get_wavefunctions.

Needs the reference checkout (imported the way make_golden.py does); the test-suite never runs this, it only reads the
committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nef_kernel.py

Per shape of tests/_spinx_oracle.py:CASES, per variant of tests/_nef_kernel_oracle.py:variants (unbiased False / True
with batchnorm_mode 'unbiased' for every shape; 'biased', 'none' and include_diag once more for shape `a`) and both
split_batch modes: NSTEPS steps of the reference's loop body (compute_loss_kernel, backward, plain SGD), unmodified, on
a DENSE Gaussian-kernel operator. The reference ships no operator callable; this one evaluates the model the way the
package's MatrixFreeKernelOperator.get_approx_kernel_op does - model(x) first, model(x_ref) only when x_ref is another
batch - which fixes the order of the running-norm updates (segment 0 once; split: 0, 1, 1, 0). Everything in float64
(stored) and again in float32 (stored as its error against the float64 run, quantity by quantity: the tests' tolerance
is max(1e-4, 4 x that error)). Tensors above SAMPLE_ABOVE elements are stored as a strided sample.

A case is admitted only if, in the float64 run at every recorded step, min_l n / max_l n >= NORM_RATIO_MIN within every
segment and (unbiased=False) min_i |Q_ii + 1e-5| >= DIAG_RATIO_MIN max_i |Q_ii|: asserted here, so that the float32
error of the divisions stays bounded and no test passes on noise. Fixtures are arrays only.
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
from tests import _nef_kernel_oracle as N  # noqa: E402

from methods.neuralef import NeuralEigenfunctions  # noqa: E402
from methods.utils import BatchL2NormalizedFunctions  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402


def dense_kernel_op_factory(ell):
    def get_approx_kernel_op(x_ref):
        def op(model, x, importance=None):
            f = model(x)
            f_ref = f if x_ref is x else model(x_ref)
            Kmat = torch.exp(-torch.cdist(x, x_ref) ** 2 / (2.0 * ell ** 2))
            return Kmat @ f_ref.detach() / x_ref.shape[0], f
        return op
    return get_approx_kernel_op


def build(name, dtype, unbiased, mode, include_diag):
    cs = N.SHAPES[name]
    args = G.make_args(ndim=cs["D"], neigs=cs["L"], mlp_hidden_dims=",".join(str(h) for h in cs["hidden"]),
                       fourier_mapping_size=cs["m"], fourier_scale=N.FOURIER_SCALE, seed=N.case_seed(name),
                       hard_mul_const=N.case_c(name))
    torch.manual_seed(args.seed)
    model = get_wavefunctions(args)
    method = NeuralEigenfunctions(model, cs["L"], mode, unbiased=unbiased, include_diag=include_diag).to(dtype)
    assert isinstance(method.model, BatchL2NormalizedFunctions) == (mode != "none")
    return method.train()


def base_model(method):
    return method.model.base_model if isinstance(method.model, BatchL2NormalizedFunctions) else method.model


def trainable_of(method):
    named = dict(base_model(method).named_parameters())
    n = len([k for k in named if k.startswith("base.ws.")])
    return [f"base.ws.{i}" for i in range(n)] + [f"base.bs.{i}" for i in range(n)], named


def run_case(out, name):
    cs = N.SHAPES[name]
    L = cs["L"]
    torch.manual_seed(N.case_seed(name) + 1000)
    xs = N.X_SCALE * torch.randn(N.NSTEPS, cs["B"], cs["D"])
    out[f"{name}_x"] = xs.numpy()
    names, named = trainable_of(build(name, torch.float32, False, "unbiased", False))
    n = len(names) // 2
    if sum(named[k].numel() for k in names) <= N.STORE_PARAMS_UP_TO:
        out[f"{name}_fB"] = named["base.feature_map._B"].detach().numpy().copy()
        for i in range(n):
            out[f"{name}_w{i}"] = named[names[i]].detach().numpy().copy()
            out[f"{name}_b{i}"] = named[names[n + i]].detach().numpy().copy()
    else:  # rebuilt from the seed by the tests: the recipe must reproduce the reference's draw
        fB, ws, bs = N.init_params(L, cs["D"], cs["m"], cs["hidden"], N.case_seed(name))
        assert torch.equal(fB, named["base.feature_map._B"].detach())
        for i in range(n):
            assert torch.equal(ws[i], named[names[i]].detach()) and torch.equal(bs[i], named[names[n + i]].detach())
    worst, low_n, low_d = 0.0, 1.0, float("inf")
    for tag, unbiased, mode, include_diag in N.variants(name):
        for split in (False, True):
            B1, _ = N.chunk_rows(cs["B"], split)
            rec = {}
            for dtype, ftag in ((torch.float64, "f64"), (torch.float32, "f32")):
                method = build(name, dtype, unbiased, mode, include_diag)
                names, named = trainable_of(method)
                op = dense_kernel_op_factory(N.ELL)
                for it in range(N.NSTEPS):
                    method.zero_grad()
                    x = xs[it].to(dtype)
                    loss, aux = method.compute_loss_kernel(op, x, None, split_batch=split)
                    loss.backward()
                    q = dict(loss=loss, phi=aux["f"], Kphi=aux["Tf"])
                    if mode != "none":
                        q.update(norm_biased=method.model._norm_biased, norm_unbiased=method.model._norm_unbiased)
                    else:  # (no state: the trainer's buffers stay at their initial ones)
                        q.update(norm_biased=torch.ones(L, dtype=dtype), norm_unbiased=torch.ones(L, dtype=dtype))
                    for i, k in enumerate(names):
                        q[f"grad_{i}"] = named[k].grad
                    rec[(ftag, it)] = {k: N.sample(v.detach().double()).clone() for k, v in q.items()}
                    if ftag == "f64":
                        with torch.no_grad():
                            stats = None if mode == "none" else N.segment_norms(base_model(method)(x), B1)
                        nr, dr = N.admission(aux["f"].detach(), aux["Tf"].detach(), stats, B1, split, unbiased)
                        assert nr >= N.NORM_RATIO_MIN and dr >= N.DIAG_RATIO_MIN, (name, tag, split, it, nr, dr)
                        low_n, low_d = min(low_n, nr), min(low_d, dr)
                    with torch.no_grad():
                        for k in names:
                            named[k] -= N.LR * named[k].grad
            for it in range(N.NSTEPS):
                p = N.prefix(name, tag, split, it)
                r64, r32 = rec[("f64", it)], rec[("f32", it)]
                keys = N.quantity_names(len(names))
                errs = [N.rel_err(r32[k], r64[k]) for k in keys]
                out[p + "vals"] = torch.cat([r64[k].reshape(-1) for k in keys]).numpy()
                out[p + "sizes"] = np.array([r64[k].numel() for k in keys], dtype=np.int32)
                out[p + "err32"] = np.array(errs)
                worst = max([worst] + [e for k, e in zip(keys, errs) if k.startswith("grad")])
    print(f"{name}: worst float32 gradient error {worst:.2e}, lowest norm ratio {low_n:.3f}, lowest diagonal ratio "
          f"{low_d:.2e}")


def main():
    out = {}
    for name in N.SHAPES:
        run_case(out, name)
    path = os.path.join(HERE, "nef_kernel.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
