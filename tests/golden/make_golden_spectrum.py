#!/usr/bin/env python3
"""Generate tests/golden/spectrum_acc.npz by IMPORTING the reference: the accumulation of compute_spectrum_evd
(methods/spectrum.py:29-87) on recorded (Tphi, phi), the anchor of tests/_spectrum_oracle.py.

Runs only where the reference checkout that make_golden.py imports is present; the test-suite never runs it, it only
reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spectrum.py

The reference's own compute_spectrum_evd is called with float64 tensors, a stub operator that hands back the recorded
(Tphi, phi) of each batch, importance_val as main_pde.py:129-130 builds it (a FLOAT32 tensor of 1 / (2 lim)^D) and
importance_train the constant 1 or the N(0, sigma^2 I) density in float64; set_first_mode_const False and True; D = 1, 2, 3.
40 rows in two batches (23 + 17: cov and quad are sums over batches, divided by n at the end). Planted: the origin,
|x_d| = 5e-9 on every axis, (0, 1, ...), one coordinate 2e-8, and a few NaN entries in f and Tf (no +-inf: the
reference's float64 nan_to_num maps them to the float64 maximum, which is not the float32 rule of the kernels).
No reference source text is stored: the fixture is arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)

from methods.spectrum import compute_spectrum_evd  # noqa: E402
from tests._spectrum_oracle import planted_rows  # noqa: E402

B, L, SIGMA, LIM = 40, 4, 16.0, 50.0
SPLIT = 23
DIMS = (1, 2, 3)


def inputs():
    g = torch.Generator().manual_seed(20240607)
    f = torch.randn(B, L, generator=g)
    Tf = 30.0 * torch.randn(B, L, generator=g)
    f[3, 1] = f[25, 0] = f[31, 3] = float("nan")
    Tf[3, 2] = Tf[12, 0] = Tf[31, 3] = float("nan")
    Tf[5, 1] = float("nan")      # (row 5 is the origin row: zeroed after nan_to_num)
    xs = {}
    for D in DIMS:
        x = SIGMA * torch.randn(B, D, generator=g)
        x[5:9] = torch.tensor(planted_rows(D))
        xs[D] = x
    return f, Tf, xs


def run(f, Tf, x, gaussian, pad):
    D = x.shape[1]
    x64, f64, Tf64 = x.double(), f.double(), Tf.double()
    batches = [(0, SPLIT), (SPLIT, B)]
    queue = list(batches)

    def operator(model, xb, importance=None):
        a, b = queue.pop(0)
        assert torch.equal(xb, x64[a:b])
        return Tf64[a:b].clone(), f64[a:b].clone()

    def loader():
        for a, b in batches:
            yield x64[a:b], 0.

    class Args:
        n_particles, ndim, sampling_scale = 1, D, SIGMA

    # (importance_train=None does not run: compute_spectrum_evd compares the shapes of the two weights, and 1. has
    # none - "no importance" is the density 1)
    imp_train = (G.importance_for(Args, torch.float64) if gaussian
                 else lambda z: torch.ones(z.shape[0], 1, dtype=torch.float64))

    def imp_val(z):  # main_pde.py:129-130: a float32 tensor
        return (1 / (2 * LIM) ** D * torch.ones(z.shape[0], 1)).float().view(-1, 1)

    res = compute_spectrum_evd(None, dataloader=loader(), operator=operator, importance_train=imp_train,
                               importance_val=imp_val, set_first_mode_const=bool(pad), normalize=False,
                               device=torch.device("cpu"))
    assert not queue
    return np.asarray(res["cov"], dtype=np.float64) * B, np.asarray(res["quad"], dtype=np.float64) * B


def main():
    f, Tf, xs = inputs()
    out = dict(f=f.numpy(), Tf=Tf.numpy(), cfg=np.array([SIGMA, LIM]), dims=np.array(DIMS))
    for D in DIMS:
        out[f"x_D{D}"] = xs[D].numpy()
        for gaussian in (0, 1):
            for pad in (0, 1):
                cov, quad = run(f, Tf, xs[D], gaussian, pad)
                out[f"cov_D{D}_g{gaussian}_p{pad}"] = cov     # (the sums: the reference's cov, quad times n)
                out[f"quad_D{D}_g{gaussian}_p{pad}"] = quad
    path = os.path.join(HERE, "spectrum_acc.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
