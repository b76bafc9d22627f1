#!/usr/bin/env python3
"""Generate tests/golden/nystrom.npz by IMPORTING the reference's Nystrom (methods/nystrom.py:8-47), the anchor of
tests/_nystrom_oracle.py.

Runs only where the reference checkout that make_golden.py imports is present; the test-suite never runs it, it only
reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nystrom.py

Both kernel kinds on xs = randn(96, 2) (seed 0), xnew = randn(40, 2), dim 6; ell 1.5 (Gaussian), 2.0 (exponential).
The kernel handed to the reference is the float32 torch composition a user of it would write (direct differences,
exp); the reference then runs its own float32 np.linalg.eigh on the host. Stored: the inputs, eigvals, eigvecs and
Nystrom(xnew). No reference source text is stored: the fixture is arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as G  # noqa: E402,F401  (installs the stubs and puts the reference on sys.path)

from methods.nystrom import Nystrom  # noqa: E402

N, NNEW, D, DIM = 96, 40, 2, 6
ELL = {"gaussian": 1.5, "exponential": 2.0}


def kernel_fn(kind, ell):
    def k(a, b):
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        return torch.exp(-d2 / (2.0 * ell ** 2)) if kind == "gaussian" else torch.exp(-d2.sqrt() / ell)
    return k


def main():
    g = torch.Generator().manual_seed(0)
    xs = torch.randn(N, D, generator=g)
    xnew = torch.randn(NNEW, D, generator=g)
    out = dict(xs=xs.numpy(), xnew=xnew.numpy(), dim=np.array(DIM))
    for kind, ell in ELL.items():
        ny = Nystrom(kernel_fn(kind, ell), xs, DIM)
        out[f"ell_{kind}"] = np.array(ell)
        out[f"eigvals_{kind}"] = ny.eigvals.numpy()
        out[f"eigvecs_{kind}"] = ny.eigvecs.numpy()
        out[f"proj_{kind}"] = ny(xnew).numpy()
    path = os.path.join(HERE, "nystrom.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
