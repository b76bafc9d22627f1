#!/usr/bin/env python3
"""Generate tests/golden/eigfuncs.npz by IMPORTING the reference: the analytic eigenfunctions and level structure of
the three 2-D ground truths (examples/operator/pde/schrodinger/ground_truths.py: get_qnums, get_degeneracy, get_eigvals,
eigfunc of Hydrogen2D, HarmonicOscillator and InfiniteWell2D) and the subspace metrics of examples/linalg.py
(subspace_distance, rotate, procrustes).

Runs only where the reference checkout that make_golden.py imports is present (it needs scipy: the reference's
hyp1f1 and sqrtm); the test-suite never runs it, it only reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eigfuncs.py

Points: float32 coordinates, widened to float64 before the reference sees them (what the kernel does). Both signs of
each coordinate, the four axes, r from 1e-3 to 70; r = 0 is left out (the reference's hydrogen formula is NaN there).
The well's points lie in and on the box [-5, 5]^2 and are handed to the reference shifted to [0, 10]. No reference
source text is stored: fixtures are arrays only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402,F401  (installs the stubs and puts the reference on sys.path)

from examples.operator.pde.schrodinger.ground_truths import (  # noqa: E402
    Hydrogen2D, HarmonicOscillator, InfiniteWell2D, cartesian_to_polar)
from examples.linalg import subspace_distance, rotate, procrustes  # noqa: E402

WELL_LIM = 5.0


def points():
    g = np.random.default_rng(20)
    radii = np.array([1e-3, 1e-2, 0.1, 0.5, 1.0, 2.0, 3.5, 5.0, 8.0, 12.0, 20.0, 35.0, 50.0, 70.0])
    ang = g.uniform(0, 2 * np.pi, (2, len(radii)))
    rows = [np.stack([r * np.cos(a), r * np.sin(a)], 1) for a in ang for r in [radii]]
    axes = np.array([[1.5, 0], [-1.5, 0], [0, 2.5], [0, -2.5], [30, 0], [0, -30], [-1e-3, 0], [0, 70.0]])
    quad = np.array([[3, 4], [-3, 4], [3, -4], [-3, -4]], dtype=np.float64)
    return np.concatenate(rows + [axes, quad]).astype(np.float32)


def well_points():
    g = np.random.default_rng(21)
    inner = g.uniform(-WELL_LIM, WELL_LIM, (24, 2))
    walls = np.array([[WELL_LIM, 1.0], [-WELL_LIM, -2.0], [0.5, WELL_LIM], [3.0, -WELL_LIM], [WELL_LIM, WELL_LIM],
                      [0, 0], [2.5, 0], [0, -2.5], [-WELL_LIM, WELL_LIM]])
    return np.concatenate([inner, walls]).astype(np.float32)


def orthonormalise(A):
    w, V = np.linalg.eigh(A.T @ A)
    return A @ ((V / np.sqrt(w)) @ V.T)


def main():
    out = {}
    x = points()
    x64 = x.astype(np.float64)
    out["x"] = x
    hyd = Hydrogen2D(charge=1.0)
    for neigs in (5, 16, 64):
        out[f"hyd_qnums_{neigs}"] = np.array(hyd.get_qnums(neigs), dtype=np.int64)
        out[f"hyd_degeneracy_{neigs}"] = np.asarray(hyd.get_degeneracy(neigs), dtype=np.int64)
        out[f"hyd_eigvals_{neigs}"] = np.asarray(hyd.get_eigvals(neigs), dtype=np.float64)
    r, th = cartesian_to_polar(x64[:, 0], x64[:, 1])
    out["hyd_psi"] = np.stack([hyd.eigfunc(n, l, r, th) for n, l in hyd.get_qnums(64)], 1)
    osc = HarmonicOscillator(k=1.0, ndim=2)
    for neigs in (4, 32, 66):
        out[f"osc_qnums_{neigs}"] = np.asarray(osc.get_qnums(neigs), dtype=np.int64)
        out[f"osc_degeneracy_{neigs}"] = np.asarray(osc.get_degeneracy(neigs), dtype=np.int64)
        out[f"osc_eigvals_{neigs}"] = np.asarray(osc.get_eigvals(neigs), dtype=np.float64)
    out["osc_psi"] = np.stack([osc.eigfunc(int(a), int(b), x64[:, 0], x64[:, 1]) for a, b in osc.get_qnums(66)], 1)
    well = InfiniteWell2D(L=2 * WELL_LIM)
    xw = well_points()
    out["well_x"] = xw
    out["well_lim"] = np.float64(WELL_LIM)
    out["well_qnums_8"] = np.array(well.get_qnums(8), dtype=np.int64)
    out["well_degeneracy_8"] = np.asarray(well.get_degeneracy(8), dtype=np.int64)
    out["well_eigvals_8"] = np.asarray(well.get_eigvals(8), dtype=np.float64)
    xs = xw.astype(np.float64) + WELL_LIM
    out["well_psi"] = np.stack([well.eigfunc(a, b, xs[:, 0], xs[:, 1]) for a, b in well.get_qnums(8)], 1)
    # examples/linalg.py on two small random pairs: (d, k) blocks cut out of wider matrices by (start, end)
    g = np.random.default_rng(22)
    for i, (d, width, s, e) in enumerate(((50, 3, 0, 3), (40, 9, 4, 9))):
        A = g.standard_normal((d, width))
        Ahat = A @ (np.eye(width) + 0.3 * g.standard_normal((width, width))) + 0.2 * g.standard_normal((d, width))
        out[f"lin{i}_A"], out[f"lin{i}_Ahat"] = A, Ahat
        out[f"lin{i}_range"] = np.array([s, e], dtype=np.int64)
        out[f"lin{i}_subspace_distance"] = np.float64(subspace_distance(A[:, s:e], Ahat[:, s:e]))
        out[f"lin{i}_rotate"] = np.real(rotate(A, Ahat, s, e))
        # procrustes on the symmetrically orthonormalised blocks: target A_, learned Ahat_
        An, Ahn = orthonormalise(A[:, s:e]), orthonormalise(Ahat[:, s:e])
        out[f"lin{i}_procrustes"] = procrustes(An, Ahn, 0, e - s)
    path = os.path.join(HERE, "eigfuncs.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")
    assert all(np.isfinite(v).all() for v in out.values())


if __name__ == "__main__":
    main()
