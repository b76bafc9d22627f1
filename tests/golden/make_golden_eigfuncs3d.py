#!/usr/bin/env python3
"""Generate tests/golden/eigfuncs3d.npz by IMPORTING the reference: the level structure and the analytic
eigenfunctions of the 3-D hydrogen atom (examples/operator/pde/schrodinger/ground_truths.py: Hydrogen3D.get_qnums,
get_degeneracy, get_eigvals, eigfunc with real_sph_harm / sph_harm, cartesian_to_spherical). The reference defines
these functions and never calls eigfunc itself; this script does, for the 55 states of n <= 5 at charge 1.0 and 1.7.

Runs only where the reference checkout that make_golden.py imports is present (it needs scipy: the reference's
genlaguerre, lpmv, gamma); the test-suite never runs it, it only reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eigfuncs3d.py

Points: float32 coordinates, widened to float64 before the reference sees them (what the kernel does): the origin,
r from 1e-3 to 120 in random directions, both halves of the z axis, the x and y axes, the z = 0 plane, all eight sign
octants. The reference is finite at every one of them (arctan2(0, 0) = 0, 0 ** 0 = 1). No reference source text is
stored: fixtures are arrays only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402,F401  (installs the stubs and puts the reference on sys.path)

from examples.operator.pde.schrodinger.ground_truths import Hydrogen3D, cartesian_to_spherical  # noqa: E402

CHARGES = (1.0, 1.7)


def points():
    g = np.random.default_rng(30)
    radii = np.array([1e-3, 1e-2, 0.1, 0.3, 0.7, 1.0, 1.5, 2.0, 3.0, 4.5, 6.0, 8.0, 11.0, 15.0, 20.0, 27.0, 35.0, 50.0,
                      70.0, 90.0, 120.0])
    d = g.standard_normal((len(radii), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    origin = np.zeros((1, 3))
    zaxis = np.array([[0, 0, 1e-3], [0, 0, 0.8], [0, 0, 5.0], [0, 0, 40.0], [0, 0, -1e-3], [0, 0, -2.5], [0, 0, -30.0]])
    xyaxes = np.array([[1.5, 0, 0], [-1.5, 0, 0], [0, 2.5, 0], [0, -2.5, 0], [25.0, 0, 0], [0, -60.0, 0]])
    plane = np.array([[1.0, 2.0, 0], [-3.0, 0.5, 0], [-0.2, -0.9, 0], [7.0, -4.0, 0], [12.0, 9.0, 0]])
    octants = np.array([[sx * 1.0, sy * 2.0, sz * 3.0] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)])
    far = np.array([[4.0, -6.0, 9.0], [-0.3, 0.1, -0.2], [0.05, 0.02, 4.0], [3.0, 3.0, 1e-4]])
    return np.concatenate([origin, radii[:, None] * d, zaxis, xyaxes, plane, octants, far]).astype(np.float32)


def main():
    out = {}
    x = points()
    out["x"] = x
    x64 = x.astype(np.float64)
    r, th, phi = cartesian_to_spherical(x64[:, 0], x64[:, 1], x64[:, 2])
    for neigs in (5, 14, 55):
        hyd = Hydrogen3D(charge=1.0)
        out[f"qnums_{neigs}"] = np.array(hyd.get_qnums(neigs), dtype=np.int64)
        out[f"degeneracy_{neigs}"] = np.asarray(hyd.get_degeneracy(neigs), dtype=np.int64)
        out[f"eigvals_{neigs}"] = np.asarray(hyd.get_eigvals(neigs), dtype=np.float64)
    out["charges"] = np.array(CHARGES)
    for i, Z in enumerate(CHARGES):
        hyd = Hydrogen3D(charge=Z)
        psi = np.stack([hyd.eigfunc(n, l, m, r, th, phi) for n, l, m in hyd.get_qnums(55)], 1)
        assert np.isrealobj(psi)
        out[f"psi_{i}"] = psi
    path = os.path.join(HERE, "eigfuncs3d.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays, {len(x)} points")
    assert all(np.isfinite(v).all() for v in out.values())


if __name__ == "__main__":
    main()
