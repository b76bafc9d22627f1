"""3-D hydrogen eigenfunctions on the host: operators.Hydrogen3D (get_qnums, get_degeneracy, eigfunc),
eigfuncs.ground_truth_table_3d, the float64 oracle tests/_eigfunc3d_oracle.py and the three-quantum-number math of
csrc/eig_math.h (a host program under AddressSanitizer and UBSan) against the reference's own values
(tests/golden/eigfuncs3d.npz, written by tests/golden/make_golden_eigfuncs3d.py: 55 states of n <= 5 at charge 1.0 and
1.7 on 52 points with the origin, both halves of the z axis, the x and y axes, the z = 0 plane and every octant).

Function values: 1e-12 relative to each function's maximum over the points (the recurrence forms measure 2.6e-15
against scipy's genlaguerre and lpmv; the margin covers exp and lgamma differences), the bound of the 2-D tests.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import _eigfunc3d_oracle as EO3
from tests._golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def z():
    return load("eigfuncs3d")


def worst(got, want):
    """max over functions of max |got - want| / max |want| (per column)"""
    return float(np.max(np.max(np.abs(got - want), axis=0) / np.max(np.abs(want), axis=0)))


def spherical(x):
    x = np.asarray(x, dtype=np.float64)
    s = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2)
    return np.sqrt(s ** 2 + x[:, 2] ** 2), np.arctan2(s, x[:, 2]), np.arctan2(x[:, 1], x[:, 0])


def test_level_structure_matches_the_reference(z):
    from neural_svd_amd import eigfuncs as E, operators as O, _lib
    gt = O.Hydrogen3D(1.0)
    for n in (5, 14, 55):
        assert np.array_equal(np.asarray(gt.get_qnums(n)), z[f"qnums_{n}"]), n
        assert np.array_equal(gt.get_degeneracy(n), z[f"degeneracy_{n}"]), n
        assert np.array_equal(np.asarray(EO3.qnums(n)), z[f"qnums_{n}"]), n
        want = z[f"eigvals_{n}"]
        got = gt.get_eigvals(n)
        assert len(got) == len(want) and np.allclose(got, want, rtol=1e-14, atol=0), n
    assert list(gt.get_degeneracy(55)) == [0, 1, 5, 14, 30]  # the reference's eigenvalue list stops after n = 4
    # the table closes every level, ends on one, and stops at 80 functions
    t = E.ground_truth_table_3d(O.Hydrogen3D(1.7), 4)
    assert isinstance(t, E.GroundTruthTable3D) and t.ndim == 3
    assert (t.kind, t.param, t.Lg, t.degeneracy) == (_lib.GT_HYDROGEN3D, 1.7, 5, (0, 1, 5))
    assert _lib.GT_HYDROGEN3D not in (3, _lib.GT_HYDROGEN2D, _lib.GT_HARMONIC2D, _lib.GT_WELL2D)
    assert t.qnums == ((1, 0, 0), (2, 0, 0), (2, 1, -1), (2, 1, 0), (2, 1, 1))
    for L, Lg, deg in ((1, 1, (0, 1)), (5, 5, (0, 1, 5)), (6, 14, (0, 1, 5, 14)), (16, 30, (0, 1, 5, 14, 30)),
                       (55, 55, (0, 1, 5, 14, 30, 55))):
        t = E.ground_truth_table_3d(gt, L)
        assert (t.Lg, t.degeneracy) == (Lg, deg), L
        assert np.array_equal(np.asarray(t.qnums), z["qnums_55"][:Lg])
    for L in (56, 64, 91):
        with pytest.raises(E.NsvdError):
            E.ground_truth_table_3d(gt, L)  # the n = 6 shell ends at 91 > 80
    with pytest.raises(E.NsvdError):
        E.ground_truth_table_3d(O.Hydrogen2D(), 4)
    with pytest.raises(E.NsvdError):
        E.ground_truth_table(gt, 4)  # the 2-D builder keeps refusing it
    assert E.table_of(gt, 16).Lg == 30 and E.table_of(O.Hydrogen2D(), 16).ndim == 2 and E.table_of(t, 3) is t


def test_ground_truth_of_the_configuration():
    from types import SimpleNamespace
    from neural_svd_amd import operators as O
    gt = O.ground_truth_of(SimpleNamespace(problem="sch", ndim=3, potential_type="hydrogen", charge=1.5))
    assert isinstance(gt, O.Hydrogen3D) and gt.charge == 1.5
    assert isinstance(O.ground_truth_of(SimpleNamespace(problem="sch", ndim=2, potential_type="hydrogen", charge=1.0)),
                      O.Hydrogen2D)
    with pytest.raises(O.ProblemConfigError):
        O.ground_truth_of(SimpleNamespace(problem="sch", ndim=3, potential_type="harmonic_oscillator", charge=1.0))


def test_functions_match_the_reference(z):
    from neural_svd_amd import eigfuncs as E, operators as O
    x = z["x"]
    q = [tuple(int(v) for v in row) for row in z["qnums_55"]]
    r, th, phi = spherical(x)
    assert not x[0].any()  # the origin is row 0
    figures = {}
    for i, Z in enumerate(z["charges"]):
        want = z[f"psi_{i}"]
        gt = O.Hydrogen3D(float(Z))
        got = {"oracle": EO3.evaluate(Z, q, x),
               "operators": np.stack([gt.eigfunc(n, l, m, r, th, phi) for n, l, m in q], 1),
               "evaluate_host": E.evaluate_host(gt, q, x)}
        for name, g in got.items():
            assert g.shape == want.shape and np.isfinite(g).all(), (name, Z)
            figures[f"{name} Z={Z}"] = worst(g, want)
            for k, (n, l, m) in enumerate(q):  # the limit at the origin: finite for l = 0, exactly 0 otherwise
                assert (g[0, k] != 0.0) == (l == 0), (name, Z, n, l, m, g[0, k])
    print(figures)
    assert all(v < TOL for v in figures.values()), figures
    with pytest.raises(E.NsvdError):
        E.evaluate_host(O.Hydrogen3D(), q[:5], x[:, :2])


def test_limits_and_scaling():
    """psi_Z(x) = Z^(3/2) psi_1(Z x); l = 0 at the origin is sqrt((Z/n)^3 / (2n)) sqrt((n-1)! / n!) n / sqrt(4 pi)
    (L_{n-1}^(1)(0) = n); on the z axis every m != 0 vanishes; the far tail is 0 or tiny, never NaN"""
    q = EO3.qnums(55)
    g = np.random.default_rng(0)
    x = (3 * g.standard_normal((20, 3))).astype(np.float32)
    x2 = (2 * x).astype(np.float32)  # exact
    assert worst(EO3.evaluate(2.0, q, x), 2 ** 1.5 * EO3.evaluate(1.0, q, x2)) < 1e-14
    at0 = EO3.evaluate(1.7, q, np.zeros((1, 3), np.float32))[0]
    for (n, l, m), v in zip(q, at0):
        if l == 0:
            assert abs(v - np.sqrt((1.7 / n) ** 3 / (2 * n) / n) * n / np.sqrt(4 * np.pi)) < 1e-15
    axis = EO3.evaluate(1.0, q, np.array([[0, 0, 2.0], [0, 0, -3.0]], np.float32))
    scale = np.max(np.abs(EO3.evaluate(1.0, q, x)), axis=0)
    for k, (n, l, m) in enumerate(q):
        if m != 0:
            assert np.max(np.abs(axis[:, k])) < 1e-15 * scale[k], (n, l, m)
    far = EO3.evaluate(1.0, q, np.array([[3e4, -4e4, 1e3]], np.float32))
    assert np.isfinite(far).all() and np.max(np.abs(far)) < 1e-300


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """the three-quantum-number part of csrc/eig_math.h compiled for the CPU with its own main, under AddressSanitizer
    and UBSan"""
    exe = str(tmp_path_factory.mktemp("eigfuncs3d_host") / "eigfuncs3d_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "neural_svd_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_eigfuncs3d_host", "harness.cpp"), "-o", exe])
    return exe


def run_host(exe, kind, param, qnums, x):
    text = f"{kind} {param!r} {len(qnums)} {len(x)}\n"
    text += " ".join(f"{int(n)} {int(l)} {int(m)}" for n, l, m in qnums) + "\n"
    text += " ".join(f"{float(v):.9g}" for v in np.asarray(x, np.float32).reshape(-1)) + "\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    vals = p.stdout.split()
    rc = int(vals[0])
    return rc, np.array([float(v) for v in vals[1:]]).reshape(len(x), len(qnums)) if rc == 0 else None


def test_device_math_on_the_host(z, host_program):
    from neural_svd_amd import _lib
    kind = _lib.GT_HYDROGEN3D
    q = z["qnums_55"]
    x = z["x"]
    far = np.array([[3e4, -4e4, 1e3], [1e30, 1e30, -1e30], [3e38, 3e38, 3e38], [0, 0, -1e35]], np.float32)
    for i, Z in enumerate(z["charges"]):
        want = z[f"psi_{i}"]
        rc, got = run_host(host_program, kind, float(Z), q, np.concatenate([x, far]))
        assert rc == 0
        fig = worst(got[:len(x)], want)
        print(f"Z = {Z}: {fig:.3e}")
        assert np.isfinite(got).all() and fig < TOL
        for k, (n, l, m) in enumerate(q):
            assert (got[0, k] != 0.0) == (l == 0), (n, l, m)   # the origin
        assert not got[len(x):].any()                           # the tail: 0, never NaN
    # Z = 2 with the 80-function table the GPU tests use (the n = 6 shell, cut), against the oracle
    g = np.random.default_rng(3)
    xr = (4 * g.standard_normal((50, 3))).astype(np.float32)
    q80 = EO3.qnums(80)
    rc, got = run_host(host_program, kind, 2.0, q80, xr)
    assert rc == 0 and worst(got, EO3.evaluate(2.0, q80, xr)) < TOL
    # n = 16 is admitted (NSVD_EIG_MAX_Q) and finite
    rc, got = run_host(host_program, kind, 1.0, [(16, 15, -15), (16, 0, 0), (16, 15, 15)], xr)
    assert rc == 0 and np.isfinite(got).all()
    # refusals of the table: n = 0, n = 17, l = n, |m| = l + 1, l < 0, a 2-D kind, kind 3, a charge that is 0 or NaN
    origin = np.zeros((1, 3), np.float32)
    ok = [(1, 0, 0)]
    for k, param, qq in ((kind, 1.0, [(0, 0, 0)]), (kind, 1.0, [(17, 0, 0)]), (kind, 1.0, [(2, 2, 0)]),
                         (kind, 1.0, [(3, 1, 2)]), (kind, 1.0, [(3, 1, -2)]), (kind, 1.0, [(2, -1, 0)]),
                         (kind, 1.0, [(1, 0, 0), (2, 1, 0), (2, 1, 2)]),
                         (_lib.GT_HYDROGEN2D, 1.0, ok), (_lib.GT_HARMONIC2D, 1.0, ok), (_lib.GT_WELL2D, 1.0, ok),
                         (3, 1.0, ok), (-1, 1.0, ok), (kind, 0.0, ok), (kind, -1.0, ok), (kind, float("nan"), ok),
                         (kind, float("inf"), ok)):
        rc, _ = run_host(host_program, k, param, qq, origin)
        assert rc == _lib.EINVAL, (k, param, qq)
    assert run_host(host_program, kind, 1.0, ok, origin)[0] == 0
