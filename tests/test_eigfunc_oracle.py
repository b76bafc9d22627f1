"""Eigenfunction accuracy on the host: the ground-truth interface of neural_svd_amd/operators.py (get_qnums,
get_degeneracy, eigfunc), the float64 oracle tests/_eigfunc_oracle.py and the per-function math of csrc/eig_math.h (a
host program under AddressSanitizer and UBSan) against the reference's own values (tests/golden/eigfuncs.npz, written by
tests/golden/make_golden_eigfuncs.py), and neural_svd_amd/eigfuncs.py's metrics against examples/linalg.py's.

Function values: 1e-12 relative to each function's maximum over the points (the recurrences measure 2e-15 against
scipy's hyp1f1; the margin covers exp and lgamma differences). Planted subspaces: every subspace distance and squared
angle below 1e-10 - the learned block is the ground truth rotated inside each level and rounded to float32, an error of
6e-8 that enters both quantities squared (the reference's subspace_distance gives about 1e-16 on this input, the level
Grams' condition numbers are at most 2.2); the planted rotation to 1e-6.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import _eigfunc_oracle as EO
from tests._golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def z():
    return load("eigfuncs")


def worst(got, want):
    """max over functions of max |got - want| / max |want| (per column)"""
    return float(np.max(np.max(np.abs(got - want), axis=0) / np.max(np.abs(want), axis=0)))


def test_level_structure_matches_the_reference(z):
    from neural_svd_amd import operators as O
    for tag, gt, sizes in (("hyd", O.Hydrogen2D(1.0), (5, 16, 64)), ("osc", O.HarmonicOscillator(1.0, 2), (4, 32, 66)),
                           ("well", O.InfiniteWell2D(10.0), (8,))):
        for n in sizes:
            assert np.array_equal(np.asarray(gt.get_qnums(n)), z[f"{tag}_qnums_{n}"]), (tag, n)
            assert np.array_equal(gt.get_degeneracy(n), z[f"{tag}_degeneracy_{n}"]), (tag, n)
            want = z[f"{tag}_eigvals_{n}"]
            got = gt.get_eigvals(n)[:len(want)]
            assert np.allclose(got, want, rtol=1e-14, atol=0), (tag, n)


def test_well_is_energy_ordered_with_accidental_degeneracies():
    from neural_svd_amd import operators as O
    w = O.InfiniteWell2D(2.0)
    q = w.get_qnums(40)
    e = [a * a + b * b for a, b in q]
    assert e == sorted(e) and q[8:10] == [(4, 1), (1, 4)] and q[10] == (3, 3)
    assert np.allclose(w.get_eigvals(40), np.array(e) * np.pi ** 2 / 4.0)
    # 50 = 5^2 + 5^2 = 7^2 + 1^2: one level of three states
    i = e.index(50)
    assert sorted(q[i:i + 3]) == [(1, 7), (5, 5), (7, 1)]
    deg = list(w.get_degeneracy(40))
    assert i in deg and i + 3 in deg and i + 1 not in deg and i + 2 not in deg


def test_functions_match_the_reference(z):
    from neural_svd_amd import operators as O
    x = z["x"].astype(np.float64)
    r, th = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2), np.arctan2(x[:, 1], x[:, 0])
    hyd, osc, well = O.Hydrogen2D(1.0), O.HarmonicOscillator(1.0, 2), O.InfiniteWell2D(2 * float(z["well_lim"]))
    qh, qo, qw = z["hyd_qnums_64"], z["osc_qnums_66"], z["well_qnums_8"]
    xw = z["well_x"].astype(np.float64)
    lim = float(z["well_lim"])
    figures = {
        "hyd oracle": worst(EO.evaluate(EO.HYDROGEN2D, 1.0, qh, z["x"]), z["hyd_psi"]),
        "hyd operators": worst(np.stack([hyd.eigfunc(n, l, r, th) for n, l in qh], 1), z["hyd_psi"]),
        "osc oracle": worst(EO.evaluate(EO.HARMONIC2D, 1.0, qo, z["x"]), z["osc_psi"]),
        "osc operators": worst(np.stack([osc.eigfunc(a, b, x[:, 0], x[:, 1]) for a, b in qo], 1), z["osc_psi"]),
        "well oracle": worst(EO.evaluate(EO.WELL2D, lim, qw, z["well_x"]), z["well_psi"]),
        "well operators": worst(np.stack([well.eigfunc(a, b, xw[:, 0] + lim, xw[:, 1] + lim) for a, b in qw], 1),
                                z["well_psi"]),
        "well operators box": worst(np.stack([well.eigfunc_box(a, b, xw[:, 0], xw[:, 1]) for a, b in qw], 1),
                                    z["well_psi"]),
    }
    print(figures)
    assert all(v < TOL for v in figures.values()), figures


def test_limits_and_parameters():
    """r = 0: the limit, not the reference's NaN; psi_Z(x) = Z psi_1(Z x); b = sqrt(k); 0 outside the box"""
    from neural_svd_amd import operators as O
    q = O.Hydrogen2D().get_qnums(16)
    at0 = EO.evaluate(EO.HYDROGEN2D, 1.0, q, np.zeros((1, 2), np.float32))[0]
    mirror = np.array([O.Hydrogen2D().eigfunc(n, l, np.zeros(1), np.zeros(1))[0] for n, l in q])
    assert np.isfinite(at0).all() and np.max(np.abs(at0 - mirror)) < 1e-15
    for (n, l), v in zip(q, at0):
        assert (v != 0.0) == (l == 0), (n, l, v)
        if l == 0:  # L_n^(0)(0) = 1: beta / sqrt(2n + 1) / sqrt(2 pi)
            assert abs(v - 1.0 / (n + 0.5) / np.sqrt(2 * n + 1) / np.sqrt(2 * np.pi)) < 1e-15
    g = np.random.default_rng(0)
    x = (3 * g.standard_normal((20, 2))).astype(np.float32)
    x2 = (2 * x).astype(np.float32)  # exact
    assert worst(EO.evaluate(EO.HYDROGEN2D, 2.0, q, x), 2 * EO.evaluate(EO.HYDROGEN2D, 1.0, q, x2)) < 1e-14
    qo = O.HarmonicOscillator().get_qnums(10)
    assert worst(EO.evaluate(EO.HARMONIC2D, 16.0, qo, x), 2 * EO.evaluate(EO.HARMONIC2D, 1.0, qo, x2)) < 1e-13
    xx = x.astype(np.float64)
    got = np.stack([O.HarmonicOscillator(k=16.0).eigfunc(a, b, xx[:, 0], xx[:, 1]) for a, b in qo], 1)
    assert worst(got, EO.evaluate(EO.HARMONIC2D, 16.0, qo, x)) < 1e-13
    out = np.array([[5.0001, 0.0], [0.0, -5.0001], [7.0, 7.0]], np.float32)
    assert not EO.evaluate(EO.WELL2D, 5.0, [(1, 1), (2, 3)], out).any()
    assert not O.InfiniteWell2D(10.0).eigfunc_box(1, 2, out[:, 0], out[:, 1]).any()


def test_ground_truth_table_ends_on_a_level():
    from neural_svd_amd import eigfuncs as E, operators as O, _lib
    t = E.ground_truth_table(O.Hydrogen2D(2.0), 16)
    assert (t.kind, t.param, t.Lg, t.degeneracy) == (_lib.GT_HYDROGEN2D, 2.0, 16, (0, 1, 4, 9, 16))
    assert E.ground_truth_table(O.Hydrogen2D(), 5).degeneracy == (0, 1, 4, 9)
    assert E.ground_truth_table(O.Hydrogen2D(), 64).Lg == 64
    assert E.ground_truth_table(O.HarmonicOscillator(), 32).Lg == 36
    t = E.ground_truth_table(O.HarmonicOscillator(4.0), 64)
    assert (t.kind, t.param, t.Lg, t.degeneracy[-2:]) == (_lib.GT_HARMONIC2D, 4.0, 66, (55, 66))
    t = E.ground_truth_table(O.InfiniteWell2D(10.0), 9)
    assert (t.kind, t.param, t.Lg, t.degeneracy) == (_lib.GT_WELL2D, 5.0, 10, (0, 1, 3, 4, 6, 8, 10))
    with pytest.raises(E.NsvdError):
        E.ground_truth_table(O.Hydrogen2D(), 70)   # the n = 8 shell ends at 81
    with pytest.raises(E.NsvdError):
        E.ground_truth_table(O.Hydrogen3D(), 4)


def small_matrices(Psi, Phi):
    n = len(Psi)
    return Psi.T @ Psi / n, Psi.T @ Phi / n, Phi.T @ Phi / n


def test_metrics_match_linalg(z):
    from neural_svd_amd.eigfuncs import eigenfunction_metrics
    for i in range(2):
        A, Ahat = z[f"lin{i}_A"], z[f"lin{i}_Ahat"]
        s, e = (int(v) for v in z[f"lin{i}_range"])
        deg = [0, e] if s == 0 else [0, s, e]
        m = eigenfunction_metrics(*small_matrices(A, Ahat), deg)
        lv = len(deg) - 2
        assert m["levels"][lv] == (s, e, e - s)
        assert abs(m["subspace_distance"][lv] - float(z[f"lin{i}_subspace_distance"])) < 1e-12
        cosv = np.linalg.norm(z[f"lin{i}_rotate"], axis=0) / np.linalg.norm(A[:, s:e], axis=0)
        assert np.max(np.abs(m["angle"][s:e] - np.arccos(cosv))) < 1e-10
        An, Ahn = A[:, s:e] @ EO._inv_sqrt(A[:, s:e].T @ A[:, s:e]), Ahat[:, s:e] @ EO._inv_sqrt(Ahat[:, s:e].T @ Ahat[:, s:e])
        P = z[f"lin{i}_procrustes"]
        assert np.max(np.abs(m["rotation"][lv] - Ahn.T @ P)) < 1e-10
        assert abs(m["procrustes_residual"][lv] - np.linalg.norm(P - An) ** 2 / (e - s)) < 1e-10
        # and the oracle's block form says the same
        o = EO.metrics(A, Ahat, deg)
        assert np.max(np.abs(o["subspace_distance"] - m["subspace_distance"])) < 1e-12
        assert np.max(np.abs(o["angle"] - m["angle"])) < 1e-10
        assert np.max(np.abs(o["gram_defect"] - m["gram_defect"])) < 1e-12


@pytest.fixture(scope="module")
def planted():
    """300 points x = 8 N(0, I) float32, hydrogen's first 16 functions, and a learned block = the ground truth rotated by
    a random orthogonal matrix inside each level and scaled per level, rounded to float32"""
    g = np.random.default_rng(5)
    x = (8 * g.standard_normal((300, 2))).astype(np.float32)
    from neural_svd_amd.operators import Hydrogen2D
    q = Hydrogen2D().get_qnums(16)
    Psi = EO.evaluate(EO.HYDROGEN2D, 1.0, q, x)
    deg = [0, 1, 4, 9, 16]
    rots, Phi = [], np.empty_like(Psi)
    for lv, (s, e) in enumerate(zip(deg[:-1], deg[1:])):
        R, _ = np.linalg.qr(g.standard_normal((e - s, e - s)))
        rots.append(R)
        Phi[:, s:e] = (0.5 + lv) * Psi[:, s:e] @ R
    return Psi, Phi.astype(np.float32).astype(np.float64), deg, rots


def test_planted_rotation_is_recovered(planted):
    from neural_svd_amd.eigfuncs import eigenfunction_metrics
    Psi, Phi, deg, rots = planted
    assert max(np.linalg.cond(Psi[:, s:e].T @ Psi[:, s:e]) for s, e in zip(deg[:-1], deg[1:])) < 2.5
    m = eigenfunction_metrics(*small_matrices(Psi, Phi), deg)
    print(m["subspace_distance"], np.nanmax(m["angle"] ** 2))
    assert m["levels"] == [(0, 1, 1), (1, 4, 3), (4, 9, 5), (9, 16, 7)]
    assert np.all(np.abs(m["subspace_distance"]) < 1e-10)
    assert np.all(m["angle"] ** 2 < 1e-10)
    assert np.all(np.abs(m["procrustes_residual"]) < 1e-10)
    for Q, R in zip(m["rotation"], rots):
        assert np.max(np.abs(Q - R.T)) < 1e-6  # Phi_hat = Psi_hat R, so Phi_hat Q = Psi_hat at Q = R^T
    # a permutation of the learned columns with `order` undoing it: the same numbers
    perm = np.random.default_rng(6).permutation(16)
    gram, cross, cov = small_matrices(Psi, Phi[:, perm])
    m2 = eigenfunction_metrics(gram, cross, cov, deg, order=np.argsort(perm))
    assert np.allclose(m2["subspace_distance"], m["subspace_distance"], atol=1e-13)
    assert np.allclose(m2["angle"] ** 2, m["angle"] ** 2, atol=1e-12)


def test_mixed_levels_equal_the_reference_formula(planted):
    """psi_1 (level 1) and psi_4 (level 2) mixed by cos a, sin a: the distance is the reference's formula on the same
    blocks - not sin^2 a, the sample Gram is not the identity"""
    from neural_svd_amd.eigfuncs import eigenfunction_metrics
    Psi, _, deg, _ = planted
    a = 0.3
    Phi = Psi.copy()
    Phi[:, 1] = np.cos(a) * Psi[:, 1] + np.sin(a) * Psi[:, 4]
    Phi[:, 4] = -np.sin(a) * Psi[:, 1] + np.cos(a) * Psi[:, 4]
    m = eigenfunction_metrics(*small_matrices(Psi, Phi), deg)
    want = [EO.subspace_distance(Psi[:, s:e], Phi[:, s:e]) for s, e in zip(deg[:-1], deg[1:])]
    print(m["subspace_distance"], want, np.sin(a) ** 2 / 3)
    assert np.max(np.abs(m["subspace_distance"] - np.array(want))) < 1e-12
    assert abs(m["subspace_distance"][0]) < 1e-12 and abs(m["subspace_distance"][3]) < 1e-12
    assert m["subspace_distance"][1] > 1e-3 and m["subspace_distance"][2] > 1e-3
    assert abs(m["subspace_distance"][1] - np.sin(a) ** 2 / 3) > 1e-6
    o = EO.metrics(Psi, Phi, deg)
    # (arccos near 1 turns a rounding of 1e-16 into an angle of 1e-8: angles are compared squared)
    assert np.max(np.abs(o["angle"] ** 2 - m["angle"] ** 2)) < 1e-12
    assert np.max(np.abs(np.array(o["procrustes_residual"]) - m["procrustes_residual"])) < 1e-10


def test_partial_last_level():
    """oscillator, L = 4 learned functions, Lg = 6: the n = 2 shell has three states and one learned column"""
    from neural_svd_amd import eigfuncs as E, operators as O
    t = E.ground_truth_table(O.HarmonicOscillator(), 4)
    assert t.Lg == 6 and t.degeneracy == (0, 1, 3, 6)
    g = np.random.default_rng(8)
    x = (1.5 * g.standard_normal((300, 2))).astype(np.float32)
    Psi = EO.evaluate(EO.HARMONIC2D, 1.0, t.qnums, x)
    Phi = np.empty((300, 4))
    Phi[:, 0] = 2 * Psi[:, 0]
    Phi[:, 1:3] = Psi[:, 1:3] @ np.array([[0.6, -0.8], [0.8, 0.6]])
    Phi[:, 3] = Psi[:, 3:6] @ np.array([0.5, -0.5, 0.7])  # inside the level's span
    m = E.eigenfunction_metrics(*small_matrices(Psi, Phi), t.degeneracy)
    assert m["levels"] == [(0, 1, 1), (1, 3, 2), (3, 6, 1)]
    assert np.all(np.abs(m["subspace_distance"]) < 1e-12)
    assert m["rotation"][2] is None and np.isnan(m["procrustes_residual"][2]) and np.isnan(m["angle"][3:]).all()
    assert np.all(m["angle"][:3] < 1e-6)
    # the learned column leaks out of the level: against the reference's formula on the blocks
    Phi[:, 3] += 0.3 * Psi[:, 1]
    m = E.eigenfunction_metrics(*small_matrices(Psi, Phi), t.degeneracy)
    want = EO.subspace_distance(Psi[:, 3:6], Phi[:, 3:4])
    assert want > 1e-3 and abs(m["subspace_distance"][2] - want) < 1e-12
    o = EO.metrics(Psi, Phi, t.degeneracy)
    assert np.max(np.abs(o["subspace_distance"] - m["subspace_distance"])) < 1e-12


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/eig_math.h compiled for the CPU with its own main, under AddressSanitizer and UBSan"""
    exe = str(tmp_path_factory.mktemp("eigfuncs_host") / "eigfuncs_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "neural_svd_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_eigfuncs_host", "harness.cpp"), "-o", exe])
    return exe


def run_host(exe, kind, param, qnums, x):
    text = f"{kind} {param!r} {len(qnums)} {len(x)}\n"
    text += " ".join(f"{int(a)} {int(b)}" for a, b in qnums) + "\n"
    text += " ".join(f"{float(v):.9g}" for v in np.asarray(x, np.float32).reshape(-1)) + "\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    vals = p.stdout.split()
    rc = int(vals[0])
    return rc, np.array([float(v) for v in vals[1:]]).reshape(len(x), len(qnums)) if rc == 0 else None


def test_device_math_on_the_host(z, host_program):
    from neural_svd_amd import _lib
    origin = np.zeros((1, 2), np.float32)
    far = np.array([[3e4, -4e4], [1e30, 1e30], [3e38, 3e38]], np.float32)  # the tail: 0, never NaN
    for kind, param, q, x, want in ((_lib.GT_HYDROGEN2D, 1.0, z["hyd_qnums_64"], z["x"], z["hyd_psi"]),
                                    (_lib.GT_HARMONIC2D, 1.0, z["osc_qnums_66"], z["x"], z["osc_psi"]),
                                    (_lib.GT_WELL2D, float(z["well_lim"]), z["well_qnums_8"], z["well_x"], z["well_psi"])):
        rc, got = run_host(host_program, kind, param, q, np.concatenate([x, origin, far]))
        assert rc == 0
        fig = worst(got[:len(x)], want)
        print(kind, fig)
        assert fig < TOL
        at0 = EO.evaluate(kind, param, q, origin)
        assert np.max(np.abs(got[len(x)] - at0[0])) <= 1e-15 * np.max(np.abs(want))
        assert not got[len(x) + 1:].any()
    # Z = 2, k = 4, lim = 5 with the tables the GPU tests use, against the oracle
    from neural_svd_amd import eigfuncs as E, operators as O
    g = np.random.default_rng(3)
    x = (4 * g.standard_normal((50, 2))).astype(np.float32)
    for gt, L in ((O.Hydrogen2D(2.0), 64), (O.HarmonicOscillator(4.0), 64), (O.InfiniteWell2D(10.0), 9)):
        t = E.ground_truth_table(gt, L)
        rc, got = run_host(host_program, t.kind, t.param, t.qnums, x)
        want = EO.evaluate(t.kind, t.param, t.qnums, x)
        assert rc == 0 and worst(got, want) < TOL
    # refusals of the table: hydrogen |l| > n, well nx = 0, an unknown kind, a parameter that is not positive
    for kind, param, q in ((_lib.GT_HYDROGEN2D, 1.0, [(1, 2)]), (_lib.GT_HYDROGEN2D, 1.0, [(17, 0)]),
                           (_lib.GT_WELL2D, 5.0, [(0, 1)]), (_lib.GT_HARMONIC2D, 1.0, [(-1, 0)]), (3, 1.0, [(1, 1)]),
                           (_lib.GT_HARMONIC2D, 0.0, [(1, 1)]), (_lib.GT_WELL2D, float("nan"), [(1, 1)])):
        rc, _ = run_host(host_program, kind, param, q, origin)
        assert rc == _lib.EINVAL, (kind, param, q)
