"""The direction-loop epilogue of csrc/fd_math.h (nsvd_fd_row_nd + nsvd_fd_evenodd_nd: the finite-difference form of
5 <= D <= 12) compiled for the HOST (g++, float32, the same source file through the stand-in header
tests/_fd_math_nd_host/nsvd_common.h) and held to the reference's float64 run (tests/golden/highdim.npz) and to the
float64 restatement on the CPU. The head outputs at the stencil points come from the float64 oracle, rounded to float32
in the even / odd form and laid out (L, E B) as the generic path hands them to the kernel: this isolates the epilogue.

Bounds: the project's own, f 2e-5 and Tf 1e-4 in the relative Frobenius norm, per row group (test_periodic_gpu's
check_rows): the molecules' near-nucleus and near-coalescence rows and the box problems' wall rows each against their
own norm. Measured here (g++ 13, x86-64), worst group of each case, f / Tf:
    cos_5d 3.6e-8 / 9.5e-8, fp_10d 4.1e-8 / 9.1e-8, h2_2d 6.1e-8 / 1.1e-7, h2_3d 1.0e-7 / 1.3e-7, lih_3d 2.8e-7 / 4.3e-7,
    box D = 5 (sqrt and exp; Gaussian, uniform, no importance) at most 2.2e-7 / 1.4e-7
At D <= 4 the form agrees with nsvd_fd_evenodd (tests/_fd_math_host, untouched) on the periodic fixture's rows: the same
expressions with the reads in another order - f and Tf are asserted bit-identical, element by element."""
import ast
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _highdim_oracle as HO
from tests import _periodic_oracle as PO
from tests import test_highdim_oracle as THO
from tests import test_periodic_oracle as TPO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z():
    return np.load(THO.GOLDEN)


def _build(tmp_path_factory, sub, sym):
    td = str(tmp_path_factory.mktemp(sub))
    for src in (os.path.join(ROOT, "neural_svd_amd", "csrc", "fd_math.h"), os.path.join(ROOT, "include", "nsvd.h"),
                os.path.join(ROOT, "tests", sub, "nsvd_common.h"), os.path.join(ROOT, "tests", sub, "harness.cpp")):
        shutil.copy(src, td)
    out = os.path.join(td, "libfdhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=on", "-fPIC", "-shared",
                           os.path.join(td, "harness.cpp"), "-o", out])
    lib = C.CDLL(out)
    getattr(lib, sym)  # the symbol exists
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = _build(tmp_path_factory, "_fd_math_nd_host", "run_nd")
    lib.run_nd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                           C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 4
    lib.run_nd.restype = None
    return lib


@pytest.fixture(scope="module")
def old_lib(tmp_path_factory):
    return _build(tmp_path_factory, "_fd_math_host", "run")


def _f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def host_problem(prob, keep):
    """the nsvd_problem of `prob` with its table in HOST memory (`keep` holds the array alive)"""
    from neural_svd_amd import hip_ops as H
    mol = prob.potential == HO.POT_MOLECULE
    hp = H.make_problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                        prob.scale_kinetic, prob.hard_mul_const, importance_kind=prob.importance,
                        operator_kind=prob.operator_kind, fp_scale=prob.fp_scale,
                        pot_coef=prob.pot_coef if len(prob.pot_coef) <= 4 else (),
                        n_particles=getattr(prob, "n_particles", 1), n_nuclei=len(prob.nuclei) if mol else 0,
                        pot_const=prob.pot_const if mol else 0.0)
    tab = _f32(np.asarray(prob.nuclei).reshape(-1)) if mol else (_f32(prob.pot_coef) if prob.pot_coef else None)
    if tab is not None:
        keep.append(tab)
        hp.pot_table, hp.pot_table_len = tab.ctypes.data, tab.size
    return hp


def stencil_outputs(x, p, eps):
    """base at the centre and its even / odd parts along every direction, float64: (B, L), (B, L, D), (B, L, D)"""
    D = x.shape[1]
    bs = [O.mlp_forward(O.fourier_features(xe, p.fourier_B), p).numpy() for xe in O.stencil_points(x, eps)]
    b0 = bs[0]
    bE = np.stack([(bs[1 + 2 * d] + bs[2 + 2 * d]) / 2 - b0 for d in range(D)], -1)
    bO = np.stack([(bs[1 + 2 * d] - bs[2 + 2 * d]) / 2 for d in range(D)], -1)
    return b0, bE, bO


def kernel_layout(b0, bE, bO):
    """(L, E B) float32: row block 0 the centre, 1 + 2 d / 2 + 2 d the even / odd parts along d"""
    B, L, D = bE.shape
    base = np.zeros((L, (1 + 2 * D) * B), np.float32)
    base[:, :B] = b0.T
    for d in range(D):
        base[:, (1 + 2 * d) * B:(2 + 2 * d) * B] = bE[:, :, d].T
        base[:, (2 + 2 * d) * B:(3 + 2 * d) * B] = bO[:, :, d].T
    return base


def run_nd(lib, prob, p, x, L):
    keep = []
    hp = host_problem(prob, keep)
    B, D = x.shape
    has_mask = p.scales is not None
    sc = _f32(p.scales.numpy()) if has_mask else _f32(np.zeros(L))
    base = kernel_layout(*stencil_outputs(x, p, prob.eps))
    out = [np.full((B, L), np.nan, np.float32) for _ in range(4)]
    trig = int(prob.potential == PO.POT_COSINE or prob.operator_kind == PO.OP_FOKKER_PLANCK)
    xs = _f32(x.numpy())
    lib.run_nd(C.addressof(hp), D, B, L, int(has_mask), _ptr(sc), _ptr(xs), _ptr(base), base.shape[1],
               int(getattr(prob, "box_mode", 0)), float(getattr(prob, "box_lim", 0.0)), trig, *[_ptr(a) for a in out])
    return out


def check_groups(what, f, Tf, f64, Tf64, groups):
    for group, rows in groups:
        rows = np.asarray(rows)
        if not rows.any():
            continue
        ef, eT = rel(f[rows], f64[rows]), rel(Tf[rows], Tf64[rows])
        print(f"{what} {group} rows ({int(rows.sum())}): f {ef:.2e} Tf {eT:.2e}")
        assert ef < 2e-5, (what, group, ef)
        assert eT < 1e-4, (what, group, eT)
    assert np.isfinite(f).all() and np.isfinite(Tf).all()


@pytest.mark.parametrize("name", THO.CASES)
def test_host_epilogue_matches_reference(z, lib, name):
    cfg, names, p, prob = THO.case_setup(z, name)
    x = torch.tensor(z[f"{name}_x"][0], dtype=torch.float64)
    f, Tf, jac, dsc = run_nd(lib, prob, p, x, cfg["neigs"])
    groups = [(g, r.numpy()) for g, r in HO.row_groups(x, prob)]
    check_groups(name, f, Tf, z[f"{name}_f64_step0_f"], z[f"{name}_f64_step0_Tf"], groups)
    # jac = d f / d base(centre), dsc = d f / d scales: what the backward reads
    c = HO.operator_forward(x, p, prob)
    base0 = O.mlp_forward(O.fourier_features(x, p.fourier_B), p)
    assert rel(jac * base0.numpy(), c.f.numpy()) < 2e-5
    if p.scales is not None:
        r0 = x.norm(dim=1, keepdim=True)
        assert rel(dsc, (c.f * r0 / p.scales.view(1, -1) ** 2).numpy()) < 2e-5
    else:
        assert not dsc.any()


@pytest.mark.parametrize("imp", ["gaussian", "uniform", "none"])
@pytest.mark.parametrize("mode", ["sqrt", "exp"])
def test_host_epilogue_box_masks_5d(lib, mode, imp):
    """Dirichlet box masks at D = 5 with each density (and the exponential mask beside the Gaussian one), against the
    float64 restatement; rows at and beyond the wall are in the batch and measured as a group of their own"""
    D, L, B, lim = 5, 4, 64, 4.0
    kind = BO.BOX_SQRT if mode == "sqrt" else BO.BOX_EXP
    common = dict(eps=0.01, op_scale=1.0, op_shift=0.5, hard_mul_const=0.9, box_mode=kind, box_lim=lim)
    if imp == "gaussian":
        prob = HO.Problem(potential=O.POT_HARMONIC, charge_or_k=0.5, sigma=2.0, importance=HO.IMP_GAUSSIAN, **common)
    elif imp == "uniform":
        prob = HO.Problem(potential=BO.POT_ZERO, sigma=lim, importance=HO.IMP_UNIFORM, **common)
    else:
        prob = HO.Problem(potential=O.POT_HYDROGEN, charge_or_k=1.0, sigma=1.0, importance=HO.IMP_NONE, **common)
    p = O.init_params(L, D, 8, (16, 16), 0.2, exp_mask_init=4.0 if imp == "gaussian" else None, seed=21).to(torch.float64)
    g = torch.Generator().manual_seed(5)
    x = (lim * (2 * torch.rand(B, D, generator=g) - 1)).float()
    x[0, 0], x[1, 4], x[2, 2] = lim, -lim, lim + 0.5           # on the wall, and beyond it
    x[3, 1], x[4, 3] = lim - 0.005, -lim + 0.005                # the stencil straddles the wall
    x[5, 0], x[5, 4] = lim - 1e-3, -lim + 1e-3
    x = x.double()
    f, Tf, jac, dsc = run_nd(lib, prob, p, x, L)
    c = HO.operator_forward(x, p, prob)
    wall = BO.wall_rows(x, prob).numpy()
    assert wall.sum() >= 6
    check_groups(f"box_{mode}_{imp}", f, Tf, c.f.numpy(), c.Tf.numpy(), (("wall", wall), ("interior", ~wall)))
    outside = (x.abs() >= lim).any(dim=1).numpy()
    assert outside.sum() == 3 and not f[outside].any()


@pytest.mark.parametrize("name", ("cos_2d", "cos_1d", "fp_2d", "fp_2d_eps01", "fp_1d", "fp_2d_expmask", "h2p_2d", "hyd_3d"))
def test_direction_loop_agrees_with_the_small_form(lib, old_lib, name):
    """D <= 4: nsvd_fd_evenodd_nd against nsvd_fd_evenodd (the old harness) on the periodic fixture's rows"""
    zp = np.load(TPO.GOLDEN)
    cfg, names, p, prob = TPO.case_setup(zp, name)
    x = torch.tensor(zp[f"{name}_x"][0], dtype=torch.float64)
    B, D = x.shape
    L = cfg["neigs"]
    f, Tf, _, _ = run_nd(lib, prob, p, x, L)
    from neural_svd_amd import hip_ops as H
    hp = H.make_problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                        prob.scale_kinetic, prob.hard_mul_const, importance_kind=prob.importance,
                        operator_kind=prob.operator_kind, fp_scale=prob.fp_scale, pot_coef=prob.pot_coef)
    has_mask = p.scales is not None
    sc = _f32(p.scales.numpy()) if has_mask else _f32(np.zeros(L))
    b0, bE, bO = stencil_outputs(x, p, prob.eps)
    fo, To = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    args = [_f32(x.numpy()), _f32(b0), _f32(bE), _f32(bO), _f32(np.zeros((B, L, 1 + 2 * D)))]
    old_lib.run(C.byref(hp), D, B, L, int(has_mask), _ptr(sc), *[_ptr(a) for a in args], 0, _ptr(fo), _ptr(To))
    # the same expressions with the reads in another order: equal bits, element by element
    assert np.array_equal(f, fo) and np.array_equal(Tf, To), (name, int((f != fo).sum()), int((Tf != To).sum()))
