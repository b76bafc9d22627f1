"""The epilogue arithmetic of csrc/fd_math.h - potentials of the coordinates, the Fokker-Planck branch in both
finite-difference forms, the exact-Laplacian product rule - compiled for the HOST (g++, float32, the same source file
through the stand-in header tests/_fd_math_host/nsvd_common.h) and held to the reference's float64 run
(tests/golden/periodic.npz) on the CPU. The head outputs at the stencil points come from the float64 oracle, rounded to
float32 in the even / odd form the kernels hand to the epilogue: this isolates the epilogue (the MLP before it is
covered on the GPU). Bounds: the project's f 2e-5, Tf 1e-4 (exact mode 2e-5) for the even / odd and exact forms. The
point-wise form is the reference's own float32 arithmetic and carries its stencil noise: 2 D + 1 values g_e, each
rounded to float32, are summed and divided by eps^2, so |Tf - Tf64| <= scale (4 D + 2) 2^-23 max_e |g_e| / (eps^2 sqrt p)
+ 1e-4 |Tf64| per entry, with max_e |g_e| / sqrt p taken as 2 |f64| (neighbouring points within eps)."""
import ast
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _periodic_oracle as PO
from tests.test_periodic_oracle import CASES, GOLDEN, case_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    td = str(tmp_path_factory.mktemp("fd_math_host"))
    for src in (os.path.join(ROOT, "neural_svd_amd", "csrc", "fd_math.h"), os.path.join(ROOT, "include", "nsvd.h"),
                os.path.join(ROOT, "tests", "_fd_math_host", "nsvd_common.h"),
                os.path.join(ROOT, "tests", "_fd_math_host", "harness.cpp")):
        shutil.copy(src, td)
    out = os.path.join(td, "libfdhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=on", "-fPIC", "-shared",
                           os.path.join(td, "harness.cpp"), "-o", out])
    return C.CDLL(out)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name", CASES)
def test_host_epilogue_matches_reference(z, lib, name):
    from neural_svd_amd import hip_ops as H
    cfg, names, p, prob = case_setup(z, name)
    x = torch.tensor(z[f"{name}_x"][0], dtype=torch.float64)
    B, D = x.shape
    L = cfg["neigs"]
    hp = H.make_problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                        prob.scale_kinetic, prob.hard_mul_const, importance_kind=prob.importance,
                        operator_kind=prob.operator_kind, fp_scale=prob.fp_scale, pot_coef=prob.pot_coef)
    has_mask = p.scales is not None
    sc = _f32(p.scales.numpy()) if has_mask else _f32(np.zeros(L))
    f, Tf = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    f64, Tf64 = z[f"{name}_f64_step0_f"], z[f"{name}_f64_step0_Tf"]
    groups = [np.ones(B, dtype=bool)]
    if prob.potential == PO.POT_H2_ION:  # near-nucleus rows and the others, each against its own norm
        near = PO.nucleus_rows(x, prob).numpy()
        groups = [near, ~near]

    def base(xe):
        return O.mlp_forward(O.fourier_features(xe, p.fourier_B), p)

    if prob.eps > 0:
        bs = [base(xe).numpy() for xe in O.stencil_points(x, prob.eps)]
        b0 = bs[0]
        bE = np.stack([(bs[1 + 2 * d] + bs[2 + 2 * d]) / 2 - b0 for d in range(D)], -1)
        bO = np.stack([(bs[1 + 2 * d] - bs[2 + 2 * d]) / 2 for d in range(D)], -1)
        bv = np.stack(bs, -1)
        args = [_f32(x.numpy()), _f32(b0), _f32(bE), _f32(bO), _f32(bv)]
        for mode in (0, 1):
            lib.run(C.byref(hp), D, B, L, int(has_mask), _ptr(sc), *[_ptr(a) for a in args], mode, _ptr(f), _ptr(Tf))
            for rows in groups:
                assert rel(f[rows], f64[rows]) < 2e-5
                if mode == 0:
                    assert rel(Tf[rows], Tf64[rows]) < 1e-4, (name, rel(Tf[rows], Tf64[rows]))
            if mode == 1:
                scale = abs(prob.op_scale) * (abs(prob.fp_scale) if prob.operator_kind else prob.scale_kinetic)
                eps = float(np.float32(prob.eps))
                tol = scale * (4 * D + 2) * 2.0 ** -23 * 2 * np.abs(f64) / eps ** 2 + 1e-4 * np.abs(Tf64)
                assert np.all(np.abs(Tf - Tf64) <= tol), (name, float(np.max(np.abs(Tf - Tf64) / tol)))
        return
    xr = x.clone().requires_grad_(True)
    b = base(xr)
    db, lb = np.zeros((B, L, D)), np.zeros((B, L))
    for l in range(L):
        (g,) = torch.autograd.grad(b[:, l].sum(), xr, create_graph=True)
        db[:, l, :] = g.detach().numpy()
        for d in range(D):
            lb[:, l] += torch.autograd.grad(g[:, d].sum(), xr, retain_graph=True)[0][:, d].numpy()
    lib.run_exact(C.byref(hp), D, B, L, int(has_mask), _ptr(sc), _ptr(_f32(x.numpy())), _ptr(_f32(b.detach().numpy())),
                  _ptr(_f32(db)), _ptr(_f32(lb)), _ptr(f), _ptr(Tf))
    for rows in groups:
        assert rel(f[rows], f64[rows]) < 2e-5
        assert rel(Tf[rows], Tf64[rows]) < 2e-5, (name, rel(Tf[rows], Tf64[rows]))
