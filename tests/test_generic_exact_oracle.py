"""NSVD_PATH_GENERIC_EXACT on the CPU: the host-side path names, get_problem / get_evd_method under the opt-in switch,
the float64 oracle of the exact mode (tests/_exact_nd_oracle.py) against the reference's own exact mode above four input
dimensions (tests/golden/exact_nd.npz, made by tests/golden/make_golden_exact_nd.py), and the epilogue's product rule
(csrc/fd_math.h: nsvd_fd_exact up to D = 4, nsvd_fd_exact_nd above) compiled for the HOST (g++, float32, the same
source through the stand-in header tests/_fd_exact_host/nsvd_common.h) against float64 double autograd of
c sqrt p(x) mask(x) box(x) u(x) for an analytic u.

Bound of the host epilogue: 1e-5 relative (Frobenius norm over all rows) on f, Tf, jac and dsc; the inputs keep 0.1
from every wall, nucleus, coalescence point and the origin by construction, which the test asserts; no row is left out.
Measured here (g++ 13, x86-64), worst case of each output: f 5.5e-7, Tf 5.1e-7, jac 5.2e-7, dsc 4.5e-7 (all at D = 12
with the Gaussian density, whose sqrt p goes through one float32 exp of an argument near -20; 2e-7 and below at D = 4
and 5)."""
import argparse
import ast
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _exact_nd_oracle as XO
from tests import _highdim_oracle as HO
from tests import test_highdim_host_epilogue as THE
from tests import test_highdim_oracle as THO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exact_nd.npz")
GOLDEN_CASES = ("cos_5d", "h2_3d")
FAKE_TABLE = 256  # a non-null address: the host-side queries look at the pointer's presence only
rel = THO.rel


# ---------------------------------------------------------------------------- 1. host-side queries
def test_constant_and_path_names():
    from neural_svd_amd import _lib
    from neural_svd_amd import hip_ops as H
    assert H.PATH_GENERIC_EXACT == _lib.PATH_GENERIC_EXACT == 4
    hdr = open(os.path.join(ROOT, "include", "nsvd.h")).read()
    assert "#define NSVD_PATH_GENERIC_EXACT 4" in hdr and "#define NSVD_ABI_VERSION 6" in hdr
    PI = float(np.pi)
    X = H.PATH_GENERIC_EXACT

    def shape(D, hidden=(16, 16), m=8, **kw):
        return H.ModelShape(L=4, D=D, m=m, hidden=hidden, **kw)

    def name(D, pot, table_len=None, eps=0.0, imp=H.IMP_UNIFORM, path=X, sh=None, **kw):
        prob = H.make_problem(pot, 1.0, eps, 1.0, 0.0, PI, importance_kind=imp, **kw)
        if table_len is not None:
            prob.pot_table, prob.pot_table_len = FAKE_TABLE, table_len
        return H.path_name(sh or shape(D), 64, path, prob)

    mol = dict(imp=H.IMP_GAUSSIAN, scale_kinetic=0.5)
    fp = dict(operator_kind=H.OP_FOKKER_PLANCK, fp_scale=1.0)
    for D in (1, 4, 5, 12):
        cos = dict(table_len=D) if D > 4 else dict(pot_coef=(0.5,) * D)
        for eps in (0.0, -1.0):
            assert name(D, H.POT_COSINE, eps=eps, **cos) == "generic_exact"
            assert name(D, H.POT_HYDROGEN, eps=eps, imp=H.IMP_GAUSSIAN) == "generic_exact"
            assert name(D, H.POT_HARMONIC, eps=eps, imp=H.IMP_NONE, sh=shape(D, (50,), 33, has_exp_mask=True)) \
                == "generic_exact"
        # any model validate() accepts: 1 .. 8 layers, any width (128 too: the path is explicit), box masks
        assert name(D, H.POT_ZERO, sh=shape(D, (128, 128, 128), 64, box_mask=H.BOX_SQRT, box_lim=PI)) == "generic_exact"
        assert name(D, H.POT_ZERO, sh=shape(D, (8,) * 7, 4, box_mask=H.BOX_EXP, box_lim=PI)) == "generic_exact"
        assert name(D, H.POT_ZERO, sh=shape(D, (), 4)) == "generic_exact"
        # eps > 0 cannot be honoured on this path; Fokker-Planck has no exact mode
        assert name(D, H.POT_COSINE, eps=0.01, **cos) == "unsupported"
        assert name(D, H.POT_HYDROGEN, eps=1e-5, imp=H.IMP_GAUSSIAN) == "unsupported"
        assert name(D, H.POT_SIN_OF_COS, **dict(cos, **fp)) == "unsupported"
        assert name(D, H.POT_SIN_OF_COS, eps=0.01, **dict(cos, **fp)) == "unsupported"
    assert name(4, H.POT_MOLECULE, 6, n_particles=2, n_nuclei=2, **mol) == "generic_exact"     # H2 in 2-D
    assert name(6, H.POT_MOLECULE, 8, n_particles=2, n_nuclei=2, **mol) == "generic_exact"     # H2 in 3-D
    assert name(12, H.POT_MOLECULE, 8, n_particles=4, n_nuclei=2, **mol) == "generic_exact"    # LiH in 3-D
    assert name(6, H.POT_MOLECULE, 8, n_particles=2, n_nuclei=2, eps=0.01, **mol) == "unsupported"
    assert name(13, H.POT_HYDROGEN) == "unsupported" and name(13, H.POT_COSINE, 13) == "unsupported"
    assert name(15, H.POT_MOLECULE, 4, n_particles=5, n_nuclei=1, **mol) == "unsupported"
    # "invalid" stays "invalid"
    assert name(5, H.POT_COSINE) == "invalid" and name(6, H.POT_MOLECULE, 6, n_particles=2, n_nuclei=2, **mol) == "invalid"
    assert name(2, H.POT_SIN_OF_COS, pot_coef=(1.0, 1.0)) == "invalid"  # (outside the Fokker-Planck kind)
    # without a problem the name of the explicit request
    assert H.path_name(shape(5), 64, X) == "generic_exact"
    # the old path values answer as before: the exact mode has no path off the MFMA kernels, and none above 4 dimensions
    for path in (H.PATH_AUTO, H.PATH_GENERIC):
        assert name(2, H.POT_HYDROGEN, imp=H.IMP_GAUSSIAN, path=path) == "unsupported"
        assert name(5, H.POT_COSINE, 5, path=path) == "unsupported"
        assert name(6, H.POT_MOLECULE, 8, n_particles=2, n_nuclei=2, path=path, **mol) == "unsupported"
        assert name(5, H.POT_COSINE, 5, eps=0.01, path=path) == "generic"
        assert name(2, H.POT_HYDROGEN, eps=0.01, imp=H.IMP_GAUSSIAN, path=path) == "generic"
    wide = shape(2, (128, 128, 128), 64)
    assert name(2, H.POT_HYDROGEN, imp=H.IMP_GAUSSIAN, path=H.PATH_AUTO, sh=wide) == "fused_mfma"
    assert name(2, H.POT_HYDROGEN, imp=H.IMP_GAUSSIAN, path=H.PATH_FUSED, sh=wide) == "fused_mfma"
    assert name(2, H.POT_HYDROGEN, imp=H.IMP_GAUSSIAN, path=H.PATH_GENERIC, sh=wide) == "unsupported"
    assert name(2, H.POT_HYDROGEN, imp=H.IMP_GAUSSIAN, path=H.PATH_FUSED) == "unsupported"
    assert name(5, H.POT_COSINE, 5, path=H.PATH_FUSED, sh=shape(5, (128, 128), 64)) == "unsupported"
    assert name(5, H.POT_COSINE, 5, eps=0.01, path=H.PATH_FUSED, sh=shape(5, (128, 128), 64)) == "fused_mfma"
    assert H.path_name(wide, 64, H.PATH_AUTO) == "fused_mfma" and H.path_name(shape(5), 64, H.PATH_GENERIC) == "generic"
    # D + 2 jet blocks fit the workspace of the 1 + 2 D stencil blocks: its size is unchanged by the new path
    assert H.workspace_bytes(shape(12), 64) > H.workspace_bytes(shape(4), 64) > 0


def _args(cfg, **over):
    a = argparse.Namespace(**dict(cfg, **over))
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    return a


def test_get_problem_and_method_under_the_switch():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.nested_lowrank import get_evd_method
    from neural_svd_amd.operators import ProblemConfigError, get_problem
    zh = np.load(THO.GOLDEN)
    cos = ast.literal_eval(str(zh["cos_5d_cfg"]))
    fp = ast.literal_eval(str(zh["fp_10d_cfg"]))
    mol = ast.literal_eval(str(zh["h2_3d_cfg"]))
    for nd in (5, 10):
        a = _args(cos, ndim=nd, high_dim_stencil=True, laplacian_eps=0.0, generic_exact_laplacian=True)
        op, gt = get_problem(a)
        assert op.operator.laplacian_eps == 0.0 and len(op.operator.potential_coef) == nd
        assert get_evd_method(a, "neuralsvd", None).path == H.PATH_GENERIC_EXACT
        # without the switch (absent or false) the refusal stands
        for over in (dict(), dict(generic_exact_laplacian=False)):
            with pytest.raises(ProblemConfigError, match="laplacian_eps"):
                get_problem(_args(cos, ndim=nd, high_dim_stencil=True, laplacian_eps=0.0, **over))
        # the switch does not replace high_dim_stencil, and gives Fokker-Planck no exact mode
        with pytest.raises(NotImplementedError, match="at most 4 input dimensions"):
            get_problem(_args(cos, ndim=nd, laplacian_eps=0.0, generic_exact_laplacian=True))
        with pytest.raises(AssertionError, match="laplacian_eps"):
            get_problem(_args(fp, ndim=nd, high_dim_stencil=True, laplacian_eps=0.0, generic_exact_laplacian=True))
    a = _args(mol, high_dim_stencil=True, laplacian_eps=0.0, generic_exact_laplacian=True)
    op, _ = get_problem(a)
    assert a.n_particles == 2 and op.operator.laplacian_eps == 0.0 and op.operator.scale_kinetic == 0.5
    with pytest.raises(AssertionError, match="laplacian_eps"):
        get_problem(_args(mol, high_dim_stencil=True, laplacian_eps=0.0))
    with pytest.raises(ProblemConfigError, match="at most 12"):
        get_problem(_args(mol, mol_name="B", high_dim_stencil=True, laplacian_eps=0.0, generic_exact_laplacian=True))
    # the method: PATH_GENERIC_EXACT only with the switch AND eps <= 0; PATH_AUTO otherwise, as before
    assert get_evd_method(_args(cos, generic_exact_laplacian=True), "neuralsvd", None).path == H.PATH_AUTO
    assert get_evd_method(_args(cos, laplacian_eps=0.0), "neuralsvd", None).path == H.PATH_AUTO
    assert get_evd_method(_args(cos), "neuralsvd", None).path == H.PATH_AUTO


# ---------------------------------------------------------------------------- 2. the oracle against the reference
@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def test_golden_is_small_and_holds_no_source(z):
    assert os.path.getsize(GOLDEN) < 512 * 1024
    for k in z.files:
        assert z[k].dtype.kind in "fiU", (k, z[k].dtype)  # numbers, and the cfg / name strings
    for name in GOLDEN_CASES:
        cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
        assert cfg["laplacian_eps"] == 0.0 and cfg["neigs"] == 3 and cfg["batch_size"] == 8
        assert cfg["mlp_hidden_dims"] == "16,16" and cfg["fourier_mapping_size"] == 8


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_oracle_matches_reference_exact_mode(z, name):
    """double autograd of the float64 restatement against the reference's exact mode: 1e-9, as the stencil mode's pin"""
    cfg, names, p, prob = THO.case_setup(z, name)
    assert prob.eps == 0.0 and p.fourier_B.shape[0] == dict(cos_5d=5, h2_3d=6)[name]
    x = torch.tensor(z[f"{name}_x"][0], dtype=torch.float64)
    assert float(XO.clearance(x, p.scales, prob).min()) > 0.1
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    r = XO.loss_and_grads(x, p, prob, v, M)
    pre = f"{name}_f64_step0_"
    scale = float((r["f"] * r["Tf"]).abs().sum()) / x.shape[0]
    assert abs(float(r["loss"]) - float(z[pre + "loss"])) < 1e-9 * scale
    assert rel(r["f"], z[pre + "f"]) < 1e-9
    assert rel(r["Tf"], z[pre + "Tf"]) < 1e-9
    for n, g in zip(names, r["grads"]):
        assert rel(g, z[pre + f"grad_{n}"]) < 1e-9, n
    # the float32 run of the reference is the yardstick of the GPU test: present, finite, close
    assert rel(z[f"{name}_f32_step0_Tf"], z[pre + "Tf"]) < 1e-3


def test_oracle_jets_are_the_closed_form():
    """the jet helpers the GPU kernel tests compare against, held to autograd and to oracle.nsvd_oracle.exact_jets"""
    g = torch.Generator().manual_seed(3)
    B, D, m = 5, 3, 4
    x = torch.randn(B, D, generator=g, dtype=torch.float64).requires_grad_(True)
    fB = torch.randn(D, m, generator=g, dtype=torch.float64)
    J = XO.fourier_jets(x.detach(), fB)
    phi = O.fourier_features(x, fB)  # (B, 2m)
    for k in range(2 * m):
        (gr,) = torch.autograd.grad(phi[:, k].sum(), x, create_graph=True)
        lap = sum(torch.autograd.grad(gr[:, d].sum(), x, retain_graph=True)[0][:, d] for d in range(D))
        assert rel(J[k, :B], phi[:, k].detach()) < 1e-14
        for d in range(D):
            assert rel(J[k, (1 + d) * B:(2 + d) * B], gr[:, d].detach()) < 1e-13
        assert rel(J[k, (D + 1) * B:], lap) < 1e-13
    # softplus of a function of x: z = phi W (one row), through the jets and through autograd
    W = torch.randn(2 * m, generator=g, dtype=torch.float64) * 8  # (pre-activations on both sides of the threshold)
    zj = (W.view(1, -1) @ J)
    out = XO.softplus_jets(zj, B, D)
    a = O.softplus(phi @ W)
    (gr,) = torch.autograd.grad(a.sum(), x, create_graph=True)
    lap = sum(torch.autograd.grad(gr[:, d].sum(), x, retain_graph=True)[0][:, d] for d in range(D))
    assert rel(out[0, :B], a.detach()) < 1e-14
    for d in range(D):
        assert rel(out[0, (1 + d) * B:(2 + d) * B], gr[:, d].detach()) < 1e-12
    assert rel(out[0, (D + 1) * B:], lap) < 1e-12


# ---------------------------------------------------------------------------- 3. the epilogue's arithmetic on the host
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    td = str(tmp_path_factory.mktemp("fd_exact_host"))
    for src in (os.path.join(ROOT, "neural_svd_amd", "csrc", "fd_math.h"), os.path.join(ROOT, "include", "nsvd.h"),
                os.path.join(ROOT, "tests", "_fd_exact_host", "nsvd_common.h"),
                os.path.join(ROOT, "tests", "_fd_exact_host", "harness.cpp")):
        shutil.copy(src, td)
    out = os.path.join(td, "libfdexact.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=on", "-fPIC", "-shared",
                           os.path.join(td, "harness.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.run_exact.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                              C.c_int, C.c_float] + [C.c_void_p] * 4
    lib.run_exact.restype = None
    return lib


def _molecule(name, ndim):
    cfg = dict(problem="sch", potential_type="quantum_chemistry", mol_name=name, ndim=ndim, laplacian_eps=0.0,
               operator_scale=1.0, operator_shift=0.0, sampling_scale=2.0, hard_mul_const=1.0, sampling_mode="gaussian")
    return HO.problem_of(cfg)


def _host_cases():
    """(id, D, problem, exponential mask scale or None): D = 4 (nsvd_fd_exact), 5 and 12 (the direction loop); the three
    densities, the exponential mask on and off, both box modes and none, the four potentials"""
    G, U, N = HO.IMP_GAUSSIAN, HO.IMP_UNIFORM, HO.IMP_NONE
    com = dict(eps=0.0, op_scale=1.5, op_shift=0.5, hard_mul_const=0.9)
    cases = []
    for D in (4, 5, 12):
        cs = tuple(0.1 + 0.07 * d for d in range(D))
        cases += [
            (f"harmonic_gauss_mask_D{D}", D, HO.Problem(potential=O.POT_HARMONIC, charge_or_k=0.5, sigma=3.0,
                                                          importance=G, **com), 4.0),
            (f"hydrogen_none_D{D}", D, HO.Problem(potential=O.POT_HYDROGEN, charge_or_k=1.0, sigma=1.0, importance=N,
                                                   **com), None),
            (f"cosine_uniform_D{D}", D, HO.Problem(potential=HO.POT_COSINE, pot_coef=cs, sigma=float(np.float32(np.pi)),
                                                    importance=U, **com), None),
            (f"harmonic_uniform_boxsqrt_D{D}", D, HO.Problem(potential=O.POT_HARMONIC, charge_or_k=0.5, sigma=4.0,
                                                              importance=U, box_mode=BO.BOX_SQRT, box_lim=4.0, **com),
             None),
            (f"hydrogen_gauss_mask_boxexp_D{D}", D, HO.Problem(potential=O.POT_HYDROGEN, charge_or_k=1.0, sigma=3.0,
                                                                importance=G, box_mode=BO.BOX_EXP, box_lim=4.0, **com),
             3.0),
            (f"zero_none_boxsqrt_mask_D{D}", D, HO.Problem(potential=BO.POT_ZERO, sigma=1.0, importance=N,
                                                            box_mode=BO.BOX_SQRT, box_lim=4.0, **com), 5.0),
        ]
    cases += [("h2_2d_gauss_mask_D4", 4, dataclasses.replace(_molecule("H2", 2), op_shift=0.5), 4.0),
              ("lih_3d_gauss_mask_D12", 12, dataclasses.replace(_molecule("LiH", 3), op_shift=0.5), 4.0),
              ("lih_3d_none_boxexp_D12", 12, dataclasses.replace(_molecule("LiH", 3), importance=HO.IMP_NONE,
                                                                  box_mode=BO.BOX_EXP, box_lim=4.0), None)]
    return cases


HOST_CASES = _host_cases()


@pytest.mark.parametrize("case", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_host_epilogue_product_rule(lib, case):
    what, D, prob, mask_scale = case
    B, L = 48, 3
    g = torch.Generator().manual_seed(17 + D)
    scales = None if mask_scale is None else mask_scale * (1.0 + 0.1 * torch.arange(L, dtype=torch.float64))
    x = XO.clear_batch(B, D, 3.5, scales, prob, 5 + D)
    assert float(XO.clearance(x, scales, prob).min()) > 0.1  # every row is measured, none is near a singular point
    # analytic heads u_l(x) = 1.5 + sin(a_l . x + phi_l): grad = a_l cos, Lap = -|a_l|^2 sin
    a = 0.6 * torch.randn(L, D, generator=g, dtype=torch.float64)
    ph = torch.randn(L, generator=g, dtype=torch.float64)
    arg = x @ a.T + ph
    u, lu = 1.5 + torch.sin(arg), -(a * a).sum(1) * torch.sin(arg)
    du = torch.cos(arg).unsqueeze(-1) * a  # (B, L, D)
    # float64 reference: double autograd of g = c sqrt p mask box u
    xr = x.clone().requires_grad_(True)
    ur = 1.5 + torch.sin(xr @ a.T + ph)
    mk = torch.ones(B, L, dtype=torch.float64) if scales is None else torch.exp(-xr.norm(dim=1, keepdim=True) / scales)
    gg = prob.hard_mul_const * BO.sqrt_importance(xr, prob) * mk * BO.box_mask(xr, prob) * ur
    lap = torch.zeros(B, L, dtype=torch.float64)
    for l in range(L):
        (gr,) = torch.autograd.grad(gg[:, l].sum(), xr, create_graph=True)
        for d in range(D):
            lap[:, l] += torch.autograd.grad(gr[:, d].sum(), xr, retain_graph=True)[0][:, d]
    sp0 = BO.sqrt_importance(x, prob)
    spc = torch.clamp(sp0, min=O.SQRT_P_CLAMP) if prob.importance != HO.IMP_NONE else sp0
    f64 = gg.detach() / spc
    Tf64 = prob.op_scale * -(-prob.scale_kinetic * lap / spc + HO.potential(x, prob) * f64) + prob.op_shift * f64
    jac64 = f64 / u
    dsc64 = None if scales is None else f64 * x.norm(dim=1, keepdim=True) / scales ** 2
    # the kernel's layout: (L, (D + 2) B) float32
    base = np.zeros((L, (D + 2) * B), np.float32)
    base[:, :B] = u.T.numpy()
    for d in range(D):
        base[:, (1 + d) * B:(2 + d) * B] = du[:, :, d].T.numpy()
    base[:, (D + 1) * B:] = lu.T.numpy()
    keep = []
    hp = THE.host_problem(prob, keep)
    sc = THE._f32(scales.numpy()) if scales is not None else THE._f32(np.zeros(L))
    xs = THE._f32(x.numpy())
    out = [np.full((B, L), np.nan, np.float32) for _ in range(4)]
    lib.run_exact(C.addressof(hp), D, B, L, int(scales is not None), THE._ptr(sc), THE._ptr(xs), THE._ptr(base),
                  base.shape[1], int(prob.box_mode), float(prob.box_lim), *[THE._ptr(o) for o in out])
    f, Tf, jac, dsc = out
    errs = dict(f=rel(f, f64), Tf=rel(Tf, Tf64), jac=rel(jac, jac64))
    if dsc64 is not None:
        errs["dsc"] = rel(dsc, dsc64)
    else:
        assert not dsc.any()
    print(what, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-5, (what, k, v)
    assert all(np.isfinite(o).all() for o in out)
