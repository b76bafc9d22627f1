"""Problems above four input dimensions and the many-electron molecules on the CPU: the float64 restatement
(tests/_highdim_oracle.py) against the reference's own float64 run (tests/golden/highdim.npz, made by
tests/golden/make_golden_highdim.py), get_problem's opt-in branches, the Molecule table, the refusals and the host-side
path names."""
import argparse
import ast
import os
from functools import partial

import numpy as np
import pytest
import torch

from oracle import nsvd_oracle as O
from tests import _box_oracle as BO
from tests import _highdim_oracle as HO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "highdim.npz")
CASES = ("cos_5d", "fp_10d", "h2_2d", "h2_3d", "lih_3d")
MOLECULES = ("h2_2d", "h2_3d", "lih_3d")
DIMS = dict(cos_5d=5, fp_10d=10, h2_2d=4, h2_3d=6, lih_3d=12)


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def case_setup(z, name, dtype=torch.float64):
    cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
    names = [str(n) for n in z[f"{name}_param_names"]]
    t = lambda n: torch.tensor(z[f"{name}_param0_{n}"], dtype=dtype)  # noqa: E731
    sc = [t(n) for n in names if n.endswith("scales")]
    p = O.Params([t(n) for n in names if ".ws." in n], [t(n) for n in names if ".bs." in n],
                 torch.tensor(z[f"{name}_fourier_B"], dtype=dtype), sc[0] if sc else None)
    return cfg, names, p, HO.problem_of(cfg)


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a), dtype=torch.float64), torch.as_tensor(np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_float64(z, name):
    """the float64 bounds of test_periodic_oracle.py (1e-9), two steps with the RMSprop update between them"""
    cfg, names, p, prob = case_setup(z, name)
    assert cfg["neigs"] == 4 and cfg["batch_size"] == 64 and cfg["mlp_hidden_dims"] == "16,16"
    assert p.fourier_B.shape[0] == DIMS[name] and cfg["laplacian_eps"] == 0.01
    v, M = O.sequential_nesting_masks(cfg["neigs"])
    sq = [torch.zeros_like(t) for t in p.trainable()]
    for it in range(2):
        x = torch.tensor(z[f"{name}_x"][it], dtype=torch.float64)
        r = HO.loss_and_grads(x, p, prob, v, M)
        pre = f"{name}_f64_step{it}_"
        assert np.all(np.isfinite(z[pre + "f"])) and np.all(np.isfinite(z[pre + "Tf"]))
        scale = float((r["f"] * r["Tf"]).abs().sum()) / x.shape[0]
        assert abs(float(r["loss"]) - float(z[pre + "loss"])) < 1e-9 * scale
        assert rel(r["f"], z[pre + "f"]) < 1e-9
        assert rel(r["Tf"], z[pre + "Tf"]) < 1e-9
        for group, rows in HO.row_groups(x, prob):  # the near-nucleus / near-coalescence rows as groups of their own
            assert rel(r["Tf"][rows], z[pre + "Tf"][rows.numpy()]) < 1e-9, group
        for n, g in zip(names, r["grads"]):
            assert rel(g, z[pre + f"grad_{n}"]) < 1e-9, n
        lr = O.cosine_lr(cfg["lr"], it, cfg["num_iters"])
        O.rmsprop_step(p.trainable(), r["grads"], sq, lr, cfg["rmsprop_decay"], 1e-10)


@pytest.mark.parametrize("name", MOLECULES)
def test_molecule_rows_and_potential(z, name):
    """the fixture's row conditions, and local_potential_energy: the restatement and this package's torch forms against
    the reference's recorded values on the 64 rows of step 0"""
    from neural_svd_amd.operators import (Molecule, electronic_potential, local_potential_energy, nuclear_energy,
                                          nuclear_potential)
    cfg, names, p, prob = case_setup(z, name)
    assert prob.n_particles * cfg["ndim"] == DIMS[name] and prob.scale_kinetic == 0.5
    for it in range(z[f"{name}_x"].shape[0]):
        x = torch.tensor(z[f"{name}_x"][it])
        en, ee = HO.distances(x, prob)
        assert float(en.min()) > 1e-3 and float(ee.min()) > 1e-3
        assert int((en < 0.1).sum()) >= 4 and int((ee < 0.1).sum()) >= 4
        groups = dict(HO.row_groups(x, prob))
        assert all(int(rows.sum()) >= 4 for rows in groups.values())
    x = torch.tensor(z[f"{name}_x"][0], dtype=torch.float64)
    want = torch.tensor(z[f"{name}_V"])
    assert bool(torch.isfinite(want).all())
    assert rel(HO.molecule_potential(x, prob).view(-1), want) < 1e-12
    mol = Molecule.from_name(cfg["mol_name"])
    assert len(mol) == len(z[f"{name}_mol_charges"]) and len(list(mol)) == len(mol)
    if cfg["ndim"] == 2:
        mol.coords = mol.coords[:, :2]
    assert mol.coords.dtype == torch.float32
    assert np.array_equal(mol.coords.numpy(), z[f"{name}_mol_coords"])
    assert np.array_equal(mol.charges.numpy(), z[f"{name}_mol_charges"])
    assert float(nuclear_energy(mol)) == float(z[f"{name}_nuclear_energy"]) == prob.pot_const
    rs = x.reshape(x.shape[0], prob.n_particles, -1)
    assert torch.equal(local_potential_energy(rs, mol), want)
    assert torch.equal(nuclear_energy(mol) + nuclear_potential(rs, mol) + electronic_potential(rs), want)


def _args(cfg, **over):
    a = argparse.Namespace(**dict(cfg, **over))
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=1, sequential=1))
    return a


@pytest.mark.parametrize("name", CASES)
def test_get_problem_under_the_switch(z, name):
    """cs, ground truths, n_particles and scale_kinetic as the reference's get_problem sets them"""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.operators import NegativeHamiltonian, NegativeLinearFokkerPlanck, get_problem
    cfg = ast.literal_eval(str(z[f"{name}_cfg"]))
    a = _args(cfg, high_dim_stencil=True, n_particles=-1)
    op, gt = get_problem(a)
    prob, inner = HO.problem_of(cfg), op.operator
    assert inner.potential_kind == prob.potential and a.n_particles == prob.n_particles == cfg["n_particles"]
    assert inner.n_particles == prob.n_particles and inner.laplacian_eps == cfg["laplacian_eps"]
    assert op.scale == cfg["operator_scale"] and op.shift == cfg["operator_shift"]
    if name in MOLECULES:
        assert isinstance(inner, NegativeHamiltonian) and inner.scale_kinetic == 0.5 and gt is None
        assert inner.potential_kind == H.POT_MOLECULE == 7 and inner.potential_coef == ()
        assert np.array_equal(inner.mol.coords.numpy(), z[f"{name}_mol_coords"])
        return
    assert tuple(inner.potential_coef) == tuple(prob.pot_coef) == tuple(z[f"{name}_cs"])
    np.testing.assert_allclose(gt, z[f"{name}_gt"], rtol=1e-14, atol=0)
    if cfg["problem"] == "fp":
        assert isinstance(inner, NegativeLinearFokkerPlanck) and inner.scale == cfg["scale_operator"] == 0.5
    else:
        assert isinstance(inner, NegativeHamiltonian) and inner.scale_kinetic == 1.0


def test_tables_at_the_other_dimensions(z):
    from neural_svd_amd.operators import get_problem
    for key, base, nd in (("cos_10d", "cos_5d", 10), ("fp_5d", "fp_10d", 5)):
        cfg = ast.literal_eval(str(z[f"{base}_cfg"]))
        op, gt = get_problem(_args(cfg, ndim=nd, high_dim_stencil=True))
        assert tuple(op.operator.potential_coef) == tuple(z[f"{key}_cs"])
        np.testing.assert_allclose(gt, z[f"{key}_gt"], rtol=1e-14, atol=0)
    assert z["cos_5d_gt"][0] == 10.0 + HO.COSINE_FIRST_EIGVAL[5] and z["cos_10d_gt"][0] == 10.0 + HO.COSINE_FIRST_EIGVAL[10]
    assert tuple(z["cos_10d_cs"]) == HO.COSINE_CS[10] and tuple(z["fp_5d_cs"]) == HO.FP_CS[5]


def test_refusals(z):
    """without the switch today's refusals stand; with it: more than 12 input dimensions, eps <= 0, unknown names"""
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.operators import (Molecule, NegativeHamiltonian, ProblemConfigError, cosine_potential,
                                          get_problem, local_potential_energy)
    cos = ast.literal_eval(str(z["cos_5d_cfg"]))
    fp = ast.literal_eval(str(z["fp_10d_cfg"]))
    mol = ast.literal_eval(str(z["h2_3d_cfg"]))
    for cfg in (cos, fp):
        for nd in (5, 10):
            for over in (dict(), dict(high_dim_stencil=False)):
                with pytest.raises(NotImplementedError, match="at most 4 input dimensions"):
                    get_problem(_args(cfg, ndim=nd, **over))
            with pytest.raises(AssertionError, match="laplacian_eps"):
                get_problem(_args(cfg, ndim=nd, high_dim_stencil=True, laplacian_eps=0.0))
        with pytest.raises(AssertionError):  # (the reference's assert on ndim stands under the switch)
            get_problem(_args(cfg, ndim=3, high_dim_stencil=True))
    with pytest.raises(NotImplementedError):
        get_problem(_args(mol))
    a = _args(mol, mol_name="Be", high_dim_stencil=True)  # 4 electrons in 3-D: 12, the limit
    op, _ = get_problem(a)
    assert a.n_particles == 4 and op.operator.n_particles == 4
    with pytest.raises(ProblemConfigError, match="at most 12"):  # 5 electrons in 3-D: 15
        get_problem(_args(mol, mol_name="B", high_dim_stencil=True))
    with pytest.raises(AssertionError):
        get_problem(_args(mol, ndim=4, high_dim_stencil=True))
    with pytest.raises(AssertionError, match="laplacian_eps"):
        get_problem(_args(mol, high_dim_stencil=True, laplacian_eps=0.0))
    with pytest.raises(KeyError):
        get_problem(_args(mol, mol_name="Xx", high_dim_stencil=True))
    with pytest.raises(NotImplementedError, match="at most 12"):
        NegativeHamiltonian(partial(cosine_potential, cs=[1.0] * 13))
    with pytest.raises(NsvdError, match="mol"):
        NegativeHamiltonian(local_potential_energy)
    # systems: a dict of the caller's, or a path (a clear error when no TOML reader is importable)
    he = Molecule.from_name("X", systems=dict(X=dict(coords=[[0.0, 0.0, 1.0]], charges=[2], charge=0, spin=0)))
    assert float(he.coords[0, 2]) == 1.0 and he.charge == 0 and len(he) == 1
    try:
        import tomllib  # noqa: F401
    except ModuleNotFoundError:
        try:
            import toml  # noqa: F401
        except ModuleNotFoundError:
            with pytest.raises(NsvdError, match="tomllib"):
                Molecule.from_name("H2", systems=os.path.join(os.path.dirname(GOLDEN), "no_such.toml"))


FAKE_TABLE = 256  # a non-null address: the host-side queries look at the pointer's presence only


def test_path_names_and_abi5_fields():
    """host-side queries, no GPU: every 'invalid' / 'unsupported' rule of ABI 5, and the all-zero tail is ABI 4's"""
    from neural_svd_amd import hip_ops as H
    PI = float(np.pi)

    def shape(D, hidden=(16, 16), m=8, **kw):
        return H.ModelShape(L=4, D=D, m=m, hidden=hidden, **kw)

    def name(D, pot, table_len=None, eps=0.01, imp=H.IMP_UNIFORM, path=H.PATH_AUTO, sh=None, **kw):
        prob = H.make_problem(pot, 1.0, eps, 1.0, 0.0, PI, importance_kind=imp, **kw)
        if table_len is not None:
            prob.pot_table, prob.pot_table_len = FAKE_TABLE, table_len
        return H.path_name(sh or shape(D), 64, path, prob)

    fp = dict(operator_kind=H.OP_FOKKER_PLANCK, fp_scale=1.0)
    for D in (5, 10, 12):
        assert name(D, H.POT_COSINE, D) == "generic" and name(D, H.POT_SIN_OF_COS, D, **fp) == "generic"
        assert name(D, H.POT_COSINE, D, path=H.PATH_GENERIC) == "generic"
        assert name(D, H.POT_COSINE) == "invalid"                       # no table
        assert name(D, H.POT_COSINE, D - 1) == "invalid" and name(D, H.POT_SIN_OF_COS, D + 1, **fp) == "invalid"
        assert name(D, H.POT_COSINE, D, eps=0.0) == "unsupported"       # no exact-Laplacian mode above 4 dimensions
        assert name(D, H.POT_HYDROGEN, imp=H.IMP_GAUSSIAN, eps=-1.0) == "unsupported"
        assert name(D, H.POT_HYDROGEN, imp=H.IMP_GAUSSIAN) == "generic"
        # 128-wide models: the MFMA forward in split form on explicit request only; auto stays generic (not measured)
        assert name(D, H.POT_COSINE, D, path=H.PATH_FUSED, sh=shape(D, (128, 128), 64)) == "fused_mfma"
        assert name(D, H.POT_COSINE, D, path=H.PATH_FUSED_BF16X3, sh=shape(D, (128, 128), 64)) == "unsupported"
        assert name(D, H.POT_COSINE, D, path=H.PATH_FUSED, eps=0.0, sh=shape(D, (128, 128), 64)) == "unsupported"
        assert name(D, H.POT_COSINE, D, sh=shape(D, (128, 128), 64)) == "generic"
        for path in (H.PATH_FUSED, H.PATH_FUSED_BF16X3):                # other shapes have no MFMA path
            assert name(D, H.POT_COSINE, D, path=path) == "unsupported"
    assert name(13, H.POT_COSINE, 13) == "unsupported" and name(13, H.POT_HYDROGEN) == "unsupported"
    assert name(13, H.POT_COSINE, 12) == "invalid"
    # D <= 4 keeps pot_coef: a table is neither needed nor looked at
    assert name(2, H.POT_COSINE, pot_coef=(0.8, 0.9)) == "generic"
    # the molecule: d = D / n_particles in {2, 3}, n_nuclei (d + 1) table entries, Schroedinger kind only
    mol = dict(imp=H.IMP_GAUSSIAN, scale_kinetic=0.5)
    assert name(4, H.POT_MOLECULE, 6, n_particles=2, n_nuclei=2, **mol) == "generic"     # H2 in 2-D
    assert name(6, H.POT_MOLECULE, 8, n_particles=2, n_nuclei=2, **mol) == "generic"     # H2 in 3-D
    assert name(12, H.POT_MOLECULE, 8, n_particles=4, n_nuclei=2, **mol) == "generic"    # LiH in 3-D
    assert name(12, H.POT_MOLECULE, 4, n_particles=4, n_nuclei=1, **mol) == "generic"    # Be in 3-D
    assert name(3, H.POT_MOLECULE, 4, n_nuclei=1, **mol) == "generic"                    # n_particles 0 is read as 1
    assert name(2, H.POT_MOLECULE, 3, n_particles=1, n_nuclei=1, sh=shape(2, (128, 128, 128), 64), **mol) == "fused_mfma"
    assert name(6, H.POT_MOLECULE, 8, n_particles=2, n_nuclei=0, **mol) == "invalid"     # no nucleus
    assert name(6, H.POT_MOLECULE, 8, n_particles=4, n_nuclei=2, **mol) == "invalid"     # 6 % 4
    assert name(8, H.POT_MOLECULE, 10, n_particles=2, n_nuclei=2, **mol) == "invalid"    # d = 4
    assert name(4, H.POT_MOLECULE, 4, n_particles=4, n_nuclei=2, **mol) == "invalid"     # d = 1
    assert name(6, H.POT_MOLECULE, 6, n_particles=2, n_nuclei=2, **mol) == "invalid"     # table of the wrong length
    assert name(6, H.POT_MOLECULE, None, n_particles=2, n_nuclei=2, **mol) == "invalid"  # no table
    assert name(6, H.POT_MOLECULE, 8, n_particles=2, n_nuclei=2, **dict(mol, imp=H.IMP_NONE, **fp)) == "invalid"
    assert name(6, H.POT_MOLECULE, 8, n_particles=2, n_nuclei=2, eps=0.0, **mol) == "unsupported"
    assert name(15, H.POT_MOLECULE, 4, n_particles=5, n_nuclei=1, **mol) == "unsupported"  # B in 3-D
    assert name(6, 6) == "invalid" and name(6, 8) == "invalid"                           # 6 stays unassigned
    # all-zero appended fields: the problems of ABI 4, unchanged
    old = H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, 16.0)
    assert (old.n_particles, old.n_nuclei, old.pot_table_len, old.pot_const, old.pot_table) == (0, 0, 0, 0.0, None)
    assert list(old.pot_coef) == [0.0] * 4
    with pytest.raises(Exception, match="must live on the GPU"):
        H.make_problem(H.POT_COSINE, 0.0, 0.01, 1.0, 0.0, 1.0, pot_table=torch.zeros(5))
    # workspace of the generic path at E = 25 stencil blocks
    assert H.workspace_bytes(shape(12), 64) > H.workspace_bytes(shape(4), 64) > 0
    with pytest.raises(Exception):
        H.workspace_bytes(shape(13), 64)


def test_uniform_density_uses_the_space_dimension():
    """(2 sigma)^-ndim with ndim the space dimension (main_pde.py:118): fused_problem_of accepts
    UniformImportance(ndim) on a model of n_particles * ndim inputs and refuses another exponent"""
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.operators import UniformImportance
    imp = UniformImportance(2.0, 3)
    assert float(imp(torch.zeros(2, 6))[0, 0]) == float(np.float32(1.0 / 4.0 ** 3))
    import neural_svd_amd.operators as OPS

    class _Model:
        hard_mul_const = 1.0

        class shape:
            D = 6

        class base:
            ws = [torch.zeros(1)]

    ham = OPS.NegativeHamiltonian(OPS.infinite_well_potential, laplacian_eps=0.01, n_particles=2)
    prob = OPS.fused_problem_of(OPS.OperatorWrapper(ham), imp, _Model())
    assert prob.n_particles == 2 and prob.use_importance == 2
    with pytest.raises(NsvdError, match="UniformImportance"):
        OPS.fused_problem_of(OPS.OperatorWrapper(ham), UniformImportance(2.0, 6), _Model())


@pytest.mark.parametrize("name", ("h2_3d",))
def test_apply_stencil_molecule_matches_restatement(z, name):
    """OperatorWrapper.apply_stencil (the torch path for densities the kernels do not carry) takes the molecule
    potential with the reference's op sequence: run on the CPU in float64 around the restatement's model"""
    from neural_svd_amd.operators import Molecule, NegativeHamiltonian, OperatorWrapper, local_potential_energy
    cfg, names, p, prob = case_setup(z, name)
    x = torch.tensor(z[f"{name}_x"][0], dtype=torch.float64)
    mol = Molecule.from_name(cfg["mol_name"])
    op = OperatorWrapper(NegativeHamiltonian(partial(local_potential_energy, mol=mol), 0.5,
                                             float(np.float32(cfg["laplacian_eps"])), prob.n_particles),
                         scale=cfg["operator_scale"], shift=cfg["operator_shift"])

    class Imp:
        def __call__(self, t):
            return BO.sqrt_importance(t.double(), prob) ** 2

    Tf, f = op.apply_stencil(lambda t: BO.wave(t.double(), p, prob), x, Imp())
    c = HO.operator_forward(x, p, prob)
    assert rel(f, c.f) < 1e-12
    assert rel(Tf, c.Tf) < 1e-3  # float32 stencil points (test_periodic_oracle's bound for the same path)
