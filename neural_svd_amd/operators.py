"""Operator side of the PDE path with the reference's names: potentials, NegativeHamiltonian,
OperatorWrapper, get_problem, the Gaussian sampler / importance and the analytic spectra.

    hydrogen_potential / harmonic_oscillator_potential  examples/operator/pde/schrodinger/potentials.py:5-8,24-27
    infinite_well_potential                             examples/operator/pde/schrodinger/potentials.py:20-21
    NegativeHamiltonian                                 examples/operator/pde/schrodinger/__init__.py:4-22
    OperatorWrapper                                     examples/__init__.py:1-9
    cosine_potential / hydrogen_mol_ion_potential       examples/operator/pde/schrodinger/potentials.py:11-17,30-31
    NegativeLinearFokkerPlanck / sin_of_cos_potential   examples/operator/pde/others.py:6-34
    nuclear_energy / nuclear_potential / electronic_potential / local_potential_energy   potentials.py:35-57
    Molecule                                            examples/operator/pde/schrodinger/molecule.py
    get_problem                                         examples/operator/pde/problems.py:23-130 (ndim 5 / 10 and
                                                        quantum_chemistry under args.high_dim_stencil)
    get_dataloader                                      examples/operator/pde/main_pde.py:89-130 (gaussian sampler)
    Hydrogen2D / HarmonicOscillator / InfiniteWell2D    examples/operator/pde/schrodinger/ground_truths.py:40-149
      .get_qnums / .get_eigvals / .get_degeneracy / .eigfunc  (numpy float64 host mirror; the device evaluation is
                                                        nsvd_eigfunc_eval, csrc/eig_math.h)
    Hydrogen3D                                          examples/operator/pde/schrodinger/ground_truths.py:152-193, 204-270
      .get_qnums / .get_eigvals / .get_degeneracy / .eigfunc  (host mirror; on the device nsvd_eigfunc3_eval)

These objects are DESCRIPTORS on the scripts' configuration (Gaussian or uniform sampler / importance, or none): calling
``operator(method, x, importance)`` forwards to the fused HIP kernel (nsvd_operator_forward). With the Laplace
sampler of main_pde.py:101-112 (`--sampling_mode laplacian`: its importance density is not in the fused
kernel's epilogue) the wrapper applies the reference's finite-difference stencil itself (diff_ops.py:9-52,
schrodinger/__init__.py:16-22, examples/__init__.py:7-9) around 1 + 2D evaluations of the HIP model
(nsvd_model_forward / _backward): "python operator + fused loss kernel"  - still all on the GPU.
"""
from __future__ import annotations

import math
from functools import partial

import numpy as np
import torch

from . import hip_ops as H
from ._lib import NsvdError


# ----------------------------------------------------------------------------------- potentials
def hydrogen_potential(x, charge=1.0):
    """-Z / ||x|| (potentials.py:5-8). The fused kernels evaluate it in their epilogue (fd_math.h); this torch form
    serves the stencil applied outside them (non-Gaussian importance) and foreign operators."""
    x = x.reshape(x.shape[0], -1)
    return -(charge / x.norm(dim=1, p=2)).reshape(-1, 1)


def harmonic_oscillator_potential(x, k=1.0):
    """k ||x||^2 (potentials.py:24-27)."""
    x = x.reshape(x.shape[0], -1)
    return (k * x.norm(dim=1, p=2) ** 2).reshape(-1, 1)


def infinite_well_potential(x):
    """V = 0 inside the well (potentials.py:20-21); the walls are the model's Dirichlet box mask."""
    return torch.zeros((x.shape[0],), device=x.device)


def hydrogen_mol_ion_potential(x, R, charge=2.0):
    """H2+: -q / |x - R e_last| - q / |x + R e_last|, the nuclei on the last axis (potentials.py:11-17)."""
    x = x.reshape(x.shape[0], -1)
    e = torch.zeros((x.shape[-1],), device=x.device, dtype=x.dtype)
    e[-1] = 1.0
    return hydrogen_potential(x - R * e, charge) + hydrogen_potential(x + R * e, charge)


def _coefs(cs, x):
    """torch.tensor(cs): float32 roundings of the literals whatever the dtype of x, as the reference makes them"""
    return torch.tensor(cs, device=x.device).view(1, -1)


def cosine_potential(x, cs):
    """sum_d cs[d] cos x_d (potentials.py:30-31)."""
    return (torch.cos(x.view(x.shape[0], -1)) * _coefs(cs, x)).sum(-1)


def sin_of_cos_potential(xs, cs):
    """sin(sum_d cs[d] cos x_d): the drift potential of NegativeLinearFokkerPlanck (others.py:33-34)."""
    return torch.sin((torch.cos(xs) * _coefs(cs, xs)).sum(-1))


# ---- quantum chemistry (potentials.py:35-57): rs is (batch, n_electrons, ndim), mol carries coords (n_nuclei, ndim) and
# charges (n_nuclei,). The HIP kernels evaluate the same sum in their epilogue (fd_math.h: nsvd_molecule_potential).
def nuclear_energy(mol):
    """sum_{a<b} Z_a Z_b / |R_a - R_b|: the nuclear repulsion energy, a constant of the molecule"""
    coords, charges = mol.coords, mol.charges
    coulombs = charges[:, None] * charges / (coords[:, None] - coords).norm(dim=-1)
    return coulombs.triu(1).sum()


def nuclear_potential(rs, mol):
    """-sum_i sum_a Z_a / |r_i - R_a|"""
    dists = (rs[:, :, None] - mol.coords).norm(dim=-1)
    return -(mol.charges / dists).sum(dim=(-1, -2))


def electronic_potential(rs):
    """sum_{i<j} 1 / |r_i - r_j|"""
    i, j = np.triu_indices(rs.shape[-2], k=1)
    dists = (rs[:, :, None] - rs[:, None, :])[:, i, j].norm(dim=-1)
    return (1 / dists).sum(dim=-1)


def local_potential_energy(rs, mol):
    return nuclear_energy(mol) + nuclear_potential(rs, mol) + electronic_potential(rs)


ANGSTROM = 1 / 0.52917721092  # bohr per angstrom, the reference's constant (molecule.py)

# The package's own table of small systems, from public data: atoms at the origin, H2+ with its nuclei at
# x = +-0.52918 angstrom (2 bohr apart), bond lengths H2 0.742 and LiH 1.595 angstrom.
_SYSTEMS = {
    "H": dict(coords=[[0.0, 0.0, 0.0]], charges=[1], charge=0, spin=1, unit="angstrom"),
    "He": dict(coords=[[0.0, 0.0, 0.0]], charges=[2], charge=0, spin=0, unit="angstrom"),
    "Li": dict(coords=[[0.0, 0.0, 0.0]], charges=[3], charge=0, spin=1, unit="angstrom"),
    "Be": dict(coords=[[0.0, 0.0, 0.0]], charges=[4], charge=0, spin=0, unit="angstrom"),
    "B": dict(coords=[[0.0, 0.0, 0.0]], charges=[5], charge=0, spin=1, unit="angstrom"),
    "H2+": dict(coords=[[-0.52918, 0.0, 0.0], [0.52918, 0.0, 0.0]], charges=[1, 1], charge=1, spin=1,
                unit="angstrom"),
    "H2": dict(coords=[[0.0, 0.0, 0.0], [0.742, 0.0, 0.0]], charges=[1, 1], charge=0, spin=0, unit="angstrom"),
    "LiH": dict(coords=[[0.0, 0.0, 0.0], [1.595, 0.0, 0.0]], charges=[3, 1], charge=0, spin=0, unit="angstrom"),
}


def _load_systems(path):
    try:
        import tomllib as _toml
        with open(path, "rb") as fh:
            return _toml.load(fh)
    except ModuleNotFoundError:
        pass
    try:
        import toml as _toml
    except ModuleNotFoundError:
        raise NsvdError(f"Molecule.from_name: reading {path} needs tomllib (Python 3.11) or the toml package; neither "
                        f"is importable - pass `systems` as a dict instead") from None
    return _toml.load(path)


class Molecule(torch.nn.Module):
    """A molecule: nuclear coordinates (rows, atomic units after the unit conversion) and charges, its total charge and
    spin (molecule.py). ``coords`` / ``charges`` are buffers, float32 when built from Python numbers."""

    all_names = set(_SYSTEMS.keys())

    def __init__(self, coords, charges, charge, spin, unit="bohr", data=None):
        assert len(coords) == len(charges)
        super().__init__()
        unit_multiplier = {"bohr": 1.0, "angstrom": ANGSTROM}[unit]
        self.register_buffer("coords", unit_multiplier * torch.as_tensor(coords))
        self.register_buffer("charges", 1.0 * torch.as_tensor(charges))
        self.charge = charge
        self.spin = spin
        self.data = data or {}

    def __len__(self):
        return len(self.charges)

    def __iter__(self):
        yield from zip(self.coords, self.charges)

    def __repr__(self):
        return (f"Molecule(coords=\n{self.coords.cpu().numpy()},\n  charges={self.charges.cpu().numpy()},\n"
                f"  charge={self.charge}, spin={self.spin}\n)")

    @classmethod
    def from_name(cls, name, systems=None, **kwargs):
        """``systems``: a dict name -> {coords, charges, charge, spin, unit}, or the path of a TOML file holding one
        (read with tomllib / toml when importable); default: this package's own small table (Molecule.all_names)."""
        import copy
        import os
        if systems is None:
            systems = _SYSTEMS
        elif isinstance(systems, (str, os.PathLike)):
            systems = _load_systems(systems)
        if name not in systems:
            raise KeyError(f"Molecule.from_name: no system {name!r} (known: {sorted(systems)})")
        system = copy.deepcopy(dict(systems[name]))
        system.update(kwargs)
        coords = system.pop("coords")
        return cls(coords, **system)


def _potential_kind(ftn):
    """-> (NSVD_POT_*, charge_or_k, pot_coef) of a potential function of this module (or a partial of one)"""
    base, kw = ftn, {}
    if isinstance(ftn, partial):
        base, kw = ftn.func, ftn.keywords
    if base is hydrogen_potential:
        return H.POT_HYDROGEN, float(kw.get("charge", 1.0)), ()
    if base is harmonic_oscillator_potential:
        return H.POT_HARMONIC, float(kw.get("k", 1.0)), ()
    if base is infinite_well_potential:
        return H.POT_ZERO, 0.0, ()
    if base in (cosine_potential, sin_of_cos_potential):
        if "cs" not in kw:
            raise NsvdError(f"{base.__name__}: bind the coefficients, partial({base.__name__}, cs=[...])")
        cs = tuple(float(c) for c in kw["cs"])
        if len(cs) > _MAX_HIGH_DIM:
            raise NotImplementedError(f"{base.__name__} with {len(cs)} coefficients: {_TOO_MANY_HIGH_DIMS}")
        return (H.POT_COSINE if base is cosine_potential else H.POT_SIN_OF_COS), 0.0, cs
    if base is hydrogen_mol_ion_potential:
        if "R" not in kw:
            raise NsvdError("hydrogen_mol_ion_potential: bind the half-distance, partial(..., R=..., charge=...)")
        return H.POT_H2_ION, float(kw.get("charge", 2.0)), (float(kw["R"]),)
    if base is local_potential_energy:
        if "mol" not in kw:
            raise NsvdError("local_potential_energy: bind the molecule, partial(local_potential_energy, mol=...)")
        return H.POT_MOLECULE, 0.0, ()
    raise NsvdError("HIP path supports hydrogen_potential, harmonic_oscillator_potential, infinite_well_potential, "
                    "cosine_potential, hydrogen_mol_ion_potential, local_potential_energy and (Fokker-Planck) "
                    "sin_of_cos_potential only")


_MAX_STENCIL_DIM = 4  # NSVD_FD_MAXD (csrc/fd_math.h); the fused MFMA kernels take D <= 3
_TOO_MANY_DIMS = ("the finite-difference stencil of the HIP kernels carries at most 4 input dimensions (NSVD_FD_MAXD; "
                  "the fused MFMA kernels 3) - ndim 5 and 10 are not built")


_MAX_HIGH_DIM = 12  # NSVD_MAX_D (csrc/nsvd_common.h): the direction-loop stencil, finite-difference mode, generic kernels
_TOO_MANY_HIGH_DIMS = "the finite-difference stencil of the HIP kernels carries at most 12 input dimensions (NSVD_MAX_D)"


class ProblemConfigError(AssertionError, NotImplementedError):
    """A configuration get_problem refuses. The reference refuses the same ones with a bare ``assert``; earlier versions
    of this package raised NotImplementedError for the problems themselves - a handler written for either catches it."""


class NegativeHamiltonian:
    def __init__(self, local_potential_ftn, scale_kinetic=1.0, laplacian_eps=1e-5, n_particles=1):
        self.potential_kind, self.potential_param, self.potential_coef = _potential_kind(local_potential_ftn)
        if self.potential_kind == H.POT_SIN_OF_COS:
            raise NsvdError("sin_of_cos_potential is the drift potential of NegativeLinearFokkerPlanck")
        self.local_potential_ftn = local_potential_ftn
        self.scale_kinetic = scale_kinetic
        self.laplacian_eps = laplacian_eps
        self.n_particles = n_particles
        self.mol = local_potential_ftn.keywords["mol"] if self.potential_kind == H.POT_MOLECULE else None
        # laplacian_eps <= 0: exact Laplacian (reference diff_ops.py:7,54-61) - forward-mode jets on the MFMA path, or
        # on the generic kernels for a method built with path=PATH_GENERIC_EXACT (args.generic_exact_laplacian)

    def __call__(self, f, xs, importance=None, threshold=1e5):
        return OperatorWrapper(self)(f, xs, importance)


class NegativeLinearFokkerPlanck:
    """others.py:6-30: T f = scale (Lap f + grad V . grad f + f Lap V) with V = local_potential_ftn, every derivative -
    those of V too - the central difference with step ``laplacian_eps``; with an importance density p the stencil runs
    on g = sqrt(p) f and everything is divided by the UNCLAMPED sqrt p(x). ``laplacian_eps <= 0`` does not exist (the
    reference's own einsum fails on the exact-Laplacian gradient's shape)."""

    def __init__(self, local_potential_ftn, scale=1.0, laplacian_eps=1e-5):
        self.potential_kind, self.potential_param, self.potential_coef = _potential_kind(local_potential_ftn)
        if self.potential_kind != H.POT_SIN_OF_COS:
            raise NsvdError("HIP path: NegativeLinearFokkerPlanck takes partial(sin_of_cos_potential, cs=[...])")
        if not laplacian_eps > 0:
            raise NotImplementedError("NegativeLinearFokkerPlanck needs laplacian_eps > 0 (the reference has no exact-"
                                      "Laplacian Fokker-Planck either: others.py:27 fails there)")
        self.local_potential_ftn = local_potential_ftn
        self.scale = scale
        self.laplacian_eps = laplacian_eps
        self.n_particles = 1
        self.scale_kinetic = 1.0  # (unused by this operator; nsvd_problem carries the field)

    def __call__(self, f, xs, importance=None):
        return OperatorWrapper(self)(f, xs, importance)


class OperatorWrapper:
    def __init__(self, operator, scale=1.0, shift=0.0):
        if not isinstance(operator, (NegativeHamiltonian, NegativeLinearFokkerPlanck)):
            raise NotImplementedError("HIP path: OperatorWrapper wraps this package's NegativeHamiltonian or "
                                      "NegativeLinearFokkerPlanck")
        self.operator, self.scale, self.shift = operator, scale, shift

    @property
    def fokker_planck(self) -> bool:
        return isinstance(self.operator, NegativeLinearFokkerPlanck)

    def __call__(self, model, x, importance=None):
        """returns (scale * Tf + shift * f, f) like the reference; ``model`` is the NestedLoRA method."""
        return model.apply_operator(self, x, importance)

    def fused(self, importance) -> bool:
        """does the fused kernel (nsvd_operator_forward) implement this importance density?"""
        if self.fokker_planck:  # (with the Gaussian density the kernel refuses it: nsvd_path_name_for "unsupported")
            return importance is None or isinstance(importance, UniformImportance)
        return importance is None or isinstance(importance, (GaussianImportance, UniformImportance))

    def apply_stencil(self, model, x, importance):
        """The reference's own op sequence for densities the fused kernel does not carry (Laplace, uniform, any
        callable): g = sqrt(p) f at the 1 + 2D stencil points, lap_g = (sum g(x +- eps e_i) - 2D g(x)) / eps^2, divided
        by clamp(sqrt(p(x)), 1e-5) (diff_ops.py:9-52), -(-c lap + V fs) (schrodinger/__init__.py:16-22), scale / shift
        (examples/__init__.py:7-9). `model(z)` is the HIP model (nsvd_model_forward). Like the reference's float32 run
        the point-wise stencil carries percent-level rounding noise in Tf - the fused kernel's even / odd
        form does not exist outside it. The shifted evaluations are not recorded for autograd: the EVD loss gives Tf no
        gradient (methods/nestedlora.py:108-111)."""
        ham = self.operator
        eps = float(ham.laplacian_eps)
        if eps <= 0:
            raise NotImplementedError("exact Laplacian with a non-Gaussian importance: not built (use the Gaussian "
                                      "sampler, or laplacian_eps > 0)")
        x = x.reshape(x.shape[0], -1).float()
        D = x.shape[1]

        def g(z):
            return importance(z).sqrt() * model(z)
        gs = g(x)
        lap = -2.0 * D * gs.detach()
        fp = self.fokker_planck
        with torch.no_grad():
            adv = torch.zeros_like(lap)
            if fp:  # V differenced by the same stencil (others.py:25)
                def pot(z):
                    return ham.local_potential_ftn(z).view(-1, 1)
                V0 = pot(x)
                lap_v = -2.0 * D * V0
            for i in range(D):
                e = torch.zeros((1, D), device=x.device)
                e[0, i] = eps
                gp, gm = g(x + e), g(x - e)
                lap = lap + gp + gm
                if fp:
                    vp, vm = pot(x + e), pot(x - e)
                    lap_v = lap_v + vp + vm
                    adv = adv + ((vp - vm) / (2 * eps)) * ((gp - gm) / (2 * eps))
            lap = lap / eps ** 2
            # (the Fokker-Planck operator divides by the unclamped sqrt p: others.py:23-24)
            sw = importance(x).sqrt() if fp else torch.clamp(importance(x).sqrt(), min=1e-5)
            lap = lap / sw
        fs = gs / sw
        if fp:
            with torch.no_grad():
                Tf = ham.scale * (lap + adv / sw + fs * (lap_v / eps ** 2))
                Tf = self.scale * Tf + self.shift * fs
            return Tf, fs
        with torch.no_grad():
            V = ham.local_potential_ftn(x.reshape(x.shape[0], ham.n_particles, -1)).view(-1, 1)
            Tf = -(-ham.scale_kinetic * lap + V * fs)
            Tf = self.scale * Tf + self.shift * fs
        return Tf, fs


class GaussianImportance:
    """p(x) of the isotropic Gaussian sampler N(0, sigma^2 I) (reference main_pde.py:94-100)."""

    def __init__(self, sigma: float, dim: int):
        self.sigma, self.dim = float(sigma), int(dim)

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1)
        logp = (-0.5 * (x / self.sigma).pow(2).sum(-1) - self.dim * math.log(self.sigma)
                - 0.5 * self.dim * math.log(2 * math.pi))
        return logp.exp().view(-1, 1)


class LaplaceImportance:
    """p(x) = prod_i exp(-|x_i| / b) / (2 b) of the Laplace sampler (main_pde.py:101-112)."""

    def __init__(self, scale: float, dim: int):
        self.scale, self.dim = float(scale), int(dim)

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1)
        logp = (-x.abs() / self.scale - math.log(2 * self.scale)).sum(-1)
        return logp.exp().view(-1, 1)


class UniformImportance:
    """p(x) = 1 / (2 s)^ndim of the uniform sampler on [-s, s]^D (main_pde.py:113-118; the reference's exponent is
    args.ndim, kept)."""

    def __init__(self, scale: float, ndim: int):
        self.scale, self.ndim = float(scale), int(ndim)

    @property
    def sigma(self) -> float:
        """the sampling scale, under the name nsvd_problem carries it (NSVD_IMP_UNIFORM)"""
        return self.scale

    def __call__(self, x):
        return torch.full((x.shape[0], 1), 1.0 / (2 * self.scale) ** self.ndim, device=x.device).float()


class UniformBoxImportance:
    """p(x) = 1 / (2 lim)^D on the validation box (reference main_pde.py:129-130)."""

    def __init__(self, lim: float, dim: int):
        self.lim, self.dim = float(lim), int(dim)

    def __call__(self, x):
        return torch.full((x.shape[0], 1), 1.0 / (2 * self.lim) ** self.dim, device=x.device).float()


def fused_problem_of(operator, importance, model) -> H.Problem:
    """Translate (OperatorWrapper, importance, WaveFunctions) into the nsvd_problem the kernels take."""
    if not isinstance(operator, OperatorWrapper):
        raise NsvdError("fused operator kernel: operator must be neural_svd_amd.operators.OperatorWrapper (other "
                        "callables go through NestedLoRA.apply_operator's call-through, not this translation)")
    if importance is not None and not isinstance(importance, (GaussianImportance, UniformImportance)):
        raise NsvdError("fused operator kernel: importance must be None, GaussianImportance or UniformImportance (other "
                        "densities go through OperatorWrapper.apply_stencil)")
    ham = operator.operator
    kind = H.IMP_NONE if importance is None else \
        (H.IMP_UNIFORM if isinstance(importance, UniformImportance) else H.IMP_GAUSSIAN)
    D = model.shape.D
    n_particles = int(getattr(ham, "n_particles", 1) or 1)
    if D % n_particles:
        raise NsvdError(f"fused operator kernel: {n_particles} particles on a model of input dimension {D}")
    if kind == H.IMP_UNIFORM and importance.ndim != D // n_particles:
        # the kernel's exponent is the space dimension D / n_particles, as the reference's args.ndim (main_pde.py:118)
        raise NsvdError(f"fused operator kernel: UniformImportance(ndim={importance.ndim}) on a model of input "
                        f"dimension {D} with {n_particles} particle(s)")
    if len(ham.potential_coef) != (1 if ham.potential_kind == H.POT_H2_ION else D) and ham.potential_coef:
        raise NsvdError(f"fused operator kernel: {len(ham.potential_coef)} potential coefficients on a model of input "
                        f"dimension {D}")
    # ABI 5: tables longer than pot_coef (cs above 4 dimensions, the molecule's nuclei) travel as a device tensor
    extra, coef = {}, ham.potential_coef
    device = model.base.ws[0].device
    if ham.potential_kind == H.POT_MOLECULE:
        mol = ham.mol
        sd = D // n_particles
        if tuple(mol.coords.shape) != (len(mol.charges), sd):
            raise NsvdError(f"fused operator kernel: molecule coordinates {tuple(mol.coords.shape)} with "
                            f"{n_particles} particles on a model of input dimension {D}")
        table = torch.cat([mol.coords.float(), mol.charges.float().view(-1, 1)], dim=1).contiguous().to(device)
        extra = dict(pot_table=table, n_nuclei=len(mol.charges), pot_const=float(nuclear_energy(mol)))
    elif len(coef) > _MAX_STENCIL_DIM:
        extra = dict(pot_table=torch.tensor(coef, dtype=torch.float32, device=device))
        coef = ()
    fp = operator.fokker_planck
    if fp and kind == H.IMP_GAUSSIAN:
        raise NsvdError("fused operator kernel: the Fokker-Planck operator with the Gaussian density goes through "
                        "OperatorWrapper.apply_stencil (the reference's problems assert against that sampler)")
    return H.make_problem(ham.potential_kind, ham.potential_param, ham.laplacian_eps, operator.scale, operator.shift,
                          importance.sigma if importance is not None else 1.0, ham.scale_kinetic,
                          float(model.hard_mul_const), importance_kind=kind,
                          operator_kind=H.OP_FOKKER_PLANCK if fp else H.OP_SCHROEDINGER,
                          fp_scale=float(ham.scale) if fp else 0.0, pot_coef=coef,
                          n_particles=n_particles if n_particles > 1 else 0, **extra)


# ----------------------------------------------------------------------------------- ground truths
def _degeneracy(keys):
    """ToyProblem._get_degeneracy (ground_truths.py:22-37): cumulative level boundaries starting at 0, a level being a
    run of equal keys. Like the reference, a LAST level of a single state is not closed ([0, 1, 4] for 5 hydrogen
    states): a boundary is appended at the end only when the last run is longer than one."""
    cnt, prev, deg = 1, keys[0], [0]
    for k in keys[1:]:
        if k == prev:
            cnt += 1
        else:
            deg.append(cnt)
            prev, cnt = k, 1
    if cnt > 1:
        deg.append(cnt)
    return np.array(deg).cumsum()


def _laguerre(k, alpha, z):
    """generalised Laguerre L_k^(alpha)(z) by (j + 1) L_{j+1} = (2j + 1 + alpha - z) L_j - (j + alpha) L_{j-1}"""
    z = np.asarray(z, dtype=np.float64)
    lm, lc = np.zeros_like(z), np.ones_like(z)
    for j in range(k):
        lm, lc = lc, ((2 * j + 1 + alpha - z) * lc - (j + alpha) * lm) / (j + 1)
    return lc


def _hermite(n, u):
    """physicists' Hermite H_n(u) by H_{j+1} = 2 u H_j - 2 j H_{j-1}"""
    u = np.asarray(u, dtype=np.float64)
    hm, hc = np.zeros_like(u), np.ones_like(u)
    for j in range(n):
        hm, hc = hc, 2 * u * hc - 2 * j * hm
    return hc


class Hydrogen2D:
    """ground_truths.py:110-149. Differences from the reference, all deliberate: ``eigfunc`` returns the LIMIT at
    r = 0 (the finite value for l = 0, 0 otherwise) where the reference's formula is 0 * log 0 = NaN; the charge enters
    the functions, psi_Z(x) = Z psi_1(Z x) (the reference's eigfunc ignores it); hyp1f1 is the Laguerre recurrence
    (hyp1f1(-k, 2a + 1, z) = k! (2a)! / (k + 2a)! L_k^(2a)(z)), not scipy.special."""

    def __init__(self, charge=1.0):
        self.charge = charge

    def get_qnums(self, neigs):
        """(n, l), l = -n .. n, shell after shell (ground_truths.py:115-118)"""
        nmax = int(np.ceil(np.sqrt(neigs)))
        return [(n, l) for n in range(0, nmax + 1) for l in range(-n, n + 1)][:neigs]

    def get_eigvals(self, neigs):
        """E_n = -Z^2 / (4 (n + 1/2)^2), degeneracy 2n + 1, first ``neigs`` states."""
        shells, n = [], 0
        while len(shells) < neigs:
            shells += [n] * (2 * n + 1)
            n += 1
        q = np.array(shells[:neigs], dtype=np.float64)
        return -self.charge ** 2 / (4 * (q + 0.5) ** 2)

    def get_degeneracy(self, neigs):
        return _degeneracy([n for n, _ in self.get_qnums(neigs)])

    def eigfunc(self, n, l, r, th):
        """psi_{n,l}(r, th), numpy float64; for l < 0 the reference's sin(l th), negative l inside (:145)."""
        r, th = np.asarray(r, dtype=np.float64), np.asarray(th, dtype=np.float64)
        Z, a = float(self.charge), abs(int(l))
        z = Z * r / (n + 0.5)
        norm = Z / (n + 0.5) * math.exp(0.5 * (math.lgamma(n - a + 1) - math.lgamma(n + a + 1) - math.log(2 * n + 1)))
        radial = norm * z ** a * np.exp(-z / 2) * _laguerre(n - a, 2 * a, z)  # (0 ** 0 = 1: the l = 0 limit at r = 0)
        if l > 0:
            return radial * np.cos(l * th) / math.sqrt(math.pi)
        if l < 0:
            return radial * np.sin(l * th) / math.sqrt(math.pi)
        return radial / math.sqrt(2 * math.pi)


class Hydrogen3D:
    """ground_truths.py:152-193 with the real spherical harmonics of :218-270. The reference defines ``eigfunc`` and
    never evaluates it (its validation grid stops at ndim 2); here it is the float64 host mirror of the device
    evaluation (nsvd_eigfunc3_eval, csrc/eig_math.h): Laguerre and associated Legendre by their recurrences, no
    scipy.special. The charge enters as the reference's a0 = 2 / Z does."""

    def __init__(self, charge=1.0):
        self.charge = charge

    def get_qnums(self, neigs):
        """(n, l, m): n = 1 .. ascending, l = 0 .. n - 1, m = -l .. l (ground_truths.py:157-160)"""
        nmax = int(np.ceil(np.sqrt(neigs)))
        return [(n, l, m) for n in range(0, nmax + 1) for l in range(0, n) for m in range(-l, l + 1)][:neigs]

    def get_degeneracy(self, neigs):
        """the reference's routine over ITS OWN get_eigvals, short lists included: (0, 1, 5, 14, 30) for neigs = 55,
        whose eigenvalue list stops after the n = 4 shell"""
        return _degeneracy(list(self.get_eigvals(neigs)))

    def eigfunc(self, n, l, m, r, th, phi):
        """psi_{n,l,m} at (r, th, phi) = cartesian_to_spherical(x, y, z): th = arctan2(sqrt(x^2 + y^2), z) the polar
        angle, phi = arctan2(y, x). With rho = Z r / n, a = |m|:
            sqrt((Z/n)^3 / (2n) (n-l-1)! / (n+l)!) rho^l exp(-rho / 2) L_{n-l-1}^(2l+1)(rho)
            * sqrt((2l+1) / (4 pi) (l-a)! / (l+a)!) P_l^a(cos th) * {1, sqrt(2) cos(a phi) (m < 0), -sqrt(2) sin(a phi) (m > 0)}
        P_l^a without the Condon-Shortley phase: the reference's lpmv carries it and real_sph_harm's sign removes it.
        The pairing of negative m with the cosine is the reference's. At r = 0: 0 ** 0 = 1 for l = 0, exactly 0 otherwise."""
        r, th, phi = (np.asarray(v, dtype=np.float64) for v in (r, th, phi))
        n, l, m = int(n), int(l), int(m)
        a = abs(m)
        if not (n >= 1 and 0 <= l < n and a <= l):
            raise ValueError("n >= 1, 0 <= l < n, |m| <= l")
        Z, lf = float(self.charge), math.lgamma
        rho = Z * r / n
        radial = (math.sqrt((Z / n) ** 3 / (2 * n)) * math.exp(0.5 * (lf(n - l) - lf(n + l + 1))) * rho ** l *
                  np.exp(-rho / 2) * _laguerre(n - l - 1, 2 * l + 1, rho))
        ct, st = np.cos(th), np.sin(th)
        # P_a^a = (2a-1)!! sin^a, then (j - a + 1) P_{j+1} = (2j + 1) cos P_j - (j + a) P_{j-1}
        pm, pc = np.zeros_like(ct), math.exp(lf(2 * a + 1) - a * math.log(2.0) - lf(a + 1)) * st ** a
        for j in range(a, l):
            pm, pc = pc, ((2 * j + 1) * ct * pc - (j + a) * pm) / (j - a + 1)
        ang = math.sqrt((2 * l + 1) / (4 * math.pi)) * math.exp(0.5 * (lf(l - a + 1) - lf(l + a + 1))) * pc
        if m < 0:
            ang = ang * math.sqrt(2.0) * np.cos(a * phi)
        elif m > 0:
            ang = ang * (-math.sqrt(2.0)) * np.sin(a * phi)
        return radial * ang

    def get_eigvals(self, neigs):
        """E_n = -Z^2 / (4 n^2), degeneracy n^2. Like the reference the shells run over n < ceil(neigs^(1/3)) + 1 - its
        bound on sum n^2 - and the list is then cut to ``neigs``: when those shells hold fewer states it comes back
        SHORT (14 values for neigs = 16, 5 for neigs = 6). Kept: compare with ``[:len(result)]``."""
        max_n = int(np.ceil(neigs ** (1.0 / 3))) + 1
        q = np.array([n for n in range(1, max_n) for _ in range(n * n)], dtype=np.float64)
        return -self.charge ** 2 / (4 * q[:neigs] ** 2)


class HarmonicOscillator:
    """ground_truths.py:66-107. Difference from the reference, deliberate: ``eigfunc`` carries k, b = sqrt(k) in the
    reference's own formula (whose callers leave b = 1); Hermite by its recurrence, not np.polynomial."""

    def __init__(self, k=1.0, ndim=2):
        assert ndim == 2, f"dim={ndim} not implemented"
        self.k, self.ndim = k, ndim

    def get_qnums(self, neigs):
        """(i, n - i), i = 0 .. n, shell after shell (ground_truths.py:73-76)"""
        q, n = [], 0
        while len(q) < neigs:
            q += [(i, n - i) for i in range(n + 1)]
            n += 1
        return np.array(q[:neigs])

    def get_eigvals(self, neigs):
        """sqrt(k) (2n + D) with degeneracy n + 1.  Like the reference, whole shells are emitted up
        to one shell PAST the one that reaches ``neigs`` (never truncated): compare with ``[:neigs]``."""
        nend, states = 0, 0
        while True:
            states += nend + 1
            nend += 1
            if states >= neigs:
                break
        vals = [2 * n + self.ndim for n in range(nend + 1) for _ in range(n + 1)]
        return math.sqrt(self.k) * np.array(vals, dtype=np.float64)

    def get_degeneracy(self, neigs):
        """over get_eigvals' WHOLE shells, as the reference (its boundaries run past ``neigs``)"""
        return _degeneracy(list(self.get_eigvals(neigs)))

    def eigfunc(self, nx, ny, x, y):
        b = math.sqrt(self.k)

        def one(n, t):
            t = np.asarray(t, dtype=np.float64)
            return (math.exp(-0.5 * (n * math.log(2.0) + math.lgamma(n + 1))) * (b / math.pi) ** 0.25 *
                    np.exp(-b * t ** 2 / 2) * _hermite(n, math.sqrt(b) * t))
        return one(int(nx), x) * one(int(ny), y)


class InfiniteWell2D:
    """ground_truths.py:40-63. Differences from the reference, deliberate: ``get_qnums`` is ENERGY-ordered (the
    reference's list is not from the ninth state on: (3, 3), E ~ 18, precedes (4, 1), E ~ 17) - by nx^2 + ny^2, stable in
    the reference's generation order, equal to the reference's list for neigs <= 8; levels are grouped by integer
    equality of nx^2 + ny^2, which catches accidental degeneracies (50 = 5^2 + 5^2 = 7^2 + 1^2). ``eigfunc`` is the
    reference's, on [0, L]; ``eigfunc_box`` is the same function in this package's coordinates, the box [-lim, lim]^2
    with L = 2 lim as get_problem builds it, and 0 outside."""

    def __init__(self, L=1.0):
        self.L = L

    def get_qnums(self, neigs):
        neigs = int(neigs)
        gen = []
        for n in range(1, neigs + 2):  # nx, ny <= neigs covers the neigs lowest states (each (n, 1) is one)
            for i in range(1, n):
                gen += [(n, i), (i, n)]
            gen.append((n, n))
        return sorted(gen, key=lambda q: q[0] ** 2 + q[1] ** 2)[:neigs]  # (sorted is stable)

    def get_eigvals(self, neigs):
        """(n_x^2 + n_y^2) pi^2 / L^2 over n_x, n_y >= 1, ascending, first ``neigs`` values (ground_truths.py:40-58)."""
        # n_x, n_y <= neigs covers them: the neigs smallest values all have n_x, n_y <= neigs (each (n, 1) is one)
        n = np.arange(1, int(neigs) + 1, dtype=np.float64)
        vals = np.sort((n[:, None] ** 2 + n[None, :] ** 2).reshape(-1))[:int(neigs)]
        return vals * np.pi ** 2 / float(self.L) ** 2

    def get_degeneracy(self, neigs):
        return _degeneracy([nx * nx + ny * ny for nx, ny in self.get_qnums(neigs)])

    def eigfunc(self, nx, ny, x, y):
        L = float(self.L)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return 2 / L * np.sin(nx * np.pi * x / L) * np.sin(ny * np.pi * y / L)

    def eigfunc_box(self, nx, ny, x, y):
        lim = 0.5 * float(self.L)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        inside = (np.abs(x) <= lim) & (np.abs(y) <= lim)
        return np.where(inside, self.eigfunc(nx, ny, x + lim, y + lim), 0.0)


def ground_truth_of(args):
    """The ground truth with eigenfunction formulae that get_problem's configuration has (ndim 2: hydrogen, the
    oscillator with get_problem's k = 1, the well with its side 2 lim; ndim 3: hydrogen); ProblemConfigError for any
    other."""
    sch = getattr(args, "problem", "sch") == "sch"
    if sch and args.ndim == 3 and args.potential_type == "hydrogen":
        return Hydrogen3D(charge=args.charge)
    _require(sch and args.ndim == 2, "eigenfunction formulae: the 2-D Schroedinger problems and 3-D hydrogen only")
    if args.potential_type == "hydrogen":
        return Hydrogen2D(charge=args.charge)
    if args.potential_type == "harmonic_oscillator":
        return HarmonicOscillator(k=1.0, ndim=2)
    if args.potential_type == "infinite_well":
        return InfiniteWell2D(L=2 * args.lim)
    raise ProblemConfigError(f"potential_type {args.potential_type}: no eigenfunction formulae")


# cs and -eigenvalues of the periodic benchmark pair (Han, Lu and Zhou 2020), as problems.py:49-61 tabulates them
_COSINE_2D_CS = (0.814723686393179, 0.905791937075619)
_COSINE_2D_EIGVALS = (
    -0.591624518674115, 0.623365592493771, 0.662887867122419, 0.891545971509540, 0.982541637674317,
    1.877877978290306, 2.146058357306075, 2.197531748842203, 2.465712127857973, 3.699555061533076,
    3.701057706578779, 3.756708397099993, 3.758994296902169, 4.954067447329610, 4.955570092375313,
    4.971698508267879, 4.973984408070056, 5.239878887283648, 5.242164787085825, 5.273721217881508,
    5.275223862927211, 8.047887977307184, 8.049390622352888, 8.050173877109360, 8.051676522155063)


def _require(cond, what):
    if not cond:
        raise ProblemConfigError(what)


def _periodic_asserts(args, name):
    """the asserts the cosine and Fokker-Planck branches share (problems.py:39-44, 100-105)"""
    _require(args.lim == np.pi, f"{name}: --lim must be pi")
    _require(not args.apply_boundary, f"{name}: periodic problem, no --apply_boundary")
    _require(args.use_fourier_feature and args.fourier_deterministic,
             f"{name}: needs --use_fourier_feature and --fourier_deterministic (integer harmonics)")
    _require(args.sampling_mode != "gaussian", f"{name}: not with the Gaussian sampler")
    _require(args.ndim in (1, 2, 5, 10), f"{name}: ndim 1, 2, 5 or 10")
    if args.ndim > 2 and not getattr(args, "high_dim_stencil", False):
        raise ProblemConfigError(f"{name} with ndim {args.ndim}: {_TOO_MANY_DIMS}")
    if args.ndim > 2 and not (getattr(args, "generic_exact_laplacian", False) and name != "problem fp"):
        _require(args.laplacian_eps > 0, f"{name} with ndim {args.ndim}: the direction-loop stencil needs laplacian_eps "
                                         f"> 0 (no exact-Laplacian mode above 4 input dimensions)")


# cs and first eigenvalue of the 5-D and 10-D pair (problems.py:62-69, 106-111)
_COSINE_5D_CS = (0.162944737278636, 0.181158387415124, 0.025397363258701, 0.182675171227804, 0.126471849245082)
_COSINE_10D_CS = _COSINE_5D_CS + (0.019508080999882, 0.055699643773410, 0.109376303840997, 0.191501367086860,
                                  0.192977707039855)
_COSINE_HIGH_EIG = {5: 0.054018930536326, 10: 0.098087448866409}
_FP_CS = {1: [1.0], 2: [1.0, 1.0], 5: [1.0, 0.8, 0.6, 0.4, 0.2], 10: [0.1, 0.3, 0.2, 0.5, 0.2, 0.1, 0.3, 0.4, 0.2, 0.2]}


def get_problem(args, device=None):
    """problems.py:23-130. ndim 5 / 10 of the periodic pair and the quantum_chemistry branch (args.mol_name, ndim 2 or
    3, n_particles * ndim <= 12) are accepted when ``args.high_dim_stencil`` is true and refused as before without it.
    ``args.generic_exact_laplacian`` (opt-in, read with getattr) lifts the ``laplacian_eps > 0`` requirement of those
    Schroedinger problems: get_evd_method then builds the method on PATH_GENERIC_EXACT, whose jets carry the exact
    Laplacian up to 12 input dimensions (the Fokker-Planck problem has no exact mode and keeps the requirement).
    The cosine and Fokker-Planck branches of the reference
    read two names its own parser (main_pde.py) never defines; here ``args.use_gaussian_sampling`` is read as
    ``args.sampling_mode == "gaussian"`` and ``args.scale_operator`` as ``getattr(args, "scale_operator", 1.0)``.
    Refusals raise ProblemConfigError (an AssertionError, as the reference's asserts, and a NotImplementedError)."""
    gt = None
    args.n_particles = 1
    if args.problem == "fp":
        _periodic_asserts(args, "problem fp")
        cs = _FP_CS[args.ndim]
        gt = np.array([0.0] + (args.neigs - 1) * [0.0])
        inner = NegativeLinearFokkerPlanck(local_potential_ftn=partial(sin_of_cos_potential, cs=cs),
                                           scale=getattr(args, "scale_operator", 1.0),
                                           laplacian_eps=args.laplacian_eps)
        op = OperatorWrapper(inner, scale=args.operator_scale, shift=args.operator_shift)
        return op, args.operator_scale * gt + args.operator_shift
    if args.problem != "sch":
        raise NotImplementedError(f"problem {args.problem}: 'sch' and 'fp' are on the HIP path")
    scale_kinetic = 1.0
    if args.potential_type == "hydrogen":
        pot = partial(hydrogen_potential, charge=args.charge)
        if args.ndim == 2:
            gt = -Hydrogen2D(charge=args.charge).get_eigvals(args.neigs)
        elif args.ndim == 3:
            gt = -Hydrogen3D(charge=args.charge).get_eigvals(args.neigs)
    elif args.potential_type == "harmonic_oscillator":
        pot = partial(harmonic_oscillator_potential, k=1.0)
        gt = -HarmonicOscillator(k=1.0, ndim=args.ndim).get_eigvals(args.neigs)
    elif args.potential_type == "infinite_well":
        assert args.ndim == 2  # as the reference (problems.py:30)
        pot = infinite_well_potential
        gt = -InfiniteWell2D(L=2 * args.lim).get_eigvals(args.neigs)
    elif args.potential_type == "cosine":
        _periodic_asserts(args, "potential_type cosine")
        if args.ndim == 1:
            cs = [1.0]
        elif args.ndim > 2:
            cs = list(_COSINE_5D_CS if args.ndim == 5 else _COSINE_10D_CS)
            gt = np.array([_COSINE_HIGH_EIG[args.ndim]] + (args.neigs - 1) * [0.0])
        else:
            _require(args.neigs <= 25, "potential_type cosine: 25 eigenvalues are tabulated for ndim 2")
            cs = list(_COSINE_2D_CS)
            gt = -np.array(_COSINE_2D_EIGVALS[:args.neigs])
        pot = partial(cosine_potential, cs=cs)
    elif args.potential_type == "hydrogen_mol_ion":
        # (each nucleus gets 2 * args.charge, as problems.py:77 passes it)
        pot = partial(hydrogen_mol_ion_potential, R=args.hydrogen_mol_ion_R, charge=2 * args.charge)
    elif args.potential_type == "quantum_chemistry" and getattr(args, "high_dim_stencil", False):
        assert args.ndim in [2, 3]  # as the reference (problems.py:80)
        mol = Molecule.from_name(args.mol_name, systems=getattr(args, "mol_systems", None))
        if device is not None:
            mol = mol.to(device)
        if args.ndim == 2:
            mol.coords = mol.coords[:, :2]
        pot = partial(local_potential_energy, mol=mol)
        args.n_particles = int((mol.charges.sum() - mol.charge).type(torch.int).item())
        scale_kinetic = 0.5
        d = args.n_particles * args.ndim
        _require(args.n_particles >= 1, f"quantum_chemistry {args.mol_name}: no electrons")
        _require(d <= _MAX_HIGH_DIM, f"quantum_chemistry {args.mol_name} at ndim {args.ndim}: {d} input dimensions - "
                                     f"{_TOO_MANY_HIGH_DIMS}")
        _require(d <= _MAX_STENCIL_DIM or args.laplacian_eps > 0 or getattr(args, "generic_exact_laplacian", False),
                 f"quantum_chemistry with {d} input dimensions needs laplacian_eps > 0 (or args.generic_exact_laplacian: "
                 f"the exact Laplacian on the generic kernels)")
    else:
        raise NotImplementedError(f"potential_type {args.potential_type}: not in scope of the HIP path")
    ham = NegativeHamiltonian(local_potential_ftn=pot, scale_kinetic=scale_kinetic, laplacian_eps=args.laplacian_eps,
                              n_particles=args.n_particles)
    op = OperatorWrapper(ham, scale=args.operator_scale, shift=args.operator_shift)
    return op, (args.operator_scale * gt + args.operator_shift if gt is not None else None)


def get_dataloader(args, device):
    """-> make_batch_ftn_train, val_data, batch_ftn_val, importance_train, importance_val.
    The sampler draws on the DEVICE (the reference draws on the host and copies, main_pde.py:92-93)."""
    d = args.n_particles * args.ndim
    shape = (args.batch_size, args.n_particles, args.ndim)
    if args.sampling_mode == "gaussian":
        def make_batch_ftn_train():
            return args.sampling_scale * torch.randn(shape, device=device)

        importance_train = GaussianImportance(args.sampling_scale, d)
    elif args.sampling_mode == "laplacian":  # main_pde.py:101-112 (steps go through OperatorWrapper.apply_stencil)
        lap = torch.distributions.Laplace(torch.zeros(shape, device=device),
                                          args.sampling_scale * torch.ones(shape, device=device))

        def make_batch_ftn_train():
            return lap.sample()

        importance_train = LaplaceImportance(args.sampling_scale, d)
    elif args.sampling_mode == "uniform":  # main_pde.py:113-118
        def make_batch_ftn_train():
            return args.sampling_scale * (2 * torch.rand(shape, device=device) - 1)

        importance_train = UniformImportance(args.sampling_scale, args.ndim)
    else:
        raise NotImplementedError(f"--sampling_mode {args.sampling_mode}")
    if args.ndim in (1, 2) and args.n_particles == 1:
        ax = np.arange(-args.lim, args.lim, args.val_eps)
        xxs = np.meshgrid(*(args.ndim * [ax]))
        val_data = torch.tensor(np.array(list(zip(*[xx.flatten() for xx in xxs])))).to(device).float()

        def batch_ftn_val():
            n = int(np.ceil(len(val_data) / float(args.batch_size)))
            for i in range(n):
                yield val_data[i * args.batch_size:min((i + 1) * args.batch_size, len(val_data))], 0.0

        importance_val = UniformBoxImportance(args.lim, args.ndim)
    else:
        val_data, batch_ftn_val, importance_val = None, None, None
    return make_batch_ftn_train, val_data, batch_ftn_val, importance_train, importance_val
