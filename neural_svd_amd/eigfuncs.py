"""Eigenfunction accuracy against the analytic ground truths: the second half of the reference's evaluation
(examples/operator/pde/schrodinger/ground_truths.py eigfunc / get_qnums / get_degeneracy; examples/linalg.py
subspace_distance :5-8, rotate :11-16, procrustes :19-28).

The reference's functions take the (n, L) blocks of learned and true functions on the validation grid. Here the grid
pass leaves three small float64 matrices (hip_ops.eigfunc_accumulate: the ground truths are evaluated and contracted on
the device, chunk by chunk, nothing of size n is stored or copied):

    gram (Lg, Lg) = Psi^T Psi / n,   cross (Lg, L) = Psi^T Phi / n,   cov (L, L) = Phi^T Phi / n

and every metric below is host numpy float64 on those, as compute_spectrum_evd post-processes cov and quad. Lg >= L:
the ground-truth table always ends on a level boundary, because a metric over a degenerate level needs the whole level.
No formula assumes gram = I: the box and the grid lose part of the outer shells (``gram_defect`` says how much).

Two families of ground truths: the three 2-D ones (GroundTruthTable, pairs of quantum numbers, nsvd_eigfunc_*) and the
3-D hydrogen atom (GroundTruthTable3D, triples (n, l, m), nsvd_eigfunc3_*: Hydrogen3D.eigfunc :177-193 with the real
spherical harmonics :218-270). Accumulator takes either; the metrics do not know the dimension.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import NsvdError
from . import operators as O

MAX_FUNCTIONS = 80  # NSVD_EIG_MAX_FN: the table travels by value in the launch arguments


@dataclass(frozen=True)
class GroundTruthTable:
    """What the two entry points take of a ground truth, and the level boundaries of its Lg functions
    (``degeneracy``: cumulative, from 0 to Lg, EVERY level closed - unlike get_degeneracy, which follows the reference
    and leaves a last level of one state open)."""
    kind: int
    param: float
    qnums: Tuple[Tuple[int, int], ...]
    degeneracy: Tuple[int, ...]

    ndim = 2  # columns of x; the entry points are nsvd_eigfunc_eval / nsvd_eigfunc_accumulate_f64

    @property
    def Lg(self) -> int:
        return len(self.qnums)


@dataclass(frozen=True)
class GroundTruthTable3D(GroundTruthTable):
    """The same for a ground truth on R^3: ``qnums`` are triples (n, l, m), the kind is GT_HYDROGEN3D and the entry
    points are nsvd_eigfunc3_eval / nsvd_eigfunc3_accumulate_f64. A type and a builder of its own
    (ground_truth_table_3d): ground_truth_table and the 2-D entry points keep refusing what they refused."""
    qnums: Tuple[Tuple[int, int, int], ...]
    ndim = 3


def _level_keys(gt, neigs) -> Tuple[int, float, list, list]:
    if isinstance(gt, O.Hydrogen2D):
        q = gt.get_qnums(neigs)
        return _lib.GT_HYDROGEN2D, float(gt.charge), q, [n for n, _ in q]
    if isinstance(gt, O.HarmonicOscillator):
        q = [tuple(int(v) for v in r) for r in gt.get_qnums(neigs)]
        return _lib.GT_HARMONIC2D, float(gt.k), q, [a + b for a, b in q]
    if isinstance(gt, O.InfiniteWell2D):
        q = gt.get_qnums(neigs)
        return _lib.GT_WELL2D, 0.5 * float(gt.L), q, [a * a + b * b for a, b in q]
    raise NsvdError(f"no two-dimensional eigenfunction formulae for {type(gt).__name__}: Hydrogen2D, "
                    f"HarmonicOscillator (ndim 2) and InfiniteWell2D have them (Hydrogen3D: ground_truth_table_3d)")


def ground_truth_table(ground_truth, L: int) -> GroundTruthTable:
    """The first Lg states of ``ground_truth``, Lg the end of the level that holds state L - 1 (hydrogen L = 16 -> 16,
    oscillator L = 32 -> 36, L = 64 -> 66). The three 2-D ground truths only: Hydrogen3D goes through
    ground_truth_table_3d, and is refused here as it always was."""
    L = int(L)
    if L < 1:
        raise ValueError("L >= 1")
    kind, param, q, keys = _level_keys(ground_truth, L + 40)  # (no level of the first 80 + states is 40 long)
    e = L
    while e < len(keys) and keys[e] == keys[L - 1]:
        e += 1
    if e > MAX_FUNCTIONS or e == len(keys):
        raise NsvdError(f"the level of state {L} ends past {MAX_FUNCTIONS} functions")
    bounds = [0] + [i for i in range(1, e) if keys[i] != keys[i - 1]] + [e]
    return GroundTruthTable(kind, param, tuple((int(a), int(b)) for a, b in q[:e]), tuple(bounds))


def ground_truth_table_3d(ground_truth, L: int) -> GroundTruthTable3D:
    """The first Lg states of operators.Hydrogen3D, Lg the end of the shell that holds state L - 1: the shells end at
    1, 5, 14, 30, 55 (L = 4 -> 5, L = 16 -> 30, L = 55 -> 55); L >= 56 is refused, the n = 6 shell ends at 91 > 80."""
    L = int(L)
    if L < 1:
        raise ValueError("L >= 1")
    if not isinstance(ground_truth, O.Hydrogen3D):
        raise NsvdError(f"no three-dimensional eigenfunction formulae for {type(ground_truth).__name__}: Hydrogen3D "
                        f"has them")
    bounds = [0]
    while bounds[-1] < L:
        bounds.append(bounds[-1] + len(bounds) ** 2)
    if bounds[-1] > MAX_FUNCTIONS:
        raise NsvdError(f"the level of state {L} ends past {MAX_FUNCTIONS} functions")
    q = ground_truth.get_qnums(bounds[-1])
    assert [n for n, _, _ in q] == [n for n in range(1, len(bounds)) for _ in range(n * n)]
    return GroundTruthTable3D(_lib.GT_HYDROGEN3D, float(ground_truth.charge),
                              tuple((int(n), int(l), int(m)) for n, l, m in q), tuple(bounds))


def table_of(ground_truth, L: int) -> GroundTruthTable:
    """a table as it is, Hydrogen3D through ground_truth_table_3d, every other ground truth through ground_truth_table"""
    if isinstance(ground_truth, GroundTruthTable):
        return ground_truth
    if isinstance(ground_truth, O.Hydrogen3D):
        return ground_truth_table_3d(ground_truth, L)
    return ground_truth_table(ground_truth, L)


def evaluate_host(ground_truth, qnums, x) -> np.ndarray:
    """psi (n, len(qnums)) float64 on the HOST, through the ground truth's own eigfunc (numpy): x (n, 2) in this
    package's coordinates (the well's box is [-lim, lim]^2), (n, 3) for Hydrogen3D. The route the device evaluation
    replaces; kept for comparison (scripts/eval_eigfuncs.py --timing) and for callers without a GPU."""
    x = np.asarray(x, dtype=np.float64)
    if isinstance(ground_truth, O.Hydrogen3D):
        if x.ndim != 2 or x.shape[1] != 3:
            raise NsvdError("evaluate_host: Hydrogen3D takes x (n, 3)")
        s2 = x[:, 0] ** 2 + x[:, 1] ** 2
        r, th, ph = np.sqrt(s2 + x[:, 2] ** 2), np.arctan2(np.sqrt(s2), x[:, 2]), np.arctan2(x[:, 1], x[:, 0])
        return np.stack([ground_truth.eigfunc(n, l, m, r, th, ph) for n, l, m in qnums], 1)
    if isinstance(ground_truth, O.Hydrogen2D):
        r, th = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2), np.arctan2(x[:, 1], x[:, 0])
        return np.stack([ground_truth.eigfunc(n, l, r, th) for n, l in qnums], 1)
    if isinstance(ground_truth, O.HarmonicOscillator):
        return np.stack([ground_truth.eigfunc(a, b, x[:, 0], x[:, 1]) for a, b in qnums], 1)
    if isinstance(ground_truth, O.InfiniteWell2D):
        return np.stack([ground_truth.eigfunc_box(a, b, x[:, 0], x[:, 1]) for a, b in qnums], 1)
    raise NsvdError(f"no eigenfunction formulae for {type(ground_truth).__name__}")


def _inv_sqrt(M):
    w, V = np.linalg.eigh(M)
    return (V / np.sqrt(w)) @ V.T


def eigenfunction_metrics(gram, cross, cov, degeneracy: Sequence[int], order: Optional[Sequence[int]] = None) -> dict:
    """gram (Lg, Lg), cross (Lg, L), cov (L, L): the three products above (divided by n; only ``gram_defect`` sees the
    scale). degeneracy: level boundaries of the ground truths, from 0 to Lg. order: a permutation of the learned columns
    (compute_spectrum_evd's sort=True order); learned column order[i] is matched with ground-truth state i.

    For each level [s, e) that has learned columns, with Gb = gram[s:e, s:e] (the WHOLE level), cols = order[s:min(e, L)]
    (k' of them), Cb = cross[s:e, cols], Sb = cov[cols, cols]:

      subspace_distance   1 - tr(Sb^-1 Cb^T Gb^-1 Cb) / k'. A complete level: linalg.subspace_distance of the two (n, k)
                          blocks. A partial last level: the distance of the learned span from the level's span.
      angle               per ground-truth function of a COMPLETE level, arccos sqrt((Cb Sb^-1 Cb^T)_ii / Gb_ii): between
                          psi_i and its projection onto the learned span of its level, the projection linalg.rotate
                          builds. NaN for the functions of a partial level.
      rotation            per complete level Q = U V^T of the SVD of Sb^-1/2 Cb^T Gb^-1/2: linalg.procrustes on the
                          symmetrically orthonormalised blocks Phi_hat, Psi_hat (None for a partial level)
      procrustes_residual ||Phi_hat Q - Psi_hat||_F^2 / k = 2 - 2 sum(singular values) / k (NaN for a partial level)
      gram_defect         max |Gb - I|: what the box and the grid lose of the level
      levels              (s, e, k') per level
    """
    gram, cross, cov = (np.asarray(a, dtype=np.float64) for a in (gram, cross, cov))
    Lg, L = cross.shape
    if gram.shape != (Lg, Lg) or cov.shape != (L, L):
        raise ValueError("gram (Lg, Lg), cross (Lg, L), cov (L, L)")
    deg = [int(d) for d in degeneracy]
    if deg[0] != 0 or deg[-1] != Lg or any(b <= a for a, b in zip(deg, deg[1:])):
        raise ValueError("degeneracy: increasing level boundaries from 0 to Lg")
    order = np.arange(L) if order is None else np.asarray(order, dtype=np.int64)
    if sorted(order.tolist()) != list(range(L)):
        raise ValueError("order: a permutation of the L learned columns")
    dist: List[float] = []
    resid: List[float] = []
    defect: List[float] = []
    rot: list = []
    levels: List[Tuple[int, int, int]] = []
    angle = np.full(Lg, np.nan)
    for s, e in zip(deg[:-1], deg[1:]):
        if s >= L:
            break
        cols = order[s:min(e, L)]
        k = len(cols)
        Gb, Cb, Sb = gram[s:e, s:e], cross[s:e][:, cols], cov[np.ix_(cols, cols)]
        GiC = np.linalg.solve(Gb, Cb)             # Gb^-1 Cb      (e - s, k')
        CSi = np.linalg.solve(Sb, Cb.T).T         # Cb Sb^-1      (e - s, k')
        dist.append(1.0 - float(np.sum(CSi * GiC)) / k)
        defect.append(float(np.max(np.abs(Gb - np.eye(e - s)))))
        levels.append((s, e, k))
        if k < e - s:
            rot.append(None)
            resid.append(float("nan"))
            continue
        cos2 = np.sum(CSi * Cb, axis=1) / np.diag(Gb)
        angle[s:e] = np.arccos(np.sqrt(np.clip(cos2, 0.0, 1.0)))
        U, sv, Vt = np.linalg.svd(_inv_sqrt(Sb) @ Cb.T @ _inv_sqrt(Gb))
        rot.append(U @ Vt)
        resid.append(2.0 - 2.0 * float(sv.sum()) / k)
    return dict(subspace_distance=np.array(dist), angle=angle[:levels[-1][1]], rotation=rot,
                procrustes_residual=np.array(resid), gram_defect=np.array(defect), levels=levels)


class Accumulator:
    """The three float64 device accumulators of one grid pass and the metrics from them."""

    def __init__(self, ground_truth, L: int, device):
        import torch
        self.table = table_of(ground_truth, L)  # (2-D or 3-D: the table's type picks the entry point in add)
        Lg = self.table.Lg
        self.gram = torch.zeros((Lg, Lg), dtype=torch.float64, device=device)
        self.cross = torch.zeros((Lg, L), dtype=torch.float64, device=device)
        self.cov = torch.zeros((L, L), dtype=torch.float64, device=device)
        self.n = 0

    def add(self, f, x, sigma: float, use_importance: bool, lim: float) -> None:
        from . import hip_ops as H
        t = self.table
        if x.dim() != 2 or x.shape[1] != t.ndim:
            raise NsvdError(f"eigenfunction accuracy: a {t.ndim}-D ground truth table on points of shape "
                            f"{tuple(x.shape)}")
        accumulate = H.eigfunc3_accumulate if t.ndim == 3 else H.eigfunc_accumulate
        accumulate(t.kind, t.param, t.qnums, f, x, sigma, use_importance, lim, self.gram, self.cross, self.cov)
        self.n += int(f.shape[0])

    def matrices(self):
        """gram, cross, cov divided by n, numpy float64"""
        return tuple((m / self.n).cpu().numpy() for m in (self.gram, self.cross, self.cov))

    def metrics(self, order=None) -> dict:
        gram, cross, cov = self.matrices()
        out = eigenfunction_metrics(gram, cross, cov, self.table.degeneracy, order)
        out.update(gram=gram, cross=cross, cov=cov, qnums=self.table.qnums, n=self.n)
        return out
