#!/usr/bin/env python3
"""Generate tests/golden/retrieval.npz by IMPORTING the reference's SketchyRetrieval
(examples/cdk/sketchy/retrieve.py). Runs only where a reference checkout is present; the test-suite never runs it, it
only reads the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_retrieval.py <path to the reference checkout>

`faiss` is registered as an empty stand-in module (retrieve.py imports it at module scope; only the sklearn route is
exercised here). Recorded, arrays only:
  * rel (Nq, Ng) bool relevance matrices (row 0 all false, row 1 all true), n_relevant_items, and the reference's
    compute_precisions_at_k (on the first K columns) and compute_average_precisions(ver = 1, 2, 3) on them as 0 / 1
    integers, plus ver 3 on the boolean matrix (avg_prec_v3_bool: the reference's running count degenerates to a
    logical or there, see below);
  * float32-representable random embeddings zq (24, 8), zg (96, 8) with class names, and the reference's own
    get_retrievals(package='sklearn', metric='euclidean') indices and relevances over the whole gallery.
sklearn leaves the order of tied distances open, so the gallery is drawn until every query's smallest gap between
adjacent squared distances exceeds 1e-3 (float32 accumulation error at this size: ~1e-6; asserted) - the reference's
ranking is then the unique one.
"""
import importlib.util
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NQ, NG, D, K, NCLS = 24, 96, 8, 10, 5
MIN_GAP = 1e-3


def load_reference(ref):
    sys.modules.setdefault("faiss", types.ModuleType("faiss"))
    path = os.path.join(ref, "examples", "cdk", "sketchy", "retrieve.py")
    spec = importlib.util.spec_from_file_location("reference_retrieve", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SketchyRetrieval


def embeddings():
    # (2280 adjacent gaps of mean ~0.2: a whole draw with none below 1e-3 has probability ~e^-11, so the gallery is
    # drawn row by row and a row that lands within the margin of an earlier distance, for any query, is drawn again)
    seed = 0
    rng = np.random.default_rng(seed)
    zq = rng.standard_normal((NQ, D)).astype(np.float32)
    rows, dist = [], np.zeros((NQ, 0))
    while len(rows) < NG:
        y = rng.standard_normal(D).astype(np.float32)
        dy = ((zq.astype(np.float64) - y.astype(np.float64)[None, :]) ** 2).sum(-1)
        if dist.shape[1] and np.abs(dist - dy[:, None]).min() <= 2 * MIN_GAP:
            continue
        rows.append(y)
        dist = np.concatenate([dist, dy[:, None]], axis=1)
    zg = np.stack(rows)
    d2 = ((zq.astype(np.float64)[:, None, :] - zg.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    gap = np.diff(np.sort(d2, axis=1), axis=1).min()
    assert gap > MIN_GAP, gap
    return seed, zq, zg, float(gap)


def main():
    SR = load_reference(sys.argv[1])
    out = {}
    rng = np.random.default_rng(7)
    rel = rng.random((NQ, NG)) < 0.2
    rel[0, :] = False
    rel[1, :] = True
    rel[2, :] = False
    rel[2, NG - 1] = True  # a single relevant row, ranked last
    nri = rng.integers(1, 40, size=NQ)
    out["rel"], out["n_relevant_items"], out["K"] = rel, nri, np.int64(K)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["prec_at_k"] = SR.compute_precisions_at_k(rel[:, :K])
        for ver in (1, 2, 3):
            out[f"avg_prec_v{ver}"] = SR.compute_average_precisions(rel.astype(np.int64), nri, ver=ver)
        # ver 3 is dtype-dependent in the reference: its running count is formed by `+` on a copy of the input, which on
        # a BOOLEAN matrix (what get_retrievals returns) is a logical or - the sum of 1 / r_m instead of m / r_m
        out["avg_prec_v3_bool"] = SR.compute_average_precisions(rel, nri, ver=3)
        for ver in (1, 2):
            assert np.array_equal(SR.compute_average_precisions(rel, nri, ver=ver), out[f"avg_prec_v{ver}"],
                                  equal_nan=True)

    seed, zq, zg, gap = embeddings()
    names = np.array([f"class_{c:02d}" for c in range(NCLS)])
    q_names = names[rng.integers(0, NCLS, size=NQ)]
    g_names = names[rng.integers(0, NCLS - 1, size=NG)]  # the last class has no photo: R = 0 for its sketches
    rels, idxs = SR.get_retrievals(zq, zg, xclss=q_names, yclss=g_names, package="sklearn", metric="euclidean")
    out.update(zq=zq, zg=zg, q_names=q_names, g_names=g_names, euclid_idx=idxs.astype(np.int64), euclid_rel=rels,
               euclid_seed=np.int64(seed), euclid_min_gap=np.float64(gap))
    np.savez_compressed(os.path.join(HERE, "retrieval.npz"), **out)
    print(f"seed {seed}, smallest gap {gap:.3e}; wrote retrieval.npz with {sorted(out)}")


if __name__ == "__main__":
    main()
