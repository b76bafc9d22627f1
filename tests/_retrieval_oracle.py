"""float64 restatement of the retrieval evaluation (reference examples/cdk/sketchy/retrieve.py) that the HIP entry
point nsvd_retrieval_eval is tested against: scores, a STABLE descending argsort (ties by ascending gallery index),
relevances, P@K and the three average precisions written from their definitions (per-query loops over the relevant
ranks); the fixture recorded from the reference proves that they are the reference's numbers."""
import numpy as np


def scores(zq, zg, metric="inner_product"):
    zq, zg = np.asarray(zq, dtype=np.float64), np.asarray(zg, dtype=np.float64)
    s = zq @ zg.T
    if metric == "euclidean":
        s = s - 0.5 * (zg * zg).sum(axis=1)[np.newaxis, :]  # the order of ascending |x - y|^2
    elif metric != "inner_product":
        raise NotImplementedError(metric)
    return s


def ranking(zq, zg, metric="inner_product"):
    return np.argsort(-scores(zq, zg, metric), axis=1, kind="stable")


def relevances(idxs, q_cls, g_cls):
    return np.asarray(g_cls)[idxs] == np.asarray(q_cls)[:, np.newaxis]


def precisions_at_k(rel):
    return rel.mean(axis=1)


def average_precisions(rel, n_relevant_items, ver):
    """The three average precisions of a (n_queries, K) relevance matrix, one query at a time from their definitions.
    With r_1 < ... < r_R the 1-based ranks of the relevant entries of a row and p_m = m / r_m the precision at the m-th:
      ver 1: mean over m of max_{m' >= m} p_m'   (interpolated precision; R = 0 -> NaN)
      ver 2: sum_m p_m / min(K, n_relevant_items)
      ver 3: integer or float matrix: mean over m of p_m; BOOLEAN matrix: mean over m of 1 / r_m  (R = 0 -> NaN)
    The boolean form of ver 3 is what the reference returns for such a matrix (its running count stays boolean there);
    tests/golden/retrieval.npz holds the reference's numbers for both dtypes and test_retrieval_oracle.py compares.
    nsvd_retrieval_eval implements the integer form, so evaluate() below passes integers."""
    rel = np.asarray(rel)
    boolean = rel.dtype == np.bool_
    n_queries, K = rel.shape
    cap = np.minimum(K, np.broadcast_to(np.asarray(n_relevant_items), (n_queries,)))
    out = np.full(n_queries, np.nan)
    for i in range(n_queries):
        ranks = np.flatnonzero(rel[i]) + 1.0           # r_1 < ... < r_R
        R = ranks.size
        p = np.arange(1, R + 1) / ranks                # p_m
        if ver == 1:
            suffix_max = p.copy()
            for m in range(R - 2, -1, -1):
                suffix_max[m] = max(suffix_max[m], suffix_max[m + 1])
            total, denom = suffix_max.sum(), R
        elif ver == 2:
            total, denom = p.sum(), cap[i]
        elif ver == 3:
            total, denom = ((1.0 / ranks).sum() if boolean else p.sum()), R
        else:
            raise ValueError(ver)
        if denom != 0:
            out[i] = total / denom
        elif total != 0:
            out[i] = np.inf                            # (x / 0; 0 / 0 stays NaN)
    return out


def evaluate(zq, zg, q_cls, g_cls, n_relevant_items, metric, K):
    """everything nsvd_retrieval_eval returns, in float64"""
    order = ranking(zq, zg, metric)
    rel = relevances(order, q_cls, g_cls)
    rel_int = rel.astype(np.int64)
    return {"topk_idx": order[:, :K], "topk_rel": rel[:, :K], "prec_at_k": precisions_at_k(rel[:, :K]),
            "avg_prec": np.stack([average_precisions(rel_int, np.asarray(n_relevant_items), v) for v in (1, 2, 3)]),
            "n_relevant_found": rel.sum(axis=1)}
