"""CPU checks of the retrieval evaluation: the float64 oracle (tests/_retrieval_oracle.py) and the package's numpy
metric functions against what the reference's SketchyRetrieval recorded (tests/golden/retrieval.npz, written by
tests/golden/make_golden_retrieval.py), compute_spectrum_svd against a numpy restatement, and the host-side argument
checks of the HIP wrapper."""
import os

import numpy as np
import pytest
import torch

from tests import _retrieval_oracle as RO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retrieval.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def same(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    assert np.all(np.abs(a[ok] - b[ok]) <= tol), np.abs(a[ok] - b[ok]).max()


def test_fixture_has_the_edge_rows(z):
    assert not z["rel"][0].any() and z["rel"][1].all() and z["rel"][2].sum() == 1 and z["rel"][2, -1]
    assert np.isnan(z["avg_prec_v1"][0]) and np.isnan(z["avg_prec_v3"][0]) and z["avg_prec_v2"][0] == 0.0
    assert float(z["euclid_min_gap"]) > 1e-3


def test_oracle_reproduces_the_reference(z):
    rel, K = z["rel"], int(z["K"])
    same(RO.precisions_at_k(rel[:, :K]), z["prec_at_k"])
    for ver in (1, 2, 3):
        same(RO.average_precisions(rel.astype(np.int64), z["n_relevant_items"], ver), z[f"avg_prec_v{ver}"])
    for ver in (1, 2):  # the same on the boolean matrix; ver 3 is dtype-dependent in the reference (avg_prec_v3_bool)
        same(RO.average_precisions(rel, z["n_relevant_items"], ver), z[f"avg_prec_v{ver}"])
    same(RO.average_precisions(rel, z["n_relevant_items"], 3), z["avg_prec_v3_bool"])
    order = RO.ranking(z["zq"], z["zg"], "euclidean")
    assert np.array_equal(order, z["euclid_idx"])
    assert np.array_equal(RO.relevances(order, z["q_names"], z["g_names"]), z["euclid_rel"])


def test_package_metric_functions_reproduce_the_reference(z):
    from neural_svd_amd.retrieval import SketchyRetrieval
    rel, K = z["rel"], int(z["K"])
    same(SketchyRetrieval.compute_precisions_at_k(rel[:, :K]), z["prec_at_k"])
    for ver in (1, 2, 3):
        same(SketchyRetrieval.compute_average_precisions(rel.astype(np.int64), z["n_relevant_items"], ver=ver),
             z[f"avg_prec_v{ver}"])
    for ver in (1, 2):
        same(SketchyRetrieval.compute_average_precisions(rel, z["n_relevant_items"], ver=ver), z[f"avg_prec_v{ver}"])
    same(SketchyRetrieval.compute_average_precisions(rel, z["n_relevant_items"], ver=3), z["avg_prec_v3_bool"])
    # on the reference's own retrievals too (K = the whole gallery)
    nri = np.arange(1, rel.shape[0] + 1)
    for ver in (1, 2, 3):
        for cast in (np.bool_, np.int64):
            same(SketchyRetrieval.compute_average_precisions(z["euclid_rel"].astype(cast), nri, ver=ver),
                 RO.average_precisions(z["euclid_rel"].astype(cast), nri, ver))


def test_constructor_maps_class_names_and_counts_among_the_sketches(z):
    import types
    from neural_svd_amd.retrieval import SketchyRetrieval
    loader = types.SimpleNamespace(batch_size=8, sketch_features=z["zq"], photo_features=z["zg"],
                                   sketch_classes=z["q_names"], photo_classes=z["g_names"])
    sr = SketchyRetrieval(loader, device="cpu")
    assert sr.sketch_ids.dtype == np.int32 and sr.photo_ids.dtype == np.int32
    assert np.array_equal(sr.sketch_ids[:, None] == sr.photo_ids[None, :], z["q_names"][:, None] == z["g_names"][None, :])
    counts = {n: int((z["q_names"] == n).sum()) for n in set(z["q_names"].tolist())}
    assert sr.n_classes_items.tolist() == [counts[n] for n in z["q_names"].tolist()]
    with pytest.raises(NotImplementedError, match="sklearn"):
        SketchyRetrieval.get_retrievals(z["zq"], z["zg"], z["q_names"], z["g_names"], metric="cosine")


@pytest.mark.parametrize("first_const", [False, True])
@pytest.mark.parametrize("sort", [False, True])
def test_compute_spectrum_svd(first_const, sort):
    from neural_svd_amd.spectrum import compute_spectrum_svd
    g = torch.Generator().manual_seed(0)
    A, B = torch.randn(6, 5, generator=g), torch.randn(6, 5, generator=g)
    scale = torch.tensor([0.3, 2.0, 1.0, 0.1, 1.5])
    model = lambda x, y: (torch.tanh(x @ A) * scale, torch.sin(y @ B) * scale)  # noqa: E731
    loader = [(torch.randn(n, 6, generator=g), torch.randn(n, 6, generator=g), torch.zeros(n)) for n in (7, 4, 9)]
    spec, ox, oy = compute_spectrum_svd(model, loader, device="cpu", sort=sort, set_first_mode_const=first_const)
    f = np.concatenate([model(x, y)[0].double().numpy() for x, y, _ in loader])
    h = np.concatenate([model(x, y)[1].double().numpy() for x, y, _ in loader])
    if first_const:
        f, h = np.pad(f, ((0, 0), (1, 0)), constant_values=1.0), np.pad(h, ((0, 0), (1, 0)), constant_values=1.0)
    mx, my = f.T @ f / len(f), h.T @ h / len(h)
    want = np.sqrt(np.diag(mx) * np.diag(my))
    wx = mx / np.sqrt(np.outer(np.diag(mx), np.diag(mx)))
    wy = my / np.sqrt(np.outer(np.diag(my), np.diag(my)))
    if sort:
        idx = np.argsort(want)[::-1]
        want, wx, wy = want[idx], wx[idx][:, idx], wy[idx][:, idx]
        assert np.all(np.diff(spec) <= 0)
    assert spec.shape == (5 + int(first_const),) and spec.dtype == np.float32
    assert np.allclose(spec, want, rtol=1e-6, atol=0) and np.allclose(ox, wx, atol=1e-6) and np.allclose(oy, wy, atol=1e-6)
    with pytest.raises(ValueError):
        compute_spectrum_svd(model, loader)


def test_retrieval_eval_refuses_cpu_tensors():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    zq, zg = torch.zeros(4, 3), torch.zeros(9, 3)
    q, g = torch.zeros(4, dtype=torch.int32), torch.zeros(9, dtype=torch.int32)
    with pytest.raises(NsvdError, match="must live on the GPU"):
        H.retrieval_eval(zq, zg, q, g, q, H.RETR_INNER_PRODUCT, 2)


def test_workspace_query():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    n = H.retrieval_workspace_bytes(12800, 10453, 512, 100)
    assert n > 0
    # bounded by a query chunk: it does not grow with Nq once the chunk is full, and never holds Nq x Ng
    assert H.retrieval_workspace_bytes(10 * 12800, 10453, 512, 100) == n and n < 12800 * 10453 * 4
    assert H.retrieval_max_gallery() >= 65536
    for bad in ((8, 16, 4, 17), (8, 16, 4, 0), (8, 16, 1025, 4), (8, 0, 4, 1), (8, 4096, 4, 2049),
                (8, H.retrieval_max_gallery() + 1, 4, 10)):
        with pytest.raises(NsvdError):
            H.retrieval_workspace_bytes(*bad)
