"""nsvd_retrieval_eval and the Python retrieval surface on the GPU against tests/_retrieval_oracle.py (float64).

The parity cases have EXACT inputs: embeddings on the grid {-16..16} / 8. For d <= 512 every product (multiples of
1/64, at most 4) and every partial sum (multiples of 1/64 below 2048 = 2^11: 17 bits) is exactly representable in
float32 in any summation order, and so is the Euclidean key x.y - |y|^2 / 2 (multiples of 1/128). The device's keys
therefore EQUAL the float64 keys, ties included, and topk_idx, topk_rel, n_relevant_found and prec_at_k must equal the
oracle's with no tolerance. avg_prec (float64 on the device, as in the oracle): 1e-6 absolute, NaN positions equal.
ver 2 divides by min(Ng, n_relevant_items) with the reference's count among the QUERIES, so it is not bounded by 1
(~24 in the widest case here) - the reason the entry point returns float64 rather than float32."""
import os

import numpy as np
import pytest
import torch

from tests import _retrieval_oracle as RO

pytestmark = pytest.mark.gpu

H = None
R = None
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retrieval.npz")
METRICS = {"inner_product": 0, "euclidean": 1}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H, R
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import hip_ops, retrieval
    H, R = hip_ops, retrieval
    yield


def grid(rng, shape, lo=-16, hi=16):
    return (rng.integers(lo, hi + 1, size=shape) / 8.0).astype(np.float32)


def run_device(zq, zg, q_cls, g_cls, nri, metric, K, **kw):
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)  # noqa: E731
    zq = zq if isinstance(zq, torch.Tensor) else t(zq, torch.float32)
    zg = zg if isinstance(zg, torch.Tensor) else t(zg, torch.float32)
    res = H.retrieval_eval(zq, zg, t(q_cls, torch.int32), t(g_cls, torch.int32), t(nri, torch.int32), METRICS[metric],
                           K, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def check_exact(got, want, K, what=""):
    print(f"{what}: topk_idx mismatches {int((got['topk_idx'] != want['topk_idx']).sum())}, "
          f"topk_rel mismatches {int((got['topk_rel'] != want['topk_rel']).sum())}, "
          f"max |avg_prec diff| {np.nanmax(np.abs(got['avg_prec'] - want['avg_prec']), initial=0.0):.3e}")
    assert np.array_equal(got["topk_idx"], want["topk_idx"]), what
    assert np.array_equal(got["topk_rel"], want["topk_rel"]), what
    assert np.array_equal(got["n_relevant_found"], want["n_relevant_found"]), what
    assert np.array_equal(got["prec_at_k"], want["prec_at_k"].astype(np.float32)), what
    assert np.array_equal(got["hits_at_k"], want["topk_rel"].sum(axis=1)), what
    assert np.array_equal(np.isnan(got["avg_prec"]), np.isnan(want["avg_prec"])), what
    ok = ~np.isnan(want["avg_prec"])
    assert np.all(np.abs(got["avg_prec"][ok] - want["avg_prec"][ok]) <= 1e-6), what


def parity(zq, zg, q_cls, g_cls, nri, metric, K, what=""):
    want = RO.evaluate(zq, zg, q_cls, g_cls, nri, metric, K)
    check_exact(run_device(zq, zg, q_cls, g_cls, nri, metric, K), want, K, what)


def labels(rng, Nq, Ng, ncls):
    q_cls = rng.integers(0, ncls, size=Nq).astype(np.int32)
    g_cls = rng.integers(0, ncls, size=Ng).astype(np.int32)
    nri = np.bincount(q_cls, minlength=ncls)[q_cls].astype(np.int32)  # the reference's count: among the queries
    return q_cls, g_cls, nri


@pytest.mark.parametrize("metric", ["inner_product", "euclidean"])
@pytest.mark.parametrize("Nq,Ng,d,K", [(1, 1, 1, 1), (33, 257, 3, 100), (129, 1023, 65, 100), (64, 1025, 64, 1),
                                       (37, 4097, 512, 2048)])
def test_tile_edges(Nq, Ng, d, K, metric):
    rng = np.random.default_rng(Nq + Ng)
    q_cls, g_cls, nri = labels(rng, Nq, Ng, 5)
    parity(grid(rng, (Nq, d)), grid(rng, (Ng, d)), q_cls, g_cls, nri, metric, K, f"{(Nq, Ng, d, K)} {metric}")


@pytest.mark.parametrize("metric", ["inner_product", "euclidean"])
@pytest.mark.parametrize("col0,d", [(0, 1), (1, 2), (511, 1), (509, 3), (64, 448)])
def test_column_windows(col0, d, metric):
    """a truncation is the window (z + col0, ld = 512, d): odd offsets, d = 1, no copy"""
    rng = np.random.default_rng(col0)
    Nq, Ng, K = 40, 300, 50
    fq, fg = grid(rng, (Nq, 512)), grid(rng, (Ng, 512))
    q_cls, g_cls, nri = labels(rng, Nq, Ng, 4)
    tq, tg = torch.from_numpy(fq).to(DEV), torch.from_numpy(fg).to(DEV)
    wq, wg = tq[:, col0:col0 + d], tg[:, col0:col0 + d]
    assert wq.data_ptr() == tq.data_ptr() + 4 * col0 and wq.stride(0) == 512
    want = RO.evaluate(fq[:, col0:col0 + d], fg[:, col0:col0 + d], q_cls, g_cls, nri, metric, K)
    check_exact(run_device(wq, wg, q_cls, g_cls, nri, metric, K), want, K, f"window {(col0, d)} {metric}")


@pytest.mark.parametrize("metric", ["inner_product", "euclidean"])
@pytest.mark.parametrize("kind", ["ternary", "zeros"])
def test_massive_ties_go_to_the_lower_index(kind, metric):
    rng = np.random.default_rng(3)
    Nq, Ng, d, K = 20, 700, 3, 64
    if kind == "ternary":
        zq = rng.integers(-1, 2, size=(Nq, d)).astype(np.float32)
        zg = rng.integers(-1, 2, size=(Ng, d)).astype(np.float32)
    else:
        zq, zg = np.zeros((Nq, d), np.float32), np.zeros((Ng, d), np.float32)
    q_cls, g_cls, nri = labels(rng, Nq, Ng, 3)
    want = RO.evaluate(zq, zg, q_cls, g_cls, nri, metric, K)
    if kind == "zeros":
        assert np.array_equal(want["topk_idx"], np.tile(np.arange(K), (Nq, 1)))
    check_exact(run_device(zq, zg, q_cls, g_cls, nri, metric, K), want, K, f"ties {kind} {metric}")


@pytest.mark.parametrize("metric", ["inner_product", "euclidean"])
@pytest.mark.parametrize("kind", ["one_class", "absent_class", "K_above_R"])
def test_class_distributions(kind, metric):
    """R = Ng; R = 0 (ver 1 and 3 NaN, ver 2 zero); fewer relevant rows than K"""
    rng = np.random.default_rng(11)
    Nq, Ng, d, K = 17, 1500, 16, 100
    zq, zg = grid(rng, (Nq, d)), grid(rng, (Ng, d))
    if kind == "one_class":
        q_cls, g_cls = np.zeros(Nq, np.int32), np.zeros(Ng, np.int32)
    elif kind == "absent_class":
        q_cls, g_cls = rng.integers(0, 4, size=Nq).astype(np.int32), rng.integers(0, 3, size=Ng).astype(np.int32)
        q_cls[:3] = 3
    else:
        q_cls = rng.integers(0, 3, size=Nq).astype(np.int32)
        g_cls = rng.integers(1, 3, size=Ng).astype(np.int32)
        g_cls[rng.choice(Ng, size=7, replace=False)] = 0  # class 0: R = 7 < K
        q_cls[:4] = 0
    nri = np.bincount(q_cls, minlength=4)[q_cls].astype(np.int32)
    want = RO.evaluate(zq, zg, q_cls, g_cls, nri, metric, K)
    got = run_device(zq, zg, q_cls, g_cls, nri, metric, K)
    check_exact(got, want, K, f"{kind} {metric}")
    if kind == "one_class":
        assert np.all(got["n_relevant_found"] == Ng) and np.all(got["prec_at_k"] == 1.0)
        assert np.allclose(got["avg_prec"][[0, 2]], 1.0, atol=1e-6)
    if kind == "absent_class":
        assert np.all(np.isnan(got["avg_prec"][0, :3])) and np.all(np.isnan(got["avg_prec"][2, :3]))
        assert np.all(got["avg_prec"][1, :3] == 0.0) and np.all(got["n_relevant_found"][:3] == 0)
    if kind == "K_above_R":
        assert np.all(got["n_relevant_found"][:4] == 7) and np.all(got["prec_at_k"][:4] <= np.float32(7 / K))


@pytest.fixture(scope="module")
def sketchy_like():
    rng = np.random.default_rng(2024)
    Nq, Ng, d = 512, 10453, 512
    zq, zg = grid(rng, (Nq, d)), grid(rng, (Ng, d))
    q_cls, g_cls, nri = labels(rng, Nq, Ng, 25)
    return zq, zg, q_cls, g_cls, nri


@pytest.mark.parametrize("metric", ["inner_product", "euclidean"])
def test_sketchy_like_gallery(sketchy_like, metric):
    zq, zg, q_cls, g_cls, nri = sketchy_like
    parity(zq, zg, q_cls, g_cls, nri, metric, 100, f"sketchy-like {metric}")


def test_large_gallery_or_refusal():
    """Ng = 70 000: exact parity inside the library's gallery limit, NSVD_EUNSUPPORTED through NsvdError beyond it"""
    from neural_svd_amd._lib import NsvdError
    rng = np.random.default_rng(5)
    Nq, Ng, d, K = 8, 70000, 8, 100
    zq, zg = grid(rng, (Nq, d)), grid(rng, (Ng, d))
    q_cls, g_cls, nri = labels(rng, Nq, Ng, 25)
    if Ng <= H.retrieval_max_gallery():
        parity(zq, zg, q_cls, g_cls, nri, "inner_product", K, "Ng = 70000")
    else:
        with pytest.raises(NsvdError, match="NSVD_EUNSUPPORTED"):
            run_device(zq, zg, q_cls, g_cls, nri, "inner_product", K)


def test_reference_euclidean_indices():
    """the reference's own get_retrievals(package='sklearn', metric='euclidean') ranking (tests/golden/retrieval.npz:
    every query's distances are more than 1e-3 apart, so that ranking is unique and float32 keys reproduce it)"""
    z = np.load(GOLDEN)
    rel, idx = R.SketchyRetrieval.get_retrievals(z["zq"], z["zg"], z["q_names"], z["g_names"], package="sklearn",
                                                 metric="euclidean", device=DEV)
    assert np.array_equal(idx, z["euclid_idx"])
    assert np.array_equal(rel, z["euclid_rel"])


def test_get_retrievals_beyond_the_kernel_cap():
    """K = None on a gallery larger than the kernel's K cap takes the documented torch.sort(stable=True) route: the
    same ranking rule, checked on exact (grid) inputs with ties"""
    rng = np.random.default_rng(13)
    Nq, Ng, d = 24, 2100, 8
    zq, zg = grid(rng, (Nq, d), -4, 4), grid(rng, (Ng, d), -4, 4)
    q_cls, g_cls, _ = labels(rng, Nq, Ng, 5)
    for metric in ("inner_product", "euclidean"):
        order = RO.ranking(zq, zg, metric)
        rel, idx = R.SketchyRetrieval.get_retrievals(zq, zg, q_cls, g_cls, metric=metric, device=DEV)
        assert idx.shape == (Nq, Ng) and np.array_equal(idx, order)
        assert np.array_equal(rel, RO.relevances(order, q_cls, g_cls))
        rel, idx = R.SketchyRetrieval.get_retrievals(torch.from_numpy(zq).to(DEV), torch.from_numpy(zg), q_cls, g_cls,
                                                     K=2048, metric=metric, device=DEV)
        assert np.array_equal(idx, order[:, :2048])


def _torch_binding():
    """the tensor-level binding (csrc/torch_binding.cpp), which build() compiles next to the library"""
    import importlib.util
    import subprocess
    from neural_svd_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "neural_svd_amd", "_nsvd_torch.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(root, "neural_svd_amd", "csrc"), "torch_binding"])
    _lib.load()
    spec = importlib.util.spec_from_file_location("_nsvd_torch", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tensor_binding_parity():
    """retrieval_eval through the tensor binding: leading dimensions from the strides of an unaligned column window,
    a one-row matrix, and absent (None) outputs - against the oracle, exactly"""
    tb = _torch_binding()
    assert tb.retrieval_max_gallery() == H.retrieval_max_gallery()
    assert tb.retrieval_limits() == [H.retrieval_max_k(), H.retrieval_max_d()]
    rng = np.random.default_rng(17)
    for Nq, Ng, col0, d, K, metric in ((40, 300, 509, 3, 50, "euclidean"), (1, 130, 1, 64, 130, "inner_product")):
        fq, fg = grid(rng, (Nq, 512)), grid(rng, (Ng, 512))
        q_cls, g_cls, nri = labels(rng, Nq, Ng, 4)
        want = RO.evaluate(fq[:, col0:col0 + d], fg[:, col0:col0 + d], q_cls, g_cls, nri, metric, K)
        wq = torch.from_numpy(fq).to(DEV)[:, col0:col0 + d]
        wg = torch.from_numpy(fg).to(DEV)[:, col0:col0 + d]
        dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        ws = torch.empty(tb.retrieval_workspace_bytes(Nq, Ng, d, K), dtype=torch.uint8, device=DEV)
        out = {"topk_idx": torch.empty((Nq, K), dtype=torch.int32, device=DEV),
               "topk_rel": torch.empty((Nq, K), dtype=torch.bool, device=DEV),
               "prec_at_k": torch.empty(Nq, dtype=torch.float32, device=DEV),
               "hits_at_k": torch.empty(Nq, dtype=torch.int32, device=DEV),
               "avg_prec": torch.empty((3, Nq), dtype=torch.float64, device=DEV),
               "n_relevant_found": torch.empty(Nq, dtype=torch.int32, device=DEV)}
        tb.retrieval_eval(wq, wg, dv(q_cls), dv(g_cls), dv(nri), METRICS[metric], K, out["topk_idx"], out["topk_rel"],
                          out["prec_at_k"], out["hits_at_k"], out["avg_prec"], out["n_relevant_found"], ws)
        torch.cuda.synchronize()
        check_exact({k: v.cpu().numpy() for k, v in out.items()}, want, K, f"tensor binding {(Nq, Ng, col0, d, K)}")
        # every optional output absent: P@K alone
        prec = torch.zeros(Nq, dtype=torch.float32, device=DEV)
        tb.retrieval_eval(wq, wg, dv(q_cls), dv(g_cls), None, METRICS[metric], K, None, None, prec, None, None, None, ws)
        torch.cuda.synchronize()
        assert np.array_equal(prec.cpu().numpy(), want["prec_at_k"].astype(np.float32))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        tb.retrieval_eval(torch.zeros(2, 3), wg, dv(q_cls), dv(g_cls), None, 0, 1, None, None, prec, None, None, None, ws)


def test_real_valued_embeddings_are_ranked_validly():
    """standard normal embeddings: exact order cannot be demanded, validity within the float32 rounding bound
    delta_ij = 2 (d + 2) 2^-24 (sum_k |x_ik y_jk| + |y_j|^2 / 2) (the last term for Euclidean only)"""
    rng = np.random.default_rng(9)
    Nq, Ng, d, K = 64, 2000, 128, 100
    zq = rng.standard_normal((Nq, d)).astype(np.float32)
    zg = rng.standard_normal((Ng, d)).astype(np.float32)
    q_cls, g_cls, nri = labels(rng, Nq, Ng, 10)
    for metric in ("inner_product", "euclidean"):
        got = run_device(zq, zg, q_cls, g_cls, nri, metric, K)
        s = RO.scores(zq, zg, metric)
        mag = np.abs(zq.astype(np.float64)) @ np.abs(zg.astype(np.float64)).T
        if metric == "euclidean":
            mag = mag + 0.5 * (zg.astype(np.float64) ** 2).sum(1)[None, :]
        delta = 2 * (d + 2) * 2.0 ** -24 * mag
        idx = got["topk_idx"].astype(np.int64)
        assert all(len(set(r.tolist())) == K for r in idx)
        sk, dk = np.take_along_axis(s, idx, axis=1), np.take_along_axis(delta, idx, axis=1)
        worst = (sk[:, 1:] - sk[:, :-1] - dk[:, 1:] - dk[:, :-1]).max()
        print(f"{metric}: worst inversion minus bound {worst:.3e}")
        assert worst <= 0
        left = np.ones((Nq, Ng), bool)
        np.put_along_axis(left, idx, False, axis=1)
        beat = np.where(left, s - delta, -np.inf).max(axis=1) - (sk[:, -1] + dk[:, -1])
        print(f"{metric}: best row left out minus K-th minus bound {beat.max():.3e}")
        assert beat.max() <= 0
        assert np.array_equal(got["topk_rel"], g_cls[idx] == q_cls[:, None])


def test_repeatable_and_graph_capturable():
    rng = np.random.default_rng(21)
    Nq, Ng, d, K = 96, 3000, 96, 100
    zq = torch.from_numpy(rng.standard_normal((Nq, d)).astype(np.float32)).to(DEV)
    zg = torch.from_numpy(rng.standard_normal((Ng, d)).astype(np.float32)).to(DEV)
    q_cls, g_cls, nri = [torch.from_numpy(a).to(DEV) for a in labels(rng, Nq, Ng, 7)]
    a = H.retrieval_eval(zq, zg, q_cls, g_cls, nri, 1, K)
    b = H.retrieval_eval(zq, zg, q_cls, g_cls, nri, 1, K)
    torch.cuda.synchronize()
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    ws = torch.empty(H.retrieval_workspace_bytes(Nq, Ng, d, K), dtype=torch.uint8, device=DEV)
    H.retrieval_eval(zq, zg, q_cls, g_cls, nri, 1, K, ws=ws)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = H.retrieval_eval(zq, zg, q_cls, g_cls, nri, 1, K, ws=ws)
    for v in c.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in a:
        assert a[k].cpu().numpy().tobytes() == c[k].cpu().numpy().tobytes(), k


class _Loader:
    def __init__(self, rng, Nq, Ng, d_in, ncls, absent):
        names = np.array([f"cls_{i:02d}" for i in range(ncls)])
        self.batch_size = 128
        self.sketch_features = rng.standard_normal((Nq, d_in)).astype(np.float32)
        self.photo_features = rng.standard_normal((Ng, d_in)).astype(np.float32)
        self.sketch_classes = names[rng.integers(0, ncls, size=Nq)]
        self.photo_classes = names[rng.integers(0, ncls - int(absent), size=Ng)]  # absent: the last class has no photo


def _snap(z):
    """embeddings snapped to the exact grid (multiples of 1/8 in [-2, 2])"""
    return torch.clamp(torch.round(z * 8.0), -16, 16) / 8.0


@pytest.fixture(scope="module")
def towers_and_loader():
    from neural_svd_amd.cdk import get_mlp
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    loaders = {absent: _Loader(rng, 300, 500, 24, 6, absent) for absent in (True, False)}
    towers = [get_mlp([24, 32, 8]).to(DEV).eval() for _ in range(2)]
    with torch.no_grad():
        for tw in towers:  # running statistics that are not the identity
            tw[1].running_mean.normal_(0, 0.1)
            tw[4].running_var.uniform_(0.5, 1.5)
    fx = lambda x: _snap(towers[0](x))  # noqa: E731
    fy = lambda y: _snap(towers[1](y))  # noqa: E731
    return loaders, fx, fy


def _oracle_for(loader, zx, zy, metric, K):
    names = sorted(set(loader.sketch_classes.tolist()) | set(loader.photo_classes.tolist()))
    ids = {n: i for i, n in enumerate(names)}
    q = np.array([ids[n] for n in loader.sketch_classes.tolist()])
    g = np.array([ids[n] for n in loader.photo_classes.tolist()])
    nri = np.bincount(q, minlength=len(names))[q]  # among the SKETCHES
    return RO.evaluate(zx, zy, q, g, nri, metric, K)


@pytest.mark.parametrize("metric", ["inner_product", "euclidean"])
def test_sketchy_retrieval_evaluate(towers_and_loader, metric):
    loaders, fx, fy = towers_and_loader
    loader = loaders[True]
    sr = R.SketchyRetrieval(loader, n_retrievals=100, metric=metric, device=DEV)
    zx, zy = sr.embed(fx, fy)
    want = _oracle_for(loader, zx.cpu().numpy(), zy.cpu().numpy(), metric, 100)
    p, ap = sr.evaluate(fx, fy, epoch=1)
    assert isinstance(ap, np.ndarray) and ap.shape == () and ap == 0.0
    assert p.dtype == np.float64 and np.array_equal(p, want["prec_at_k"])
    for ver in (1, 2, 3):
        p, ap = sr.evaluate(fx, fy, epoch=1, ap_ver=ver, return_map_all=True, tag="test")
        assert np.array_equal(p, want["prec_at_k"])
        assert np.array_equal(np.isnan(ap), np.isnan(want["avg_prec"][ver - 1]))
        assert np.nanmax(np.abs(ap - want["avg_prec"][ver - 1])) <= 1e-6
    with pytest.raises(NotImplementedError, match="sklearn"):
        R.SketchyRetrieval(loader, metric="cosine", device=DEV).evaluate(fx, fy, epoch=1)


def test_evaluate_truncations(towers_and_loader):
    loaders, fx, fy = towers_and_loader
    loader = loaders[False]
    dims = [-4, -1, 1, 2, 8]
    perm = torch.tensor([3, 1, 4, 0, 7, 6, 2, 5])
    sr = R.SketchyRetrieval(loader, n_retrievals=100, device=DEV)
    zx, zy = [z.cpu().numpy() for z in sr.embed(fx, fy)]
    for pm in (None, perm):
        got_dims, got_p, got_ap = R.evaluate_truncations((fx, fy), loader, [8, 1, -1, 2, -4], perm=pm, device=DEV)
        assert got_dims.tolist() == dims
        order = np.arange(8) if pm is None else pm.numpy()
        for i, t in enumerate(dims):
            cols = order[:t] if t > 0 else order[t:]
            want = _oracle_for(loader, zx[:, cols], zy[:, cols], "inner_product", 100)
            assert got_p[i] == want["prec_at_k"].mean()
            assert np.isfinite(got_ap[i]) and abs(got_ap[i] - np.mean(want["avg_prec"][0])) <= 1e-6
