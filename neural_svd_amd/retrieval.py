"""Retrieval evaluation of the CDK towers with the reference's interface (examples/cdk/sketchy/retrieve.py:17-201):
``SketchyRetrieval`` (P@K and mAP@all of sketch-to-photo retrieval) and ``evaluate_truncations`` (the closing loop of
examples/cdk/sketchy/main_sketchy.py:325-358 over truncations of the nested embedding).

The exact search (faiss ``IndexFlatIP`` / ``IndexFlatL2`` in the reference), the relevance bookkeeping and the metrics
are ONE HIP call per evaluation, ``nsvd_retrieval_eval`` (include/nsvd.h): embeddings stay on the device, and no
(n_queries, n_gallery) array is ever formed. Ranking rule: descending key, ties by ascending gallery index.
``compute_precisions_at_k`` / ``compute_average_precisions`` are numpy restatements of the reference's formulas for a
caller who already holds a relevance matrix; they need no GPU."""
from __future__ import annotations

import os
import random
from collections import Counter
from shutil import copyfile

import numpy as np
import torch

from . import hip_ops as H

_METRICS = {"inner_product": H.RETR_INNER_PRODUCT, "euclidean": H.RETR_EUCLIDEAN}


def _metric_id(metric):
    if metric == "cosine":
        raise NotImplementedError("metric='cosine': the reference routes it to sklearn's NearestNeighbors and no "
                                  "script uses it; normalise the embeddings and use 'inner_product'")
    if metric not in _METRICS:
        raise NotImplementedError(f"metric={metric!r} (one of {sorted(_METRICS)})")
    return _METRICS[metric]


def _class_ids(*name_arrays):
    """one int32 id per distinct class name over all the arrays (ids follow the sorted names)"""
    names = sorted(set().union(*[set(np.asarray(a).tolist()) for a in name_arrays]))
    table = {n: i for i, n in enumerate(names)}
    return [np.asarray([table[n] for n in np.asarray(a).tolist()], dtype=np.int32) for a in name_arrays]


def _device_matrix(z, device):
    if isinstance(z, torch.Tensor):
        z = z.detach()
        return z.to(device=device if not z.is_cuda else z.device, dtype=torch.float32)
    return torch.as_tensor(np.ascontiguousarray(z), dtype=torch.float32).to(device)


def _embed(model, features, batch_size, device):
    """model(features) in chunks of batch_size; the embeddings stay on the device"""
    out = []
    for lo in range(0, features.shape[0], batch_size):
        chunk = features[lo: lo + batch_size]
        chunk = chunk.to(device) if isinstance(chunk, torch.Tensor) else torch.Tensor(chunk).to(device)
        out.append(model(chunk).detach().float())
    return torch.cat(out, dim=0)


class SketchyRetrieval:
    """retrieve.py's SketchyRetrieval. ``test_loader`` is duck-typed: ``batch_size``, ``sketch_features``,
    ``photo_features`` (numpy), ``sketch_classes``, ``photo_classes`` (numpy arrays of class names); the path
    attributes (``sketch_paths``, ``photo_paths``, ``sketch_idx_per_class``, ``path_sketch``, ``path_photo``) only when
    images are saved. Class names become int32 ids once, here."""

    def __init__(self, test_loader, n_images_to_save=10, n_retrievals=100, metric="inner_product", run_path=None,
                 device=None):
        self.test_loader = test_loader
        self.batch_size = test_loader.batch_size
        self.n_images_to_save = n_images_to_save
        self.n_retrievals = n_retrievals
        self.metric = metric
        self.run_path = run_path
        self.device = torch.device(device if device is not None else "cuda")
        # the reference's quirk, kept: the number of "relevant items" of a query is the size of its class among the
        # SKETCHES (retrieve.py:31-35), not among the photos it retrieves from
        self.n_classes = Counter(np.asarray(test_loader.sketch_classes).tolist())
        self.n_classes_items = np.array([self.n_classes[c] for c in np.asarray(test_loader.sketch_classes).tolist()])
        self.sketch_ids, self.photo_ids = _class_ids(test_loader.sketch_classes, test_loader.photo_classes)
        self._dev = None

    @staticmethod
    def parse_class(path):
        return path.split("/")[-2]

    def _device_labels(self):
        if self._dev is None:
            d = self.device
            self._dev = (torch.from_numpy(self.sketch_ids).to(d), torch.from_numpy(self.photo_ids).to(d),
                         torch.from_numpy(self.n_classes_items.astype(np.int32)).to(d))
        return self._dev

    def embed(self, model_x, model_y):
        """(zxs, zys) on the device: the two towers over the loader's features in chunks of batch_size"""
        with torch.no_grad():
            return (_embed(model_x, self.test_loader.sketch_features, self.batch_size, self.device),
                    _embed(model_y, self.test_loader.photo_features, self.batch_size, self.device))

    def evaluate_embeddings(self, zxs, zys, epoch=0, save_retrieved_images=False, ap_ver=1, tag="",
                            return_map_all=False, verbose=True):
        """evaluate() from embeddings already on the device (any column window of them): one nsvd_retrieval_eval."""
        qc, gc, nri = self._device_labels()
        want_ap = bool(return_map_all or save_retrieved_images)
        K = min(int(self.n_retrievals), zys.shape[0])
        res = H.retrieval_eval(zxs, zys, qc, gc, nri if want_ap else None, _metric_id(self.metric), K,
                               want_topk=bool(save_retrieved_images), want_ap=want_ap)
        precision_Ks = res["hits_at_k"].cpu().numpy().astype(np.float64) / K  # float64, as numpy's mean of K booleans
        if verbose:
            print(f"{tag}\tP@{self.n_retrievals} ({self.metric})\t{precision_Ks.mean():.4f}")
        average_precisions = np.array(0.)
        if want_ap:
            average_precisions = res["avg_prec"][int(ap_ver) - 1].double().cpu().numpy()
            if verbose:
                print(f"{tag}\tmAP ({self.metric})\t{average_precisions.mean():.4f}")
            if save_retrieved_images:
                self.save_retrieved_images(res["topk_idx"].cpu().numpy().astype(np.int64), epoch, tag=tag)
        return precision_Ks, average_precisions

    def evaluate(self, model_x, model_y, epoch, save_retrieved_images=False, ap_ver=1, tag="", return_map_all=False):
        if ap_ver not in (1, 2, 3):
            raise ValueError("ap_ver must be 1, 2 or 3")
        zxs, zys = self.embed(model_x, model_y)
        return self.evaluate_embeddings(zxs, zys, epoch, save_retrieved_images, ap_ver, tag, return_map_all)

    @staticmethod
    def get_retrievals(zxs, zys, xclss, yclss, K=None, package="faiss", metric="euclidean", device=None):
        """(relevances, retrieved_zys_idxs), both (n_queries, K) numpy arrays, K=None: the whole gallery. zxs / zys:
        numpy arrays or tensors (moved to ``device``, default 'cuda', when not already on a GPU). ``package`` is
        accepted and ignored: the search is this library's. Up to K = 2048 (the kernel's cap) the indices come from
        nsvd_retrieval_eval; beyond it from torch.sort(stable=True) on the negated keys of query chunks, the same
        ranking rule (descending key, ties by ascending index) at library-kernel cost."""
        assert package in ["faiss", "sklearn"]
        mid = _metric_id(metric)
        dev = torch.device(device if device is not None else "cuda")
        zq, zg = _device_matrix(zxs, dev), _device_matrix(zys, dev)
        dev = zq.device
        Ng = zg.shape[0]
        K = Ng if K is None else int(K)
        xclss, yclss = np.asarray(xclss), np.asarray(yclss)
        if K <= H.retrieval_max_k():
            xi, yi = _class_ids(xclss, yclss)
            res = H.retrieval_eval(zq, zg, torch.from_numpy(xi).to(dev), torch.from_numpy(yi).to(dev), None, mid, K,
                                   want_topk=True, want_ap=False)
            idxs = res["topk_idx"].cpu().numpy().astype(np.int64)
        else:
            half = 0.5 * (zg * zg).sum(1) if mid == H.RETR_EUCLIDEAN else None
            rows = max(1, (1 << 26) // max(Ng, 1))
            parts = []
            for lo in range(0, zq.shape[0], rows):
                s = zq[lo: lo + rows] @ zg.T
                if half is not None:
                    s = s - half
                parts.append(torch.sort(-s, dim=1, stable=True).indices[:, :K].cpu())
            idxs = torch.cat(parts, dim=0).numpy()
        relevances = (yclss[idxs] == xclss[:, np.newaxis])
        return relevances, idxs

    def save_retrieved_images(self, retrieved_zys_idxs, epoch, tag=""):
        """For every sketch class: one query sketch of the class, picked at random, and its first n_images_to_save
        retrieved photos copied into <run_path>/retrievals/e<epoch>/<tag>_<class>/ as query.jpg, 0.jpg, 1.jpg, ... -
        a photo of another class gets the suffix _f (the layout the reference's script writes)."""
        loader = self.test_loader
        out_root = os.path.join(self.run_path, "retrievals", f"e{epoch:03d}")
        top = np.asarray(retrieved_zys_idxs)[:, :self.n_images_to_save]
        for cls in sorted(set(np.asarray(loader.sketch_classes).tolist())):
            folder = os.path.join(out_root, f"{tag}_{cls}")
            os.makedirs(folder, exist_ok=True)
            q = random.choice(loader.sketch_idx_per_class[cls])
            query_file = os.path.join(loader.path_sketch, loader.sketch_paths[q])
            if not os.path.exists(query_file):
                raise FileNotFoundError(f"query sketch {query_file} is missing")
            copyfile(query_file, os.path.join(folder, "query.jpg"))
            for rank, g in enumerate(top[q]):
                photo = loader.photo_paths[g]
                photo_file = os.path.join(loader.path_photo, photo)
                if not os.path.exists(photo_file):
                    raise FileNotFoundError(f"retrieved photo {photo_file} is missing")
                wrong = self.parse_class(photo) != cls
                copyfile(photo_file, os.path.join(folder, f"{rank}_f.jpg" if wrong else f"{rank}.jpg"))

    @staticmethod
    def compute_precisions_at_k(relevances):
        """P@K = (correct retrievals) / K per query; relevances: (n_queries, K)"""
        return np.asarray(relevances).mean(axis=1)

    @staticmethod
    def compute_average_precisions(relevances, n_relevant_items, ver=1):
        """AP per query from a (n_queries, K) relevance matrix (retrieve.py:170-201). ver 1: interpolated precision
        (running maximum from the right) averaged over the relevant ranks; ver 2: sum of the precisions at the relevant
        ranks over min(K, n_relevant_items); ver 3: the same sum over the number of relevant retrievals.

        ver 3 is dtype-dependent in the reference, and that is reproduced: its running count is `+` on a copy of the
        input, which on a BOOLEAN matrix (what get_retrievals returns) is a logical or, so ver 3 of a boolean matrix
        is sum_m (1 / r_m) / R. On a 0 / 1 integer matrix it is the sum_m (m / r_m) / R the formula is written for, and
        that is what nsvd_retrieval_eval / evaluate(ap_ver=3) compute."""
        boolean = np.asarray(relevances).dtype == np.bool_
        rel = np.asarray(relevances).astype(bool)
        K = rel.shape[1]
        hits = rel.cumsum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            precs = hits / np.arange(1, K + 1)[np.newaxis, :]
            found = rel.sum(axis=1)
            if ver == 1:
                max_precs = np.maximum.accumulate(precs[:, ::-1], axis=1)[:, ::-1]
                return (max_precs * rel).sum(axis=1) / found
            if ver == 2:
                return (precs * rel).sum(axis=1) / np.minimum(K, np.asarray(n_relevant_items))
            if ver == 3:
                if boolean:
                    return (rel / np.arange(1, K + 1)[np.newaxis, :]).sum(axis=1) / found
                return (precs * rel).sum(axis=1) / found
        raise ValueError("ver must be 1, 2 or 3")


def evaluate_truncations(model, loader, trunc_dims, perm=None, n_retrievals=100, metric="inner_product", ap_ver=1,
                         device=None, retrieval=None, verbose=False):
    """The truncation sweep of main_sketchy.py:325-358: P@K and mAP@all of the embedding cut to its first t coordinates
    (t > 0: ``perm[:t]``) or its last -t (t < 0: ``perm[t:]``), for every t of ``sorted(trunc_dims)``.

    ``model``: a HeteroNetwork (``forward_single(x, side)[1]`` is the embedding) or a pair of callables (model_x,
    model_y). The loader's features are embedded ONCE; each truncation is one nsvd_retrieval_eval call on a column
    window of the embeddings (no copy). A ``perm`` that is not the identity gathers the columns once.
    Returns (trunc_dims sorted, prec_at_Ks, map_at_alls) as numpy arrays - what the script saves."""
    if retrieval is None:
        retrieval = SketchyRetrieval(loader, n_retrievals=n_retrievals, metric=metric, device=device)
    if isinstance(model, (tuple, list)):
        model_x, model_y = model
    else:
        model_x = lambda x: model.forward_single(x, "x")[1]  # noqa: E731
        model_y = lambda y: model.forward_single(y, "y")[1]  # noqa: E731
    zxs, zys = retrieval.embed(model_x, model_y)
    width = zxs.shape[1]
    if perm is not None:
        perm = torch.as_tensor(perm, dtype=torch.long)
        if perm.numel() != width:
            raise ValueError(f"perm must hold the {width} embedding coordinates")
        if not torch.equal(perm, torch.arange(width)):
            zxs, zys = zxs[:, perm.to(zxs.device)].contiguous(), zys[:, perm.to(zys.device)].contiguous()
    dims = sorted(int(t) for t in trunc_dims)
    prec_at_Ks, map_at_alls = [], []
    for t in dims:
        if t == 0 or abs(t) > width:
            raise ValueError(f"truncation {t} outside the embedding width {width}")
        cols = slice(0, t) if t > 0 else slice(width + t, width)
        p, ap = retrieval.evaluate_embeddings(zxs[:, cols], zys[:, cols], ap_ver=ap_ver, tag=f"test{t}",
                                              return_map_all=True, verbose=verbose)
        prec_at_Ks.append(p.mean())
        map_at_alls.append(ap.mean())
    return np.array(dims), np.array(prec_at_Ks), np.array(map_at_alls)
