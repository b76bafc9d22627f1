#!/usr/bin/env python3
"""Time nsvd_retrieval_eval against what a user can compose from library calls on the same GPU.

    python scripts/bench_retrieval.py [--nq 12800 --ng 10453 --d 512 --k 100 --classes 25 --reps 15]

Shape: a Sketchy-like evaluation (12 800 sketches, 10 453 photos, 512-d embeddings, P@100, all three average
precisions). Two things are timed with device events, the two routes alternating in one loop after a warm-up call each, medians
of --reps / --sweep-reps:
  * one evaluation at the full width, and
  * the 28-truncation sweep of scripts/exps/sketchy.sh (first / last k coordinates; column windows, no copies).
The baseline is the library composition: zq @ zg.T, torch.sort(descending=True, stable=True), a class gather, and
cumsum-based P@K / AP (all three versions) in query chunks of --chunk rows (the (chunk, Ng) score, index and float64
precision arrays bound its memory). Before timing, both routes are compared on grid-valued (exactly representable)
embeddings: identical top-K indices, AP within 1e-6.
Writes profiles/retrieval_bench.json. The numbers are reported as they come out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import hip_ops as H  # noqa: E402

# scripts/exps/sketchy.sh:35
TRUNC_DIMS = [-512, -448, -384, -320, -256, -192, -128, -64, -32, -16, -8, -4, -2, -1, 1, 2, 4, 8, 16, 32, 64, 128, 192,
              256, 320, 384, 448, 512]


def baseline(zq, zg, q_cls, g_cls, nri, metric, K, chunk):
    """library calls only; returns (topk_idx, prec_at_k, avg_prec (3, Nq)) like the HIP entry point"""
    Nq, Ng = zq.shape[0], zg.shape[0]
    half = 0.5 * (zg * zg).sum(1) if metric == H.RETR_EUCLIDEAN else None
    ranks = torch.arange(1, Ng + 1, device=zq.device, dtype=torch.float64)
    topk, prec, ap = [], [], []
    for lo in range(0, Nq, chunk):
        s = zq[lo: lo + chunk] @ zg.T
        if half is not None:
            s = s - half
        idx = torch.sort(s, dim=1, descending=True, stable=True).indices
        rel = g_cls[idx] == q_cls[lo: lo + chunk, None]
        relf = rel.double()
        precs = relf.cumsum(1) / ranks
        found = relf.sum(1)
        hits = (precs * relf).sum(1)
        max_precs = torch.flip(torch.cummax(torch.flip(precs, [1]), dim=1).values, [1])
        topk.append(idx[:, :K].int())
        prec.append(relf[:, :K].mean(1))
        ap.append(torch.stack([(max_precs * relf).sum(1) / found,
                               hits / torch.minimum(torch.full_like(found, Ng), nri[lo: lo + chunk].double()),
                               hits / found]))
    return torch.cat(topk), torch.cat(prec), torch.cat(ap, dim=1)


def median_ms_alternating(fns, reps):
    """medians (and all times) of several routes timed ALTERNATELY in one loop, so that whatever else the host and the
    device are doing falls on all of them alike; one warm-up call each first (code objects, library algorithm choice,
    allocator)"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, ts in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(float(a.elapsed_time(b)))
    return [(float(np.median(ts)), ts) for ts in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=12800)
    ap.add_argument("--ng", type=int, default=10453)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--classes", type=int, default=25)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sweep-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    q_cls = torch.randint(0, a.classes, (a.nq,), generator=g, device=dev, dtype=torch.int32)
    g_cls = torch.randint(0, a.classes, (a.ng,), generator=g, device=dev, dtype=torch.int32)
    nri = torch.bincount(q_cls.long(), minlength=a.classes)[q_cls.long()].int()
    ws_bytes = H.retrieval_workspace_bytes(a.nq, a.ng, a.d, a.k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    # ---- agreement on exactly representable inputs (ties included) ----
    nchk = min(a.nq, 512)
    eq = torch.randint(-16, 17, (nchk, a.d), generator=g, device=dev).float() / 8
    eg = torch.randint(-16, 17, (a.ng, a.d), generator=g, device=dev).float() / 8
    agree = {}
    for name, metric in (("inner_product", H.RETR_INNER_PRODUCT), ("euclidean", H.RETR_EUCLIDEAN)):
        got = H.retrieval_eval(eq, eg, q_cls[:nchk], g_cls, nri[:nchk], metric, a.k, ws=ws)
        bi, bp, bap = baseline(eq, eg, q_cls[:nchk], g_cls, nri[:nchk], metric, a.k, a.chunk)
        d_ap = (got["avg_prec"].double() - bap)
        agree[name] = {"topk_idx_equal": bool(torch.equal(got["topk_idx"], bi)),
                       "prec_at_k_max_abs_diff": float((got["prec_at_k"].double() - bp).abs().max()),
                       "avg_prec_max_abs_diff": float(d_ap[~d_ap.isnan()].abs().max())}
    print("agreement:", json.dumps(agree))

    # ---- timing on standard normal embeddings ----
    zq = torch.randn(a.nq, a.d, generator=g, device=dev)
    zg = torch.randn(a.ng, a.d, generator=g, device=dev)
    ip = H.RETR_INNER_PRODUCT
    (hip_ms, hip_all), (base_ms, base_all) = median_ms_alternating(
        [lambda: H.retrieval_eval(zq, zg, q_cls, g_cls, nri, ip, a.k, ws=ws),
         lambda: baseline(zq, zg, q_cls, g_cls, nri, ip, a.k, a.chunk)], a.reps)
    dims = [t for t in TRUNC_DIMS if abs(t) <= a.d]

    def window(z, t):
        return z[:, :t] if t > 0 else z[:, a.d + t:]

    def sweep_hip():
        for t in dims:
            H.retrieval_eval(window(zq, t), window(zg, t), q_cls, g_cls, nri, ip, a.k, want_topk=False, ws=ws)

    def sweep_base():
        for t in dims:
            baseline(window(zq, t), window(zg, t), q_cls, g_cls, nri, ip, a.k, a.chunk)

    (hip_sweep_ms, hip_sweep_all), (base_sweep_ms, base_sweep_all) = median_ms_alternating(
        [sweep_hip, sweep_base], a.sweep_reps)
    torch.cuda.reset_peak_memory_stats()
    baseline(zq, zg, q_cls, g_cls, nri, ip, a.k, a.chunk)
    torch.cuda.synchronize()
    base_peak = torch.cuda.max_memory_allocated()
    out = {"device": torch.cuda.get_device_name(0), "Nq": a.nq, "Ng": a.ng, "d": a.d, "K": a.k, "classes": a.classes,
           "reps": a.reps, "sweep_reps": a.sweep_reps,
           "timer": "device events; the two routes alternate in one loop after one warm-up call each; medians",
           "hip_eval_ms": hip_ms, "hip_eval_ms_all": hip_all,
           "baseline_eval_ms": base_ms, "baseline_eval_ms_all": base_all, "baseline_chunk_rows": a.chunk,
           "baseline_over_hip": base_ms / hip_ms,
           "sweep_truncations": dims, "hip_sweep_ms": hip_sweep_ms, "baseline_sweep_ms": base_sweep_ms,
           "hip_sweep_ms_all": hip_sweep_all, "baseline_sweep_ms_all": base_sweep_all,
           "baseline_over_hip_sweep": base_sweep_ms / hip_sweep_ms,
           "hip_workspace_bytes": int(ws_bytes), "baseline_peak_allocated_bytes": int(base_peak),
           "score_matrix_bytes_never_formed": int(a.nq) * int(a.ng) * 4,
           "contraction_gflop": 2e-9 * a.nq * a.ng * a.d, "agreement_on_exact_inputs": agree}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}))


if __name__ == "__main__":
    main()
