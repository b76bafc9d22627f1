#!/usr/bin/env python3
"""Timing of the Nystrom baseline on the GPU (neural_svd_amd.Nystrom, csrc/nystrom.hip + csrc/rbf_apply.hip).

    python scripts/bench_nystrom.py [--n 8192 --dim 16 --L 10 --ref-n 4096 --out profiles/nystrom_bench.json]

1. The matrix-free solve at --n points (D = --dim, L eigenpairs, both kernel kinds, xs = randn): wall time of the whole
   constructor (host clock around work that ends in a device synchronise; median of --repeats after one warm-up run),
   iterations, convergence, and the split of ONE iteration into its four steps - apply (nsvd_rbf_apply: 3 launches),
   Gram (nsvd_tsgram_f64 twice: S, A of this iteration and C of the next basis), small solve (nsvd_ritz_step_f64, one
   workgroup) and rotate (nsvd_ts_rotate) - each timed with device events over --step-repeats back-to-back calls on
   the solver's own shapes, after a warm-up of the same calls.
2. The reference's own sequence (methods/nystrom.py:25-39) at --ref-n points on the same machine: the float32 Gram by
   torch ops on the GPU, the copy to the host, float32 np.linalg.eigh there - and this solver on the same points.

Everything is a time on this GPU and this host; nothing here is a share of peak. Writes one JSON record."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import Nystrom, hip_ops as H  # noqa: E402
from neural_svd_amd.kernel_ops import RadialKernelOperator  # noqa: E402

DEV = "cuda:0"


def events_us(fn, repeats):
    """mean device time of fn() in microseconds: `repeats` back-to-back calls between two events, after 5 warm-up calls"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / repeats


def iteration_split(op, xs, L, oversample, repeats):
    n = xs.shape[0]
    m = min(n, L + oversample)
    g = torch.Generator(device=DEV).manual_seed(1)
    V = torch.linalg.qr(torch.randn(n, m, device=DEV, generator=g))[0].contiguous()
    W, Vn = torch.empty_like(V), torch.empty_like(V)
    f64 = torch.float64
    S, At, C, Q, T = (torch.empty((m, m), dtype=f64, device=DEV) for _ in range(5))
    theta, resid = torch.empty(m, dtype=f64, device=DEV), torch.empty(m, dtype=f64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_a = H.rbf_apply_workspace(n, n, op.dim, m, DEV)
    ws_g = H.tsgram_workspace(n, m, DEV)

    def apply():
        H.rbf_apply(xs, xs, V, op.kind, op.ell, 1.0 / n, ws=ws_a, out=W)

    def gram():
        H.tsgram_f64(W, V, ws=ws_g, out_xtx=S, out_xty=At)
        H.tsgram_f64(V, None, ws=ws_g, out_xtx=C)

    def solve():
        H.ritz_step_f64(S, At, status, theta, resid, Q, T, C=C)

    def rotate():
        H.ts_rotate(W, T, m, out=Vn)

    out = {}
    for name, fn in (("apply", apply), ("gram", gram), ("small_solve", solve), ("rotate", rotate)):
        out[name + "_us"] = round(events_us(fn, repeats), 2)
    assert int(status.item()) == 0
    out["iteration_us"] = round(sum(out.values()), 2)
    out["block_width"] = m
    return out


def solve_record(op, xs, L, repeats):
    Nystrom(op, xs, L)  # code objects, allocator
    times, ny = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ny = Nystrom(op, xs, L)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return ny, dict(solve_ms_median=round(1e3 * statistics.median(times), 3), solve_ms_min=round(1e3 * min(times), 3),
                    solve_ms_max=round(1e3 * max(times), 3), repeats=repeats, iterations=ny.iterations,
                    converged=bool(ny.converged), worst_relative_residual=float(ny.residuals.max()),
                    eigvals=[float(v) for v in ny.eigvals.cpu()])


def reference_sequence(xs, ell, L, repeats):
    """methods/nystrom.py:25-39 with the Gaussian kernel as torch ops: Gram on the GPU, eigh in float32 on the host"""
    def gram():
        d2 = (xs * xs).sum(1)[:, None] + (xs * xs).sum(1)[None, :] - 2.0 * xs @ xs.T  # (the cheap form: no n x n x D block)
        return torch.exp(-d2.clamp_min(0.0) / (2.0 * ell ** 2))
    gram()
    torch.cuda.synchronize()
    rec = dict(gram_ms=[], copy_ms=[], eigh_ms=[], total_ms=[])
    vals = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        K = gram()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        Kh = K.data.cpu().numpy()
        t2 = time.perf_counter()
        w, U = np.linalg.eigh(Kh)
        vals = w[::-1][:L] / xs.shape[0]
        t3 = time.perf_counter()
        for k, v in (("gram_ms", t1 - t0), ("copy_ms", t2 - t1), ("eigh_ms", t3 - t2), ("total_ms", t3 - t0)):
            rec[k].append(round(1e3 * v, 3))
    out = {k: min(v) for k, v in rec.items()}
    out.update(repeats=repeats, eigvals=[float(v) for v in vals], host_threads=torch.get_num_threads())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--oversample", type=int, default=8)
    ap.add_argument("--ref-n", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-repeats", type=int, default=200)
    ap.add_argument("--ref-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nystrom_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nystrom.py needs a GPU (neural_svd_amd has no CPU path)")
    ell = {"gaussian": float(a.dim) ** 0.5, "exponential": float(a.dim) ** 0.5}
    kinds = {"gaussian": H.RBF_GAUSSIAN, "exponential": H.RBF_EXPONENTIAL}
    xs = torch.randn(a.n, a.dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    rec = dict(n=a.n, dim=a.dim, L=a.L, oversample=a.oversample, device=torch.cuda.get_device_name(0), kinds={})
    for name, kind in kinds.items():
        op = RadialKernelOperator(kind, ell[name], a.dim, device=DEV)
        _, r = solve_record(op, xs, a.L, a.repeats)
        r["ell"] = ell[name]
        r["per_iteration"] = iteration_split(op, xs, a.L, a.oversample, a.step_repeats)
        rec["kinds"][name] = r
        print(name, json.dumps(r))
    # the widest block the solver takes (L = 64, m = 72): where the one-workgroup solve weighs most
    op = RadialKernelOperator(H.RBF_GAUSSIAN, ell["gaussian"], a.dim, device=DEV)
    rec["per_iteration_L64"] = iteration_split(op, xs, 64, a.oversample, max(a.step_repeats // 4, 10))
    print("L=64", json.dumps(rec["per_iteration_L64"]))
    xr = xs[:a.ref_n].contiguous()
    ref = reference_sequence(xr, ell["gaussian"], a.L, a.ref_repeats)
    _, ours = solve_record(op, xr, a.L, a.repeats)
    lam0 = ref["eigvals"][0]
    rec["reference_sequence"] = dict(n=a.ref_n, reference=ref, this_solver=ours,
                                     eigvals_max_diff_over_largest=max(abs(x - y) for x, y in
                                                                       zip(ref["eigvals"], ours["eigvals"])) / lam0)
    print("reference sequence", json.dumps(rec["reference_sequence"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
