#!/usr/bin/env python3
"""Timing of the truncated-SVD baseline of the kernel SVD operators on the GPU (neural_svd_amd.NystromSVD,
csrc/nystrom_svd.hip + the two-sided products of csrc/rbf_apply_pair.hip / csrc/dot_apply_pair.hip).

    python scripts/bench_ksvd_baseline.py [--n 8192 --dim 16 --L 10 --ref-n 4096 --out profiles/ksvd_baseline_bench.json]

1. The matrix-free solve at --n points a side (D = --dim, L triplets; Gaussian, exponential and arc-cosine kinds;
   xs = randn, ys = 0.5 randn): wall time of the whole constructor (host clock around work that ends in a device
   synchronise; median of --repeats after one warm-up run), iterations, convergence, and the split of ONE iteration into
   its four steps - pair product (apply_pair_raw), two fused Grams (nsvd_tsgram3_f64 twice), small step
   (nsvd_svd_ritz_step_f64, one workgroup) and two rotations (nsvd_ts_rotate twice) - each timed with device events over
   --step-repeats back-to-back calls on the solver's own shapes and a real iteration state, after a warm-up of the same
   calls.
2. The two fused Gram calls against the four nsvd_tsgram_f64 calls that give the same six matrices (that kernel is
   unchanged: the figure is the earlier kernel's, measured in the same session).
3. At L = 64 (m = 72): the small step alone, and the Grams.
4. The library route at --ref-n points a side on the same machine: the float32 cross Gram by torch ops on the GPU, then
   torch.linalg.svd on the device (when the installation runs it) and the copy to the host with float32 np.linalg.svd
   there - and this solver on the same points.

Everything is a time on this GPU and this host; nothing here is a share of peak. Writes one JSON record."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import NystromSVD, hip_ops as H  # noqa: E402
from neural_svd_amd.kernel_ops import DotKernelOperator, RadialKernelOperator  # noqa: E402

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


def iteration_split(op, xs, ys, L, oversample, repeats):
    nx, ny = xs.shape[0], ys.shape[0]
    m = min(nx, ny, L + oversample)
    g = torch.Generator(device=DEV).manual_seed(1)
    U = torch.linalg.qr(torch.randn(nx, m, device=DEV, generator=g))[0].contiguous()
    V = torch.linalg.qr(torch.randn(ny, m, device=DEV, generator=g))[0].contiguous()
    P, R, Un, Vn = torch.empty_like(U), torch.empty_like(V), torch.empty_like(U), torch.empty_like(V)
    f64 = torch.float64
    Sp, PtU, Cu, Sr, RtV, Cv, A, B, Tu, Tv = (torch.empty((m, m), dtype=f64, device=DEV) for _ in range(10))
    sigma, rl, rr = (torch.empty(m, dtype=f64, device=DEV) for _ in range(3))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_a = op.workspace_pair(nx, ny, m, DEV)
    ws_u, ws_v = H.tsgram3_workspace(nx, m, DEV), H.tsgram3_workspace(ny, m, DEV)
    ws_u2, ws_v2 = H.tsgram_workspace(nx, m, DEV), H.tsgram_workspace(ny, m, DEV)
    scale = 1.0 / math.sqrt(nx * ny)

    def apply():
        op.apply_pair_raw(xs, ys, V, U, scale, scale, ws=ws_a, out_x=P, out_y=R)

    def gram():
        H.tsgram3_f64(P, U, ws=ws_u, out_xtx=Sp, out_xty=PtU, out_yty=Cu)
        H.tsgram3_f64(R, V, ws=ws_v, out_xtx=Sr, out_xty=RtV, out_yty=Cv)

    def gram_four_calls():
        H.tsgram_f64(P, U, ws=ws_u2, out_xtx=Sp, out_xty=PtU)
        H.tsgram_f64(U, None, ws=ws_u2, out_xtx=Cu)
        H.tsgram_f64(R, V, ws=ws_v2, out_xtx=Sr, out_xty=RtV)
        H.tsgram_f64(V, None, ws=ws_v2, out_xtx=Cv)

    def step():
        H.svd_ritz_step_f64(PtU, RtV, Sp, Sr, status, Cu, Cv, sigma, rl, rr, A, B, Tu, Tv)

    def rotate():
        H.ts_rotate(P, Tu, m, out=Un)
        H.ts_rotate(R, Tv, m, out=Vn)

    out = {}
    for name, fn in (("pair_product", apply), ("fused_gram_two_calls", gram), ("small_step", step), ("rotate_two", rotate)):
        out[name + "_us"] = round(events_us(fn, repeats), 2)
    out["iteration_us"] = round(sum(out.values()), 2)
    out["gram_four_tsgram_f64_calls_us"] = round(events_us(gram_four_calls, repeats), 2)
    out["status"] = int(status.item())  # (NSVD_RITZ_* bits of the timed small steps: 0 on a healthy state)
    out["block_width"] = m
    return out


def solve_record(op, xs, ys, L, repeats):
    NystromSVD(op, xs, ys, L)  # code objects, allocator
    times, sol = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = NystromSVD(op, xs, ys, L)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sol, dict(solve_ms_median=round(1e3 * statistics.median(times), 3), solve_ms_min=round(1e3 * min(times), 3),
                     solve_ms_max=round(1e3 * max(times), 3), repeats=repeats, iterations=sol.iterations,
                     converged=bool(sol.converged), worst_relative_residual=float(sol.residuals.max()),
                     svals=[float(v) for v in sol.svals.cpu()])


def library_route(xs, ys, ell, L):
    """the float32 Gaussian cross Gram by torch ops on the GPU, then a library SVD: on the device, and on the host"""
    scale = 1.0 / math.sqrt(xs.shape[0] * ys.shape[0])

    def gram():
        d2 = (xs * xs).sum(1)[:, None] + (ys * ys).sum(1)[None, :] - 2.0 * xs @ ys.T  # (the cheap form)
        return torch.exp(-d2.clamp_min(0.0) / (2.0 * ell ** 2)) * scale
    gram()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    C = gram()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = dict(gram_ms=round(1e3 * (t1 - t0), 3), host_threads=torch.get_num_threads())
    try:
        torch.linalg.svd(C[:64, :64])  # code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s_dev = torch.linalg.svd(C, full_matrices=False)[1]
        torch.cuda.synchronize()
        out.update(device_svd_ms=round(1e3 * (time.perf_counter() - t0), 3), device_svals=[float(v) for v in s_dev[:L].cpu()])
    except Exception as e:  # (an installation without the device solver: said so, the host figure stands alone)
        out.update(device_svd_ms=None, device_svd_error=str(e)[:200])
    t0 = time.perf_counter()
    Ch = C.cpu().numpy()
    t1 = time.perf_counter()
    s_host = np.linalg.svd(Ch, full_matrices=False)[1]
    t2 = time.perf_counter()
    out.update(copy_ms=round(1e3 * (t1 - t0), 3), host_svd_ms=round(1e3 * (t2 - t1), 3),
               host_svals=[float(v) for v in s_host[:L]])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksvd_baseline_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ksvd_baseline.py needs a GPU (neural_svd_amd has no CPU path)")
    ell = float(a.dim) ** 0.5
    ops = {"gaussian": RadialKernelOperator(H.RBF_GAUSSIAN, ell, a.dim, device=DEV),
           "exponential": RadialKernelOperator(H.RBF_EXPONENTIAL, ell, a.dim, device=DEV),
           "arccos1": DotKernelOperator(H.DOT_ARCCOS1, a.dim, device=DEV)}
    gen = torch.Generator(device=DEV).manual_seed(0)
    xs = torch.randn(a.n, a.dim, device=DEV, generator=gen)
    ys = 0.5 * torch.randn(a.n, a.dim, device=DEV, generator=gen)
    rec = dict(n=a.n, dim=a.dim, L=a.L, oversample=a.oversample, ell=ell, device=torch.cuda.get_device_name(0), kinds={})
    for name, op in ops.items():
        _, r = solve_record(op, xs, ys, a.L, a.repeats)
        r["per_iteration"] = iteration_split(op, xs, ys, a.L, a.oversample, a.step_repeats)
        rec["kinds"][name] = r
        print(name, json.dumps(r))
    # the widest block the solver takes (L = 64, m = 72): where the one-workgroup step weighs most
    rec["per_iteration_L64"] = iteration_split(ops["gaussian"], xs, ys, 64, a.oversample, max(a.step_repeats // 4, 10))
    print("L=64", json.dumps(rec["per_iteration_L64"]))
    xr, yr = xs[:a.ref_n].contiguous(), ys[:a.ref_n].contiguous()
    ref = library_route(xr, yr, ell, a.L)
    _, ours = solve_record(ops["gaussian"], xr, yr, a.L, a.repeats)
    rec["library_route"] = dict(n=a.ref_n, library=ref, this_solver=ours,
                                svals_max_diff_over_largest=max(abs(x - y) for x, y in
                                                                zip(ref["host_svals"], ours["svals"])) / ref["host_svals"][0])
    print("library route", json.dumps(rec["library_route"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
