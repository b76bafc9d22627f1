#!/usr/bin/env python3
"""Time the dense two-sided product (nsvd_kernel_apply_pair) against the route it replaces.

    python scripts/bench_dense_pair.py [--reps 30 --inner 5]

Square shapes (N1 = N2 = 10 000, L = 64; B1 = B2 = 8192 - cfg4's shape - and B = 2048): the one-pass call against two
nsvd_kernel_apply calls, one on A and one on a transposed copy that this script makes (that entry point takes a single N:
it cannot do more than square). One rectangular shape (20 000 x 5 000, B = 8192) alone. Device events around `inner`
back-to-back calls, every shape warmed up, the two contenders alternated in one process, median (min, max) of `reps`
windows.

Algorithmic bytes of the one-pass call, counted from shapes (B1p, N2p, Lp = B1, N2, L rounded up to 64; RG, CG =
hip_ops.kernel_apply_pair_partition): the gathered rows once per 64 heads, 4 B1p N2p Lp / 64; the partial copies written
and read, 2 * 4 (CG B1p + RG N2p) Lp; the scatter (g read, Sg^T written and read), 4 (B2 L + 2 Lp N2p); f and f^T,
4 (B1 L + 2 Lp B1p); the outputs, 4 (B1 + B2) L. The share of the HBM peak is those bytes / time / 8.0 TB/s (the spec
figure of the MI355X). Workspace bytes of both routes are reported; the two-call route also holds the transposed copy.
Writes profiles/dense_pair_bench.json. The numbers are reported as they come out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import _lib  # noqa: E402
from neural_svd_amd import hip_ops as H  # noqa: E402

HBM_PEAK = 8.0e12
MFMA_F32_PEAK = 155e12


def up64(n):
    return (n + 63) // 64 * 64


def median_ms_alternating(fns, reps, inner):
    for fn in fns:  # warm-up of every shape: code objects, LDS opt-in, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, ts in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ts.append(float(a.elapsed_time(b)) / inner)
    return [dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts))) for ts in times]


def pair_bytes(N2, B1, B2, L, RG, CG):
    B1p, N2p, Lp = up64(B1), up64(N2), up64(L)
    return dict(gathered_rows=4 * B1p * N2p * (Lp // 64), partial_copies=2 * 4 * (CG * B1p + RG * N2p) * Lp,
                scatter=4 * (B2 * L + 2 * Lp * N2p), f_stage=4 * (B1 * L + 2 * Lp * B1p), outputs=4 * (B1 + B2) * L)


def bench_shape(N1, N2, B, L, dev, reps, inner, with_two_call):
    gen = torch.Generator(device=dev).manual_seed(N1 + N2 + B)
    A = torch.zeros((N1, up64(N2)), dtype=torch.float32, device=dev)
    A[:, :N2] = torch.randn(N1, N2, device=dev, generator=gen)
    rows = torch.randint(N1, (B,), device=dev, generator=gen)
    cols = torch.randint(N2, (B,), device=dev, generator=gen)
    g, f = torch.randn(B, L, device=dev, generator=gen), torch.randn(B, L, device=dev, generator=gen)
    ws = H.kernel_apply_pair_workspace(N1, N2, B, B, L, dev)
    ox, oy = torch.empty(B, L, device=dev), torch.empty(B, L, device=dev)

    def one_pass():
        H.kernel_apply_pair(A, N1, N2, rows, cols, g, f, 1.0 / B, 1.0 / B, ws=ws, out_x=ox, out_y=oy)
    fns = [one_pass]
    rec = dict(N1=N1, N2=N2, B1=B, B2=B, L=L, workspace_bytes_one_pass=int(ws.numel()))
    if with_two_call:
        At = torch.zeros((N2, up64(N1)), dtype=torch.float32, device=dev)
        At[:, :N1] = A[:, :N2].T
        n2 = _lib.load().nsvd_kernel_apply_workspace_bytes(N1, B, L)
        ws2 = torch.empty(n2, dtype=torch.uint8, device=dev)
        tx, ty = torch.empty(B, L, device=dev), torch.empty(B, L, device=dev)

        def two_calls():
            H.kernel_apply(A, N1, rows, cols, g, 1.0 / B, ws=ws2, out=tx)
            H.kernel_apply(At, N2, cols, rows, f, 1.0 / B, ws=ws2, out=ty)
        fns.append(two_calls)
        rec.update(workspace_bytes_two_calls=int(n2), transposed_copy_bytes=int(At.numel() * 4))
    t = median_ms_alternating(fns, reps, inner)
    RG, CG = H.kernel_apply_pair_partition(N1, N2, B, B, L)
    by = pair_bytes(N2, B, B, L, RG, CG)
    total = sum(by.values())
    sec = t[0]["median_ms"] * 1e-3
    flops = 4.0 * up64(B) * up64(N2) * up64(L)  # two contractions of the padded block
    rec.update(row_groups=RG, col_groups=CG, one_pass=t[0], algorithmic_bytes=by, algorithmic_bytes_total=total,
               hbm_share=total / sec / HBM_PEAK, gathered_rows_only_hbm_share=by["gathered_rows"] / sec / HBM_PEAK,
               mfma_f32_share=flops / sec / MFMA_F32_PEAK)
    if with_two_call:
        ex = float((ox - tx).norm() / tx.norm())
        ey = float((oy - ty).norm() / ty.norm())
        rec.update(two_calls=t[1], one_pass_over_two_calls=t[0]["median_ms"] / t[1]["median_ms"],
                   rel_diff_out_x=ex, rel_diff_out_y=ey)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_pair_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dense_pair.py needs a GPU (neural_svd_amd has no CPU path)")
    dev = "cuda:0"
    recs = [bench_shape(10000, 10000, 8192, 64, dev, a.reps, a.inner, True),
            bench_shape(10000, 10000, 2048, 64, dev, a.reps, a.inner, True),
            bench_shape(20000, 5000, 8192, 64, dev, a.reps, a.inner, False)]
    for r in recs:
        line = (f"{r['N1']} x {r['N2']}  B {r['B1']}  L {r['L']}: one pass {r['one_pass']['median_ms']:.3f} ms "
                f"({r['one_pass']['min_ms']:.3f} - {r['one_pass']['max_ms']:.3f}), groups {r['row_groups']} x "
                f"{r['col_groups']}, {r['algorithmic_bytes_total'] / 1e6:.0f} MB = {100 * r['hbm_share']:.1f}% of the HBM "
                f"peak, {100 * r['mfma_f32_share']:.1f}% of the fp32 MFMA peak, workspace "
                f"{r['workspace_bytes_one_pass'] / 2 ** 20:.0f} MiB")
        if "two_calls" in r:
            line += (f"; two kernel_apply calls {r['two_calls']['median_ms']:.3f} ms "
                     f"({r['two_calls']['min_ms']:.3f} - {r['two_calls']['max_ms']:.3f}), workspace "
                     f"{r['workspace_bytes_two_calls'] / 2 ** 20:.0f} MiB + transposed copy "
                     f"{r['transposed_copy_bytes'] / 2 ** 20:.0f} MiB; ratio {r['one_pass_over_two_calls']:.3f}")
        print(line)
    rec = dict(shapes=recs, reps=a.reps, inner=a.inner, hbm_peak=HBM_PEAK, mfma_f32_peak=MFMA_F32_PEAK,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
