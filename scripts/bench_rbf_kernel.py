#!/usr/bin/env python3
"""Time nsvd_rbf_apply (the matrix-free radial kernel operator) against what a user can compose from library calls.

    python scripts/bench_rbf_kernel.py [--b 8192 --d 16 --l 64 --n 10000 --ell 4 --reps 30 --inner 10]

Three routes at B1 = B2 = --b, D = --d, L = --l, timed with device events, ALTERNATING in one loop after a warm-up call
each, --inner calls per timed window, medians over --reps windows:
  * `rbf_apply`: hip_ops.rbf_apply (transpose / pad pass, main kernel, slice reduction), workspace and output reused;
  * `library`: the float32 library composition torch.cdist -> exp -> matmul on the same GPU (the yardstick: it stores
    the (B, B) kernel matrix);
  * `kernel_apply`: nsvd_kernel_apply on a stored N = --n dense operator with the same batch and L (what the
    interface had before).
The main kernel alone is bracketed once with nsvd_profile_next_forward. Share of the fp32 MFMA peak (155 TFLOP/s, dense
v_mfma_f32_32x32x2_f32): the issue's model counts 2 B^2 L for the contraction plus 2 B^2 D for distances on the matrix
pipe (10.7 GFLOP at the defaults); this kernel takes the distances by direct differences on the VALU, so the MFMA work
it executes is the contraction alone (8.6 GFLOP) - both fractions are reported, named.
Before timing, rbf_apply is compared with the library composition (max-normalised difference).
Writes profiles/rbf_apply_bench.json. The numbers are reported as they come out.

    python scripts/bench_rbf_kernel.py --dot [--b 8192 --dot-d 16,64 --l 64 --degree 2]

times the dot-product kinds instead (nsvd_dot_apply): at each D of --dot-d, in ONE alternating loop with the same
window scheme, `dot_apply` polynomial (gamma = 1 / D, coef0 = 1, --degree) and arc-cosine, the float32 library
composition of each (x @ x.T, the map, @ f: it stores the (B, B) matrix) and `rbf_apply` (Gaussian, ell = sqrt(D)) on
the same shape; the main kernels alone bracketed with nsvd_profile_next_forward. The MFMA work nsvd_dot_apply executes
is BOTH contractions, 2 B^2 L + 2 B^2 Dp with Dp = D rounded up to 8. Writes profiles/dot_apply_bench.json.

    python scripts/bench_rbf_kernel.py --pair [--b 8192 --pair-d 2,16,64 --l 64]

times the two-sided call (nsvd_rbf_apply_pair: K g and K^T f, every kernel value evaluated once) against TWO
nsvd_rbf_apply calls with swapped arguments (what the interface had before), both kinds, at each D of --pair-d, in ONE
alternating loop with the same window scheme; x ~ N(0, I), y ~ N(0, I / 4), ell = sqrt(D). The MFMA work either route
executes is 4 B^2 L. Writes profiles/rbf_apply_pair_bench.json.

    python scripts/bench_rbf_kernel.py --dot --pair [--b 8192 --pair-d 2,16,64 --l 64 --degree 2]

does the same for the dot-product kinds: nsvd_dot_apply_pair (every x_i . y_j formed and mapped once) against TWO
nsvd_dot_apply calls with swapped arguments, polynomial (gamma = 1 / D, coef0 = 1, --degree) and arc-cosine, at each D
of --pair-d. Per wave and 64-row chunk the two calls issue 2 (Dp / 2 + 32) MFMAs and the fused call Dp / 2 + 64
(Dp = D rounded up to 8); the record carries that ratio beside the measured one, and the spread (min, max) of the 30
windows beside each median. Writes profiles/dot_apply_pair_bench.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import hip_ops as H  # noqa: E402
from neural_svd_amd.kernel_ops import synthetic_psd_kernel  # noqa: E402

MFMA_F32_PEAK = 155e12


def median_ms_alternating(fns, reps, inner):
    for fn in fns:
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


def main_kernel_ms(fn, n=5):
    """the main kernel alone (events recorded by the library around its launch), median of n"""
    ks = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        H.profile_next_forward(e0, e1)
        fn()
        torch.cuda.synchronize()
        ks.append(float(e0.elapsed_time(e1)))
    return float(np.median(ks))


def bench_dot(a, dev):
    B, L = a.b, a.l
    scale = 1.0 / B
    recs = []
    for D in [int(v) for v in a.dot_d.split(",")]:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, D, device=dev, generator=g)
        f = torch.randn(B, L, device=dev, generator=g)
        gamma, coef0, degree, ell = 1.0 / D, 1.0, a.degree, float(D) ** 0.5
        ws, out = H.dot_apply_workspace(B, B, D, L, dev), torch.empty(B, L, device=dev)
        rws, rout = H.rbf_apply_workspace(B, B, D, L, dev), torch.empty(B, L, device=dev)

        def poly():
            H.dot_apply(x, x, f, H.DOT_POLYNOMIAL, gamma, coef0, degree, scale, ws=ws, out=out)

        def arccos():
            H.dot_apply(x, x, f, H.DOT_ARCCOS1, 1.0, 1.0, 2, scale, ws=ws, out=out)

        def lib_poly():
            return ((gamma * (x @ x.T) + coef0) ** degree) @ f * scale

        def lib_arccos():
            n = x.norm(dim=1)
            p = n[:, None] * n[None, :]
            c = ((x @ x.T) / p).clamp(-1.0, 1.0)
            t = torch.acos(c)
            return (p * (torch.sin(t) + (torch.pi - t) * c).clamp(min=0.0)) @ f * (scale / torch.pi)

        def rbf():
            H.rbf_apply(x, x, f, H.RBF_GAUSSIAN, ell, scale, ws=rws, out=rout)

        poly()
        ref = lib_poly()
        agree_p = float((out - ref).abs().max() / ref.abs().max())
        arccos()
        ref = lib_arccos()
        agree_a = float((out - ref).abs().max() / ref.abs().max())
        del ref
        t_p, t_a, t_lp, t_la, t_r = median_ms_alternating([poly, arccos, lib_poly, lib_arccos, rbf], a.reps, a.inner)
        k_p, k_a, k_r = main_kernel_ms(poly), main_kernel_ms(arccos), main_kernel_ms(rbf)
        Dp = (D + 7) // 8 * 8
        flop = 2.0 * B * B * L + 2.0 * B * B * Dp
        recs.append(dict(B1=B, B2=B, D=D, Dp=Dp, L=L, degree=degree, gamma=gamma, coef0=coef0, rbf_ell=ell,
                         dot_apply_polynomial=t_p, dot_apply_arccos1=t_a, library_polynomial=t_lp,
                         library_arccos1=t_la, rbf_apply_gaussian=t_r,
                         dot_main_kernel_ms_polynomial=k_p, dot_main_kernel_ms_arccos1=k_a, rbf_main_kernel_ms=k_r,
                         gflop_mfma_executed_both_contractions=flop / 1e9,
                         mfma_peak_fraction_executed_main_kernel_polynomial=flop / MFMA_F32_PEAK / (k_p * 1e-3),
                         mfma_peak_fraction_executed_main_kernel_arccos1=flop / MFMA_F32_PEAK / (k_a * 1e-3),
                         rbf_mfma_peak_fraction_executed_main_kernel=2.0 * B * B * L / MFMA_F32_PEAK / (k_r * 1e-3),
                         speedup_vs_library_polynomial=t_lp["median_ms"] / t_p["median_ms"],
                         speedup_vs_library_arccos1=t_la["median_ms"] / t_a["median_ms"],
                         ratio_to_rbf_apply_polynomial=t_p["median_ms"] / t_r["median_ms"],
                         ratio_to_rbf_apply_arccos1=t_a["median_ms"] / t_r["median_ms"],
                         max_normalised_difference_to_library_polynomial=agree_p,
                         max_normalised_difference_to_library_arccos1=agree_a))
        print(json.dumps(recs[-1]))
    rec = dict(reps=a.reps, calls_per_window=a.inner, mfma_f32_peak_flops=MFMA_F32_PEAK,
               device=torch.cuda.get_device_name(0), shapes=recs)
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "dot_apply_bench.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)


def bench_pair(a, dev):
    B, L = a.b, a.l
    scale = 1.0 / B
    recs = []
    for D in [int(v) for v in a.pair_d.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, D, device=dev, generator=gen)
        y = 0.5 * torch.randn(B, D, device=dev, generator=gen)
        g = torch.randn(B, L, device=dev, generator=gen)
        f = torch.randn(B, L, device=dev, generator=gen)
        ell = float(D) ** 0.5
        pws = H.rbf_apply_pair_workspace(B, B, D, L, dev)
        rws = H.rbf_apply_workspace(B, B, D, L, dev)
        px, py, rx, ry = (torch.empty(B, L, device=dev) for _ in range(4))
        flop = 4.0 * B * B * L
        for name, kind in (("gaussian", H.RBF_GAUSSIAN), ("exponential", H.RBF_EXPONENTIAL)):
            def pair():
                H.rbf_apply_pair(x, y, g, f, kind, ell, scale, scale, ws=pws, out_x=px, out_y=py)

            def two_calls():
                H.rbf_apply(x, y, g, kind, ell, scale, ws=rws, out=rx)
                H.rbf_apply(y, x, f, kind, ell, scale, ws=rws, out=ry)

            pair()
            two_calls()
            agree = max(float((px - rx).abs().max() / rx.abs().max()), float((py - ry).abs().max() / ry.abs().max()))
            t_p, t_2 = median_ms_alternating([pair, two_calls], a.reps, a.inner)
            k_p = main_kernel_ms(pair)
            recs.append(dict(B1=B, B2=B, D=D, L=L, kind=name, ell=ell, partition=list(H.rbf_apply_pair_partition(B, B, D, L)),
                             workspace_mib=pws.numel() / 2 ** 20, rbf_apply_pair=t_p, two_rbf_apply_calls=t_2,
                             pair_main_kernel_ms=k_p, speedup_over_two_calls=t_2["median_ms"] / t_p["median_ms"],
                             gflop_mfma_executed_both_contractions=flop / 1e9,
                             mfma_peak_fraction_executed_pair_whole_call=flop / MFMA_F32_PEAK / (t_p["median_ms"] * 1e-3),
                             mfma_peak_fraction_executed_pair_main_kernel=flop / MFMA_F32_PEAK / (k_p * 1e-3),
                             mfma_peak_fraction_executed_two_calls=flop / MFMA_F32_PEAK / (t_2["median_ms"] * 1e-3),
                             max_normalised_difference_between_routes=agree))
            print(json.dumps(recs[-1]))
    rec = dict(reps=a.reps, calls_per_window=a.inner, mfma_f32_peak_flops=MFMA_F32_PEAK,
               device=torch.cuda.get_device_name(0), shapes=recs)
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "rbf_apply_pair_bench.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)


def bench_dot_pair(a, dev):
    B, L = a.b, a.l
    scale = 1.0 / B
    recs = []
    for D in [int(v) for v in a.pair_d.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, D, device=dev, generator=gen)
        y = 0.5 * torch.randn(B, D, device=dev, generator=gen)
        g = torch.randn(B, L, device=dev, generator=gen)
        f = torch.randn(B, L, device=dev, generator=gen)
        gamma, coef0, degree = 1.0 / D, 1.0, a.degree
        pws = H.dot_apply_pair_workspace(B, B, D, L, dev)
        dws = H.dot_apply_workspace(B, B, D, L, dev)
        px, py, rx, ry = (torch.empty(B, L, device=dev) for _ in range(4))
        Dp = (D + 7) // 8 * 8
        model = 2.0 * (Dp / 2 + 32) / (Dp / 2 + 64)
        for name, kind in (("polynomial", H.DOT_POLYNOMIAL), ("arccos1", H.DOT_ARCCOS1)):
            def pair():
                H.dot_apply_pair(x, y, g, f, kind, gamma, coef0, degree, scale, scale, ws=pws, out_x=px, out_y=py)

            def two_calls():
                H.dot_apply(x, y, g, kind, gamma, coef0, degree, scale, ws=dws, out=rx)
                H.dot_apply(y, x, f, kind, gamma, coef0, degree, scale, ws=dws, out=ry)

            pair()
            two_calls()
            agree = max(float((px - rx).abs().max() / rx.abs().max()), float((py - ry).abs().max() / ry.abs().max()))
            t_p, t_2 = median_ms_alternating([pair, two_calls], a.reps, a.inner)
            k_p = main_kernel_ms(pair)
            flop_pair = 4.0 * B * B * L + 2.0 * B * B * Dp
            speedup = t_2["median_ms"] / t_p["median_ms"]
            recs.append(dict(B1=B, B2=B, D=D, Dp=Dp, L=L, kind=name, degree=degree, gamma=gamma, coef0=coef0,
                             partition=list(H.dot_apply_pair_partition(B, B, D, L)),
                             workspace_mib=pws.numel() / 2 ** 20, dot_apply_pair=t_p, two_dot_apply_calls=t_2,
                             pair_main_kernel_ms=k_p, speedup_over_two_calls=speedup,
                             mfma_instruction_count_model_ratio=model, model_held=bool(speedup >= model),
                             gflop_mfma_executed_pair=flop_pair / 1e9,
                             mfma_peak_fraction_executed_pair_whole_call=flop_pair / MFMA_F32_PEAK / (t_p["median_ms"] * 1e-3),
                             mfma_peak_fraction_executed_pair_main_kernel=flop_pair / MFMA_F32_PEAK / (k_p * 1e-3),
                             max_normalised_difference_between_routes=agree))
            print(json.dumps(recs[-1]))
    rec = dict(reps=a.reps, calls_per_window=a.inner, mfma_f32_peak_flops=MFMA_F32_PEAK,
               device=torch.cuda.get_device_name(0), shapes=recs)
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "dot_apply_pair_bench.json")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)


DEFAULT_OUT = os.path.join(ROOT, "profiles", "rbf_apply_bench.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dot", action="store_true", help="time the dot-product kinds (nsvd_dot_apply) instead")
    ap.add_argument("--dot-d", default="16,64", help="--dot: the input dimensions, comma separated")
    ap.add_argument("--degree", type=int, default=2, help="--dot: the polynomial kind's degree")
    ap.add_argument("--pair", action="store_true", help="time nsvd_rbf_apply_pair against two nsvd_rbf_apply calls (with --dot: nsvd_dot_apply_pair against two "
                    "nsvd_dot_apply calls)")
    ap.add_argument("--pair-d", default="2,16,64", help="--pair: the input dimensions, comma separated")
    ap.add_argument("--b", type=int, default=8192)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--l", type=int, default=64)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--ell", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rbf_kernel.py needs a GPU: a CPU run measures nothing")
    dev = "cuda:0"
    if a.dot and a.pair:
        return bench_dot_pair(a, dev)
    if a.dot:
        return bench_dot(a, dev)
    if a.pair:
        return bench_pair(a, dev)
    B, D, L = a.b, a.d, a.l
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, D, device=dev, generator=g)
    f = torch.randn(B, L, device=dev, generator=g)
    ws = H.rbf_apply_workspace(B, B, D, L, dev)
    out = torch.empty(B, L, device=dev)
    scale, ell = 1.0 / B, a.ell

    def rbf():
        H.rbf_apply(x, x, f, H.RBF_GAUSSIAN, ell, scale, ws=ws, out=out)

    def library():
        return torch.exp(torch.cdist(x, x) ** 2 * (-1.0 / (2.0 * ell * ell))) @ f * scale

    op = synthetic_psd_kernel(a.n, 256, D, 0, dev)
    idx = op.sample_indices(B, g)
    ka_ws = torch.empty(H._lib.load().nsvd_kernel_apply_workspace_bytes(op.N, B, L), dtype=torch.uint8, device=dev)
    ka_out = torch.empty(B, L, device=dev)

    def dense():
        H.kernel_apply(op.K, op.N, idx, idx, f, scale, ws=ka_ws, out=ka_out)

    rbf()
    ref = library()
    agree = float((out - ref).abs().max() / ref.abs().max())
    t_rbf, t_lib, t_dense = median_ms_alternating([rbf, library, dense], a.reps, a.inner)
    k_ms = main_kernel_ms(rbf)
    flop_contraction, flop_dist = 2.0 * B * B * L, 2.0 * B * B * D
    rec = dict(B1=B, B2=B, D=D, L=L, ell=ell, N_dense=a.n, reps=a.reps, calls_per_window=a.inner,
               rbf_apply=t_rbf, library_cdist_exp_matmul=t_lib, kernel_apply_dense=t_dense,
               rbf_main_kernel_ms=k_ms,
               speedup_vs_library=t_lib["median_ms"] / t_rbf["median_ms"],
               ratio_to_dense_kernel_apply=t_rbf["median_ms"] / t_dense["median_ms"],
               gflop_model_contraction_plus_mfma_distances=(flop_contraction + flop_dist) / 1e9,
               mfma_peak_fraction_on_model_flop_main_kernel=(flop_contraction + flop_dist) / MFMA_F32_PEAK / (k_ms * 1e-3),
               mfma_peak_fraction_on_model_flop_whole_call=(flop_contraction + flop_dist) / MFMA_F32_PEAK /
               (t_rbf["median_ms"] * 1e-3),
               gflop_mfma_executed_contraction_only=flop_contraction / 1e9,
               mfma_peak_fraction_executed_main_kernel=flop_contraction / MFMA_F32_PEAK / (k_ms * 1e-3),
               max_normalised_difference_to_library=agree, device=torch.cuda.get_device_name(0))
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
