#!/usr/bin/env python3
"""Time the deep ReLU kinds of the matrix-free dot-product kernel operator (nsvd_dot_apply and nsvd_dot_apply_pair with
NSVD_DOT_RELU_NNGP / NSVD_DOT_RELU_NTK) against what a user can compose from library calls.

    python scripts/bench_relu_kernels.py [--b 8192 --d 16,64 --l 64 --depths 1,3,8 --reps 20 --inner 5]

At B1 = B2 = --b, L = --l, each D of --d, gamma = 2, coef0 = 0.1, x ~ N(0, I / D), y ~ N(0, I / (4 D)) (so that
|x|^2 ~ 1 at every D), timed with device events, ALTERNATING in one loop after a warm-up call each, --inner
calls per timed window, medians (and min, max) over --reps windows, bench_rbf_kernel.py's scheme:
  * `dot_apply` / `dot_apply_pair` of both kinds at each depth of --depths, workspace and outputs reused;
  * `arccos1`: the same entry point with NSVD_DOT_ARCCOS1 (what the depth-1 NNGP case is compared with);
  * `library`: the float32 composition x @ y.T, the recursion in torch ops, @ f (and .T @ f for the pair) on the same
    GPU - it stores the (B, B) matrix and every temporary of the recursion.
The main kernels alone are bracketed with nsvd_profile_next_forward. Before timing every route is compared with its
library composition (max-normalised difference). Writes profiles/relu_kernels_bench.json. The numbers are reported as
they come out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_rbf_kernel import main_kernel_ms, median_ms_alternating  # noqa: E402
from neural_svd_amd import hip_ops as H  # noqa: E402

KINDS = (("nngp", H.DOT_RELU_NNGP), ("ntk", H.DOT_RELU_NTK))
GAMMA, COEF0 = 2.0, 0.1


def library_matrix(x, y, ntk, gamma, coef0, depth):
    S = x @ y.T
    T = S.clone() if ntk else None
    qx, qy = (x * x).sum(1), (y * y).sum(1)
    for _ in range(depth):
        p = torch.sqrt(qx[:, None] * qy[None, :])
        c = (S / p).clamp(-1.0, 1.0)
        t = torch.acos(c)
        S1 = torch.where(p > 0, gamma * p * ((torch.sin(t) + (torch.pi - t) * c).clamp(min=0.0) / torch.pi) + coef0, coef0)
        if ntk:
            T = torch.where(p > 0, S1 + gamma * T * ((torch.pi - t) / torch.pi), coef0)
        S = S1
        qx, qy = gamma * qx + coef0, gamma * qy + coef0
    return T if ntk else S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8192)
    ap.add_argument("--d", default="16,64")
    ap.add_argument("--l", type=int, default=64)
    ap.add_argument("--depths", default="1,3,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relu_kernels_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L = a.b, a.l
    depths = [int(v) for v in a.depths.split(",")]
    recs = []
    for D in [int(v) for v in a.d.split(",")]:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, D, device=dev, generator=g) / D ** 0.5
        y = torch.randn(B, D, device=dev, generator=g) / (2.0 * D ** 0.5)
        f, gg = torch.randn(B, L, device=dev, generator=g), torch.randn(B, L, device=dev, generator=g)
        ws, out = H.dot_apply_workspace(B, B, D, L, dev), torch.empty(B, L, device=dev)
        pws = H.dot_apply_pair_workspace(B, B, D, L, dev)
        ox, oy = torch.empty(B, L, device=dev), torch.empty(B, L, device=dev)
        sc = 1.0 / B
        names, fns, agree = [], [], {}

        def add(name, fn):
            names.append(name)
            fns.append(fn)

        add("apply/arccos1", lambda: H.dot_apply(x, y, f, H.DOT_ARCCOS1, 1.0, 1.0, 2, sc, ws=ws, out=out))
        add("pair/arccos1", lambda: H.dot_apply_pair(x, y, gg, f, H.DOT_ARCCOS1, 1.0, 1.0, 2, sc, sc, ws=pws, out_x=ox, out_y=oy))
        for kname, kind in KINDS:
            for depth in depths:
                tag = f"{kname}/depth{depth}"
                add("apply/" + tag, lambda kind=kind, depth=depth: H.dot_apply(x, y, f, kind, GAMMA, COEF0, depth, sc, ws=ws, out=out))
                add("pair/" + tag, lambda kind=kind, depth=depth: H.dot_apply_pair(x, y, gg, f, kind, GAMMA, COEF0, depth, sc, sc,
                                                                                  ws=pws, out_x=ox, out_y=oy))
                ntk = kind == H.DOT_RELU_NTK

                def lib_apply(ntk=ntk, depth=depth):
                    return library_matrix(x, y, ntk, GAMMA, COEF0, depth) @ f * sc

                def lib_pair(ntk=ntk, depth=depth):
                    K = library_matrix(x, y, ntk, GAMMA, COEF0, depth)
                    return K @ gg * sc, K.T @ f * sc
                add("library_apply/" + tag, lib_apply)
                add("library_pair/" + tag, lib_pair)
                fns[-4]()
                ref = lib_apply()
                agree["apply/" + tag] = float((out - ref).abs().max() / ref.abs().max())
                fns[-3]()
                rx, ry = lib_pair()
                agree["pair/" + tag] = max(float((ox - rx).abs().max() / rx.abs().max()),
                                           float((oy - ry).abs().max() / ry.abs().max()))
                del ref, rx, ry
        times = median_ms_alternating(fns, a.reps, a.inner)
        kern = {n: main_kernel_ms(fn) for n, fn in zip(names, fns) if not n.startswith("library")}
        rec = dict(B1=B, B2=B, D=D, L=L, gamma=GAMMA, coef0=COEF0, reps=a.reps, inner=a.inner,
                   routes={n: dict(t, **({"main_kernel_ms": kern[n]} if n in kern else {}),
                                   **({"vs_library_maxnorm": agree[n]} if n in agree else {}))
                           for n, t in zip(names, times)})
        recs.append(rec)
        for n, t in zip(names, times):
            print(f"D={D} {n:34s} {1e3 * t['median_ms']:10.1f} us" + (f"  main kernel {1e3 * kern[n]:9.1f} us" if n in kern else "")
                  + (f"  vs library {agree[n]:.1e}" if n in agree else ""), flush=True)
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), records=recs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
