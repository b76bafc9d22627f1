#!/usr/bin/env python3
"""nsvd_spin_jac_step against the torch.einsum composition of the same contraction on the same operands, same GPU.

    python scripts/bench_spin.py [--L 10 32 --B 8192 --m 64 --iters 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_spin.py --iters 5      (per-kernel times)

Per L: one entry point call (recomputation of activations and deltas, the MFMA contraction, the block reduction) timed
with events over --iters calls after warm-up, and the library composition: per layer
j_new = einsum('ba,chb,ckb->achk', phi, delta_i, a_{i-1}) * 2 / B1, J <- (1 - decay) J + decay j_new,
g = einsum('ac,achk->chk', gsigma, J) on activations and deltas prepared beforehand (NOT timed for torch: its figure is
the contraction alone). Prints one JSON line and writes profiles/spin_kernel_bench.json (merging with what is there)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import hip_ops as H  # noqa: E402
from neural_svd_amd.trainer import reference_init  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[10, 32])
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spin_kernel_bench.json"))
    a = ap.parse_args()
    dev, hidden, decay = "cuda:0", (128, 128), 0.01
    rows = []
    for L in a.L:
        shape = H.ModelShape(L=L, D=a.dim, m=a.m, hidden=hidden)
        fB, ws, bs, _ = reference_init(shape, 0.3, None, 0)
        ws, bs, fB = [w.to(dev) for w in ws], [b.to(dev) for b in bs], fB.to(dev)
        params = H.pack_params(shape, ws, bs, fB, None)
        grads_t = [torch.zeros_like(t) for t in ws + bs]
        grads = H.pack_params(shape, grads_t[:3], grads_t[3:], None, None)
        x = torch.randn(a.B, a.dim, device=dev)
        phi = H.model_forward(shape, params, x, 1.0, H.model_workspace(shape, a.B, dev))
        gsigma = torch.randn(L, L, dtype=torch.float64, device=dev)
        J = torch.zeros((L, H.spin_state_floats(shape)), dtype=torch.float32, device=dev)
        ws_j = H.spin_jac_workspace(shape, a.B, dev)
        t_hip = timed(lambda: H.spin_jac_step(shape, params, x, phi, 1.0, gsigma, decay, J, grads, ws=ws_j), a.iters)
        flop = 2.0 * L * L * a.B * sum(h * k for h, k in zip(shape.dims, (2 * a.m,) + hidden))
        row = dict(L=L, B=a.B, m=a.m, hidden=list(hidden), spin_jac_step_us=round(t_hip, 1),
                   contraction_tflops_of_the_whole_call=round(flop / t_hip * 1e-6, 1))
        if not a.no_torch:
            feat = torch.cat([torch.sin(x @ fB), torch.cos(x @ fB)], 1)
            z0 = torch.einsum("lhd,bd->lhb", ws[0], feat) + bs[0]
            a0 = torch.nn.functional.softplus(z0)
            z1 = torch.einsum("lhp,lpb->lhb", ws[1], a0) + bs[1]
            a1 = torch.nn.functional.softplus(z1)
            d2 = torch.ones((L, 1, a.B), device=dev)
            d1 = torch.einsum("chp,chb->cpb", ws[2], d2) * torch.sigmoid(z1)
            d0 = torch.einsum("chp,chb->cpb", ws[1], d1) * torch.sigmoid(z0)
            Jt = [torch.zeros((L,) + tuple(w.shape), device=dev) for w in ws]
            gs = gsigma.float()

            def compose():
                for i, (d, inp) in enumerate(((d0, None), (d1, a0), (d2, a1))):
                    if inp is None:
                        jn = torch.einsum("ba,chb,bk->achk", phi, d, feat)
                    else:
                        jn = torch.einsum("ba,chb,ckb->achk", phi, d, inp)
                    Jt[i].mul_(1.0 - decay).add_(jn, alpha=decay * 2.0 / a.B)
                    torch.einsum("ac,achk->chk", gs, Jt[i])

            t_torch = timed(compose, max(a.iters // 4, 2))
            row.update(torch_einsum_composition_us=round(t_torch, 1), speedup=round(t_torch / t_hip, 2))
        rows.append(row)
    rec = dict(device=torch.cuda.get_device_name(0), jac_step=rows)
    print(json.dumps(rec))
    old = {}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
    old.update(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(old, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
