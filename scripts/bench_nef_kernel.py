#!/usr/bin/env python3
"""Timing of NeuralEF on the matrix-free kernel operators (csrc/nef_rows.hip, neural_svd_amd.neuralef.NefKernelTrainer).

    python scripts/bench_nef_kernel.py [--B 8192 --steps 100 --repeats 200 --rounds 3 --out profiles/nef_kernel_bench.json]

1. The step: NefKernelTrainer.step against the class-path loop it replaces - NeuralEigenfunctions.compute_loss_kernel,
   loss.backward() and nsvd_opt_step per tensor - on the same Gaussian RadialKernelOperator, model and batches, at
   D in {2, 16}, L in {10, 64} and both split_batch modes. Steps per second from a host clock around --steps steps that
   end in a device synchronise, after a warm-up of 10; the two sides alternate over --rounds rounds in one process.
2. The two kernels: nsvd_nef_rows_forward and nsvd_nef_rows_backward on a (B, L) block against the torch composition
   they replace (norm / divide and the running-norm updates forward; torch autograd through u / n(u) backward), as
   mean device time of --repeats back-to-back calls between two events; the results are compared.

Everything is a time on this GPU; nothing here is a share of peak. Writes one JSON record."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import hip_ops as H  # noqa: E402
from neural_svd_amd.kernel_ops import RadialKernelOperator  # noqa: E402
from neural_svd_amd.neuralef import NefKernelTrainer, NeuralEigenfunctions  # noqa: E402

DEV = "cuda:0"
M, HIDDEN, FOURIER_SCALE, LR = 64, (128, 128), 0.3, 1e-3


def class_path(op, tr, L, split):
    """the class-path loop on the trainer's initial weights: returns step(x)"""
    from neural_svd_amd.models import GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    fm = GaussianFourierFeatureTransform(input_dim=op.dim, mapping_size=M, scale=FOURIER_SCALE)
    base = ParallelMLP(input_dim=op.dim, mlp_hidden_dims=list(HIDDEN), output_dim=1, num_copies=L,
                       nonlinearity="softplus", bias=True, feature_map=fm)
    model = WaveFunctions(base, boundary_mask=lambda x: 1.0, hard_mul_const=1.0)
    with torch.no_grad():
        fm._B.copy_(tr.P.fourier_B)
        for dst, src in zip(list(base.ws) + list(base.bs), tr.P.views(tr.P.flat)):
            dst.copy_(src)
    method = NeuralEigenfunctions(model, L, "unbiased").to(DEV).train()
    params = model.trainable_tensors()
    cfg = H.opt_config("rmsprop", LR, alpha=0.99, eps=1e-10)
    sq = [torch.zeros_like(p.data).view(-1) for p in params]
    t = [0]

    def step(x):
        method.zero_grad()
        loss, _ = method.compute_loss_kernel(op.get_approx_kernel_op, x, None, split_batch=split)
        loss.backward()
        for p, s in zip(params, sq):
            H.opt_step(cfg, p.data.view(-1), p.grad.contiguous().view(-1), s, None, None, t[0])
        t[0] += 1
        return loss
    return step


def steps_per_s(step, xs, steps):
    for i in range(10):
        step(xs[i % len(xs)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(xs[i % len(xs)])
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def bench_step(D, L, B, split, steps, rounds):
    op = RadialKernelOperator(H.RBF_GAUSSIAN, 1.5, D, 1.0, DEV)
    tr = NefKernelTrainer(op, L=L, m=M, hidden=HIDDEN, batch_size=B, split_batch=split, lr=LR,
                          fourier_scale=FOURIER_SCALE, seed=0)
    cls = class_path(op, tr, L, split)
    g = torch.Generator(device=DEV).manual_seed(1)
    xs = [op.sample(B, g) for _ in range(8)]
    rates = dict(trainer=[], class_path=[])
    for _ in range(rounds):
        rates["trainer"].append(steps_per_s(tr.step, xs, steps))
        rates["class_path"].append(steps_per_s(cls, xs, steps))
    out = {k: dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
           for k, v in rates.items()}
    out["trainer_over_class_path"] = round(out["trainer"]["median"] / out["class_path"]["median"], 2)
    return out


def events_us(fn, repeats):
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


def bench_rows(L, B, split, repeats, rounds):
    B1 = (B + 1) // 2 if split else B
    order = (0, 1, 1, 0) if split else (0,)
    g = torch.Generator(device=DEV).manual_seed(L)
    u = torch.randn(B, L, device=DEV, generator=g) * (0.5 + torch.rand(L, device=DEV, generator=g))
    cot = torch.randn(B, L, device=DEV, generator=g)
    ws = H.nef_rows_workspace(B, L, DEV)
    phi, stats, du = torch.empty_like(u), torch.empty((2, L), device=DEV), torch.empty_like(u)
    nb, nu = torch.ones(L, device=DEV), torch.ones(L, device=DEV)
    init = torch.zeros(1, dtype=torch.int32, device=DEV)
    tb, tu = torch.ones(1, L, device=DEV), torch.ones(1, L, device=DEV)
    m = 0.9
    segs = ((0, B1), (B1, B)) if split else ((0, B),)

    def hip_fwd():
        H.nef_rows_forward(u, B1, nb, nu, init, m, order, ws=ws, out=phi, stats=stats)

    def torch_fwd():
        ns = [u[a:b].norm(dim=0, keepdim=True) / (b - a) ** 0.5 for a, b in segs]
        for h in order:
            tb.copy_(m * tb + (1 - m) * ns[h])
            tu.copy_(torch.sqrt(m * tu ** 2 + (1 - m) * ns[h] ** 2))
        return torch.cat([u[a:b] / n for (a, b), n in zip(segs, ns)])

    def hip_bwd():
        H.nef_rows_backward(phi, stats, B1, cot, ws=ws, out=du)

    ur = u.clone().requires_grad_(True)

    def torch_bwd():
        out = torch.cat([ur[a:b] / (ur[a:b].norm(dim=0, keepdim=True) / (b - a) ** 0.5) for a, b in segs])
        return torch.autograd.grad(out, ur, cot)[0]

    fns = dict(hip_forward=hip_fwd, torch_forward=torch_fwd, hip_backward=hip_bwd, torch_forward_backward=torch_bwd)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(events_us(fn, repeats))
    rec = {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
           for k, v in times.items()}
    hip_fwd()
    hip_bwd()
    rec["max_rel_diff"] = max(float((phi - torch_fwd()).norm() / phi.norm()), float((du - torch_bwd()).norm() / du.norm()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nef_kernel_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nef_kernel.py needs a GPU (neural_svd_amd has no CPU path)")
    rec = dict(B=a.B, m=M, hidden=list(HIDDEN), steps=a.steps, repeats=a.repeats, rounds=a.rounds,
               device=torch.cuda.get_device_name(0), step={}, rows={})
    for D in (2, 16):
        for L in (10, 64):
            for split in (False, True):
                key = f"D{D}_L{L}_split{int(split)}"
                rec["step"][key] = bench_step(D, L, a.B, split, a.steps, a.rounds)
                print(key, json.dumps(rec["step"][key]), flush=True)
    for L in (10, 64):
        for split in (False, True):
            key = f"L{L}_split{int(split)}"
            rec["rows"][key] = bench_rows(L, a.B, split, a.repeats, a.rounds)
            print(key, json.dumps(rec["rows"][key]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
