#!/usr/bin/env python3
"""The CDK path's first quality number: train configs[4]'s towers (512 -> 8192 -> 512, batch 1024) with FusedCdkStep
on a SYNTHETIC class-structured paired dataset, then run the truncation sweep of scripts/exps/sketchy.sh
(evaluate_truncations: P@100 and mAP@all for 28 truncations of the nested embedding) on held-out classes.

    python scripts/eval_cdk_retrieval.py [--steps 2000 --seed 0]

Dataset (generated on the device from --seed; the Sketchy data itself is out of scope): 125 classes; per class and
domain a 512-d centroid = a shared class direction + a domain-specific offset; a sample = its class centroid + noise.
Training pairs are (sketch, photo) draws of the same class from the first 100 classes; evaluation is zero-shot-like,
on the 25 classes never seen in training (--nq sketches as queries, --ng photos as the gallery).
Writes profiles/cdk_retrieval_synthetic.json: the curve as it came out, monotone or not."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd.cdk import FusedCdkStep, HeteroNetwork, NestedLoRAForCDK, get_mlp  # noqa: E402
from neural_svd_amd.retrieval import evaluate_truncations  # noqa: E402

TRUNC_DIMS = [-512, -448, -384, -320, -256, -192, -128, -64, -32, -16, -8, -4, -2, -1, 1, 2, 4, 8, 16, 32, 64, 128, 192,
              256, 320, 384, 448, 512]  # scripts/exps/sketchy.sh:35


class Synthetic:
    def __init__(self, dev, seed, ncls=125, d=512, domain_shift=1.0, noise=2.0):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.g, self.dev, self.d, self.noise = g, dev, d, noise
        shared = torch.randn(ncls, d, generator=g, device=dev)
        self.centroids = [shared + domain_shift * torch.randn(ncls, d, generator=g, device=dev) for _ in range(2)]

    def draw(self, domain, cls):
        return self.centroids[domain][cls] + self.noise * torch.randn(len(cls), self.d, generator=self.g, device=self.dev)

    def classes(self, n, lo, hi):
        return torch.randint(lo, hi, (n,), generator=self.g, device=self.dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nq", type=int, default=2500)
    ap.add_argument("--ng", type=int, default=5000)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--mu", type=float, default=16.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdk_retrieval_synthetic.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_cdk_retrieval.py needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    B, sizes, train_cls, ncls = 1024, [512, 8192, 512], 100, 125
    torch.manual_seed(a.seed)
    model = HeteroNetwork([get_mlp(sizes, bias=True, nonlinearity="lrelu0.2", use_bn=True) for _ in range(2)],
                          [nn.Identity(), nn.Identity()], mu=a.mu, regularize_mode="l2_ball").to(dev).train()
    method = NestedLoRAForCDK(model, neigs=sizes[-1], step=1, sequential=False, set_first_mode_const=True).to(dev)
    step = FusedCdkStep(method, lr=a.lr, momentum=0.9, max_grad_norm=1.0, t_max=a.steps, batch_size=B)
    data = Synthetic(dev, a.seed, ncls=ncls, d=sizes[0])
    losses = []
    t0 = time.time()
    for t in range(a.steps):
        cls = data.classes(B, 0, train_cls)
        out = step.step(data.draw(0, cls), data.draw(1, cls))
        if t % max(1, a.steps // 20) == 0 or t == a.steps - 1:
            losses.append((t, float(out[0])))
    step.flush_counters()
    torch.cuda.synchronize()
    train_s = time.time() - t0
    model.eval()

    q_cls, g_cls = data.classes(a.nq, train_cls, ncls), data.classes(a.ng, train_cls, ncls)
    loader = types.SimpleNamespace(
        batch_size=B, sketch_features=data.draw(0, q_cls), photo_features=data.draw(1, g_cls),
        sketch_classes=np.array([f"class_{c:03d}" for c in q_cls.cpu().tolist()]),
        photo_classes=np.array([f"class_{c:03d}" for c in g_cls.cpu().tolist()]))
    t0 = time.time()
    dims, prec, mAP = evaluate_truncations(model, loader, TRUNC_DIMS, n_retrievals=100, device=dev)
    torch.cuda.synchronize()
    eval_s = time.time() - t0
    first = [(int(t), float(m)) for t, m in zip(dims, mAP) if t > 0]
    out = {"dataset": {"classes": ncls, "train_classes": train_cls, "d": sizes[0], "domain_shift": 1.0, "noise": 2.0,
                       "queries": a.nq, "gallery": a.ng, "seed": a.seed},
           "towers": sizes, "batch": B, "steps": a.steps, "lr": a.lr, "mu": a.mu, "loss_trace": losses,
           "train_seconds": train_s, "sweep_seconds_host_clock": eval_s, "chance_P": 1.0 / (ncls - train_cls),
           "trunc_dims": [int(t) for t in dims], "prec_at_100": [float(p) for p in prec],
           "map_at_all_ver1": [float(m) for m in mAP],
           "map_monotone_in_first_k": bool(all(b[1] >= a_[1] for a_, b in zip(first, first[1:])))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
