"""Eigenfunction accuracy of a trained model: the headline hydrogen configuration (BASELINE.json configs[1]: 2-D
hydrogen, L = 16, batch 512; scripts/exps/pde/hydrogen.sh's schedule) trained through FusedTrainer and measured at the
schedule's evaluation points against the analytic eigenfunctions (FusedTrainer.eigenfunction_accuracy: per-level
subspace distance, per-function angle, Procrustes residual, the levels' Gram defect on the arange(-lim, lim, 0.1)^2 grid).
--potential harmonic_oscillator: oscillator.sh's configuration on one GPU (L = 32, batch 4096, sequential nesting,
exponential mask; Lg = 36, the metric needs the whole n = 7 shell).
--ndim 3 (hydrogen only): the 3-D hydrogen atom on the fused kernels, L = 5 = the n = 1 and n = 2 shells
(1 and 4 states; the box [-20, 20]^3 holds them, it would cut the n = 3 shell), batch 512, a SHORT run (5000 steps unless --steps says otherwise: this is the evaluation path's
script, not a converged 3-D result), measured against operators.Hydrogen3D on the cubic grid arange(-20, 20, 0.4)^3
(10^6 points, the 2-D headline grid's size).

    python scripts/eval_eigfuncs.py --steps 500000 [--nesting sequential] [--timing]
    python scripts/eval_eigfuncs.py --ckpt weights.pth          # evaluate saved weights, no training
    python scripts/eval_eigfuncs.py --ndim 3 [--steps 5000] [--timing]

Writes profiles/eigfunc_accuracy_<problem>.json (hydrogen3d for --ndim 3; or --out). --save-ckpt writes the trained weights (torch.save of
{"model": state_dict, "ema": EMA state_dict}, the reference's key layout), the file --ckpt reads.

--timing (after the last evaluation, on the same trainer in the same process): wall time, ending in a device
synchronise, of spectrum() and of eigenfunction_accuracy() on the grid, alternated, five warm repetitions each; and of
the HOST route to the same metrics - the weighted functions copied off the device, the ground truths evaluated by
numpy, the three products and the metrics on the host.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_svd_amd import eigfuncs as E
from neural_svd_amd import hip_ops as H
from neural_svd_amd.operators import HarmonicOscillator, Hydrogen2D, Hydrogen3D
from neural_svd_amd.trainer import FusedTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(m):
    """the metrics as JSON: per level and per function"""
    return dict(levels=[list(v) for v in m["levels"]],
                subspace_distance=[float(v) for v in m["subspace_distance"]],
                angle_rad=[None if np.isnan(v) else float(v) for v in m["angle"]],
                procrustes_residual=[None if np.isnan(v) else float(v) for v in m["procrustes_residual"]],
                gram_defect=[float(v) for v in m["gram_defect"]],
                eigvals=[float(v) for v in m["eigvals"]])


def timed(fn, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return sorted(out)


def host_route(tr, gt, lim, val_eps, chunk=8192):
    """the same metrics without the new kernel: the weighted functions (n, L) copied to the host, the ground truths
    evaluated there (numpy float64), products and metrics on the host"""
    t = E.table_of(gt, tr.shape.L)
    D = tr.shape.D
    ax = torch.from_numpy(np.arange(-lim, lim, val_eps))
    grid = torch.stack([g.reshape(-1) for g in torch.meshgrid(*(D * [ax]), indexing="xy")], dim=1).float().to(tr.device)
    inv = (2.0 * lim) ** (0.5 * D)  # 1 / sqrt(p_val), p_val = (2 lim)^-D
    sigma = tr.problem.sigma
    phi = []
    ws = H.new_workspace(tr.shape, chunk, tr.device)
    for i in range(0, len(grid), chunk):
        xb = grid[i:i + chunk]
        wsb = ws if len(xb) == chunk else H.new_workspace(tr.shape, len(xb), tr.device)
        f, _ = H.operator_forward(tr.shape, tr._ema_params, tr.problem, xb, wsb, False, tr.path)
        w = torch.exp(-0.25 * (xb / sigma).pow(2).sum(1, keepdim=True)) / (np.sqrt(2 * np.pi) * sigma) ** (0.5 * D) * inv
        phi.append(torch.nan_to_num(w * f).cpu())
    phi = torch.cat(phi).numpy().astype(np.float64)
    psi = E.evaluate_host(gt, t.qnums, grid.cpu().numpy()) * inv
    n = len(grid)
    return E.eigenfunction_metrics(psi.T @ psi / n, psi.T @ phi / n, phi.T @ phi / n, t.degeneracy), phi.nbytes // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--potential", default="hydrogen", choices=["hydrogen", "harmonic_oscillator"])
    ap.add_argument("--ndim", type=int, default=2, choices=[2, 3], help="3: the 3-D hydrogen atom (hydrogen only)")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--evals", default="10000,50000,100000,250000,500000")
    ap.add_argument("--nesting", default=None, choices=["joint", "sequential"],
                    help="default: joint for hydrogen (hydrogen.sh), sequential for the oscillator (oscillator.sh)")
    ap.add_argument("--ckpt", default=None, help="evaluate these saved weights instead of training")
    ap.add_argument("--save-ckpt", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    val_eps = 0.1
    if a.ndim == 3:
        if a.potential != "hydrogen":
            ap.error("--ndim 3: hydrogen only")
        a.steps = a.steps or 5000
        L, B, lim, val_eps, gt = 5, 512, 20.0, 0.4, Hydrogen3D(1.0)
        shape = H.ModelShape(L=L, D=3, m=1024, hidden=(128, 128, 128))
        prob = H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, 8.0)
        kw = dict(sampling_scale=8.0, fourier_scale=0.1)
        sequential = a.nesting == "sequential"
    elif a.potential == "hydrogen":
        a.steps = a.steps or 500000
        L, B, lim, gt = 16, 512, 50.0, Hydrogen2D(1.0)
        shape = H.ModelShape(L=L, D=2, m=1024, hidden=(128, 128, 128))
        prob = H.make_problem(H.POT_HYDROGEN, 1.0, 0.01, 100.0, 0.0, 16.0)
        kw = dict(sampling_scale=16.0, fourier_scale=0.1)
        sequential = a.nesting == "sequential"
    else:
        a.steps = a.steps or 100000
        L, B, lim, gt = 32, 4096, 5.0, HarmonicOscillator(1.0, 2)
        shape = H.ModelShape(L=L, D=2, m=256, hidden=(128, 128, 128), has_exp_mask=True)
        prob = H.make_problem(H.POT_HARMONIC, 1.0, 0.01, 1.0, 16.0, 4.0)
        kw = dict(sampling_scale=4.0, fourier_scale=1.0, exp_mask_init=10.0)
        sequential = a.nesting != "joint"
    tr = FusedTrainer(shape, prob, B, sequential=sequential, step=1, lr=1e-4, rmsprop_decay=0.999, ema_decay=0.995,
                      num_iters=a.steps, seed=a.seed, device=dev, **kw)
    table = E.table_of(gt, L)
    rec = dict(config="%d-D %s, L=%d (Lg=%d), B=%d, %s nesting, lr 1e-4 cosine over %d steps, EMA 0.995, eps 0.01, seed %d; "
                      "grid arange(-%g, %g, %g)^%d" % (a.ndim, a.potential, L, table.Lg, B,
                                                       "sequential" if sequential else "joint", a.steps, a.seed, lim, lim,
                                                       val_eps, a.ndim),
               qnums=[list(q) for q in table.qnums], evals=[])
    if a.ckpt:
        ck = torch.load(a.ckpt, map_location=dev)
        tr.P.load_state_dict(ck["model"], ck.get("ema"))
        rec["config"] += "; weights from " + os.path.basename(a.ckpt)
        evals = []
        e = dict(step=None, **record(tr.eigenfunction_accuracy(gt, lim, val_eps, use_ema=True)))
        rec["evals"].append(e)
        print(json.dumps(e), flush=True)
    else:
        evals = sorted({int(e) for e in a.evals.split(",") if int(e) <= a.steps} | {a.steps})
    done = 0
    for target in evals:
        for _ in range(target - done):
            tr.step()
        done = target
        e = dict(step=done, loss=float(tr.loss[0]), **record(tr.eigenfunction_accuracy(gt, lim, val_eps, use_ema=True)))
        rec["evals"].append(e)
        print(json.dumps(e), flush=True)
    if a.save_ckpt:
        torch.save(dict(model=tr.state_dict(), ema=tr.state_dict(ema=True)), a.save_ckpt)
    if a.timing:
        tr.spectrum(lim, val_eps)  # (eigenfunction_accuracy is warm from the evaluations above)
        tr.eigenfunction_accuracy(gt, lim, val_eps)
        t_spec, t_eig = [], []
        for _ in range(5):  # alternated
            t_spec += timed(lambda: tr.spectrum(lim, val_eps), 1)
            t_eig += timed(lambda: tr.eigenfunction_accuracy(gt, lim, val_eps), 1)
        host, nbytes = None, 0

        def run_host():
            nonlocal host, nbytes
            host, nbytes = host_route(tr, gt, lim, val_eps)
        t_host = timed(run_host, 2)
        dev_m = tr.eigenfunction_accuracy(gt, lim, val_eps)
        rec["timing"] = dict(
            grid_points=int(round(2 * lim / val_eps)) ** a.ndim, spectrum_seconds=sorted(t_spec),
            eigenfunction_accuracy_seconds=sorted(t_eig),
            added_fraction_median=(sorted(t_eig)[2] - sorted(t_spec)[2]) / sorted(t_spec)[2],
            host_route_seconds=t_host, host_route_bytes_copied=int(nbytes),
            host_vs_device_max_distance_difference=float(np.max(np.abs(host["subspace_distance"] -
                                                                       dev_m["subspace_distance"]))))
        print(json.dumps(rec["timing"]), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "eigfunc_accuracy_%s.json" %
                                ("hydrogen3d" if a.ndim == 3 else a.potential))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(rec, open(out, "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
