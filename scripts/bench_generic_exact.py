"""Stencil mode against jet mode on the generic kernels: FusedTrainer steps with PATH_GENERIC at laplacian_eps = 0.01 (the
even / odd stencil, 2 D + 1 streams per sample) and with PATH_GENERIC_EXACT at laplacian_eps = 0 (forward-mode jets,
D + 2 streams), same model, same seed, ALTERNATING windows of steps in one loop so that clock and thermal drift hit both.

    python scripts/bench_generic_exact.py --out profiles/generic_exact_bench.json

Rows: configs[1] (2-D hydrogen, L = 16, B = 512, m = 1024) with hidden widths (64, 64, 64) and (256, 256, 256); the cosine
problem at ndim 5 and 10 and H2 at ndim 3 (D = 6) with the drop-in scripts' models (hidden (128, 128, 128), B = 512).
Per row: steps/s of both modes (median of the windows, with min and max) and their ratio; the forward alone
(nsvd_operator_forward, the part whose contraction work scales with the stream count) timed the same way, its ratio, the
model's expectation (2 D + 1) / (D + 2) for it and whether the measured forward ratio reached it; the relative
error of each mode's Tf on one batch of 128 rows against the float64 oracle of the SAME mode (tests/_highdim_oracle.py:
the float64 stencil at eps = 0.01, double autograd for the exact mode), and the distance between the two float64
operators themselves (the stencil's truncation error, which no arithmetic removes).
The comparison base is the stencil mode of the same commit. Nothing here changes what NSVD_PATH_AUTO picks."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from neural_svd_amd import hip_ops as H
from neural_svd_amd.trainer import FusedTrainer
from oracle import nsvd_oracle as O
from tests import _highdim_oracle as HO

DEV = "cuda:0"
PI32 = float(np.float32(np.pi))


def rows():
    hyd = dict(D=2, L=16, m=1024, B=512, sigma=16.0, fourier_scale=0.1, mask=None,
               oracle=HO.Problem(potential=O.POT_HYDROGEN, charge_or_k=1.0, op_scale=100.0, op_shift=0.0, sigma=16.0,
                                 importance=HO.IMP_GAUSSIAN))
    out = [dict(hyd, name="configs[1], hidden (64, 64, 64)", hidden=(64, 64, 64)),
           dict(hyd, name="configs[1], hidden (256, 256, 256)", hidden=(256, 256, 256))]
    for nd in (5, 10):
        out.append(dict(name=f"cosine, ndim {nd}", D=nd, L=4, m=32, B=512, hidden=(128, 128, 128), sigma=PI32,
                        fourier_scale=0.05, mask=None,
                        oracle=HO.Problem(potential=HO.POT_COSINE, pot_coef=HO.COSINE_CS[nd], op_scale=1.0, op_shift=10.0,
                                          sigma=PI32, importance=HO.IMP_UNIFORM)))
    cfg = dict(problem="sch", potential_type="quantum_chemistry", mol_name="H2", ndim=3, laplacian_eps=0.01,
               operator_scale=1.0, operator_shift=0.0, sampling_scale=2.0, hard_mul_const=1.0, sampling_mode="gaussian")
    out.append(dict(name="H2, ndim 3 (D = 6)", D=6, L=4, m=64, B=512, hidden=(128, 128, 128), sigma=2.0,
                    fourier_scale=0.1, mask=4.0, oracle=HO.problem_of(cfg)))
    return out


def hip_problem(prob, D):
    kw = dict(pot_coef=prob.pot_coef)
    if prob.potential == HO.POT_MOLECULE:
        kw = dict(pot_table=torch.tensor(prob.nuclei, dtype=torch.float32, device=DEV).contiguous(),
                  n_nuclei=len(prob.nuclei), pot_const=prob.pot_const)
    elif D > 4 and prob.pot_coef:
        kw = dict(pot_table=torch.tensor(prob.pot_coef, dtype=torch.float32, device=DEV))
    return H.make_problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                          prob.scale_kinetic, prob.hard_mul_const, importance_kind=prob.importance,
                          n_particles=prob.n_particles if prob.n_particles > 1 else 0, **kw)


def trainer(row, exact):
    prob = dataclasses.replace(row["oracle"], eps=0.0 if exact else 0.01)
    shape = H.ModelShape(L=row["L"], D=row["D"], m=row["m"], hidden=row["hidden"], has_exp_mask=row["mask"] is not None)
    tr = FusedTrainer(shape, hip_problem(prob, row["D"]), row["B"], sequential=False, lr=1e-4, seed=0, device=DEV,
                      sampling_scale=row["sigma"], fourier_scale=row["fourier_scale"], exp_mask_init=row["mask"],
                      path=H.PATH_GENERIC_EXACT if exact else H.PATH_GENERIC, sample_seed=5)
    return tr, prob


def tf_error(tr, prob, x):
    """relative error of the HIP Tf against the float64 oracle of the same mode on the rows x, initial weights"""
    n = x.shape[0]
    nl = len(tr.shape.hidden) + 1
    t = [u.double().cpu() for u in tr.P.views(tr.P.flat)]
    p = O.Params(t[:nl], t[nl:2 * nl], tr.P.fourier_B.double().cpu(), t[2 * nl] if tr.shape.has_exp_mask else None)
    ws = H.new_workspace(tr.shape, n, DEV)
    f, Tf = H.operator_forward(tr.shape, tr._params, tr.problem, x, ws, False, tr.path)
    torch.cuda.synchronize()
    c = HO.operator_forward(x.double().cpu(), p, prob)
    return float((Tf.double().cpu() - c.Tf).norm() / c.Tf.norm()), c.Tf


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def summary(v):
    return dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    assert o.windows >= 30, "medians of at least 30 windows"
    table = []
    for row in rows():
        trs = {mode: trainer(row, mode == "jets") for mode in ("stencil", "jets")}
        err, tf64 = {}, {}
        x0 = trs["stencil"][0].sample()[:128].clone().contiguous()  # one batch of 128 rows for both modes
        for mode, (tr, prob) in trs.items():
            assert H.path_name(tr.shape, tr.B, tr.path, tr.problem) == ("generic_exact" if mode == "jets" else "generic")
            err[mode], tf64[mode] = tf_error(tr, prob, x0)
        x = {mode: tr.sample().clone() for mode, (tr, _) in trs.items()}
        fwd = {mode: (lambda tr=tr, xx=x[mode]: tr.forward(xx)) for mode, (tr, _) in trs.items()}
        for mode, (tr, _) in trs.items():
            for _ in range(o.warmup):
                tr.step()
                fwd[mode]()
        sps = {m: [] for m in trs}
        fps = {m: [] for m in trs}
        for _ in range(o.windows):
            for mode, (tr, _) in trs.items():
                sps[mode].append(window(tr.step, o.steps))
            for mode in trs:
                fps[mode].append(window(fwd[mode], o.steps))
        D = row["D"]
        model = (2 * D + 1) / (D + 2)
        step_ratio = statistics.median(sps["jets"]) / statistics.median(sps["stencil"])
        fwd_ratio = statistics.median(fps["jets"]) / statistics.median(fps["stencil"])
        rec = dict(row=row["name"], D=D, L=row["L"], B=row["B"], m=row["m"], hidden=list(row["hidden"]),
                   steps_per_s=dict(stencil=summary(sps["stencil"]), jets=summary(sps["jets"])),
                   step_ratio_jets_over_stencil=round(step_ratio, 3),
                   forwards_per_s=dict(stencil=summary(fps["stencil"]), jets=summary(fps["jets"])),
                   forward_ratio_jets_over_stencil=round(fwd_ratio, 3), model_forward_ratio=round(model, 3),
                   model_held=bool(fwd_ratio >= model),
                   tf_rel_err_vs_float64_of_same_mode=dict(stencil=err["stencil"], jets=err["jets"]),
                   float64_stencil_vs_float64_exact=float((tf64["stencil"] - tf64["jets"]).norm() / tf64["jets"].norm()),
                   windows=o.windows, steps_per_window=o.steps)
        table.append(rec)
        print(json.dumps(rec), flush=True)
        del trs
        torch.cuda.empty_cache()
    if o.out:
        os.makedirs(os.path.dirname(o.out) or ".", exist_ok=True)
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=table), open(o.out, "w"), indent=1)


if __name__ == "__main__":
    main()
