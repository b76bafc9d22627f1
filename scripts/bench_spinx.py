#!/usr/bin/env python3
"""Timing of SpINx's two own kernels on the GPU (csrc/spinx.hip, nsvd_ts_rotate2 in csrc/nystrom.hip).

    python scripts/bench_spinx.py [--B 8192 --repeats 200 --rounds 5 --out profiles/spinx_bench.json]

1. nsvd_spinx_solve next to nsvd_spin_solve at L in {10, 32, 64}: one workgroup each, on the Grams of a random
   (B, L) block; nsvd_spinx_solve with and without the state update.
2. The cotangent products at B rows: the two nsvd_ts_rotate2 calls (dP = P T_pp + K T_kp, dK = P T_pk + K T_kk) against
   the four nsvd_ts_rotate calls plus two torch adds they replace; the two results are compared (one rounding against
   three).

Every time is the mean device time of --repeats back-to-back calls between two events after a warm-up of the same calls;
the two sides of a comparison alternate over --rounds rounds in the same process and the median round is reported with
the extremes. Everything is a time on this GPU; nothing here is a share of peak. Writes one JSON record."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_svd_amd import hip_ops as H  # noqa: E402

DEV = "cuda:0"
F64 = torch.float64


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


def alternate(fns, repeats, rounds):
    """{name: dict(median, min, max)} in microseconds, the candidates taking turns within every round"""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(events_us(fn, repeats))
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
            for k, v in times.items()}


def bench_L(L, B, repeats, rounds):
    g = torch.Generator(device=DEV).manual_seed(L)
    P = torch.randn(B, L, device=DEV, generator=g) * (0.5 + torch.rand(L, device=DEV, generator=g))
    K = (P @ torch.randn(L, L, device=DEV, generator=g) / L ** 0.5 + 0.3 * torch.randn(B, L, device=DEV, generator=g))
    Gpp, Gpk, Gkk = H.tsgram3_f64(P, K)
    w = torch.ones(L + 1, dtype=F64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    state, chol = (torch.zeros((L, L), dtype=torch.float32, device=DEV) for _ in range(2))
    out64 = torch.empty(2 * L + 2, dtype=F64, device=DEV)
    T_s, T_pp, T_kp, T_pk, T_kk = (torch.empty((L, L), dtype=F64, device=DEV) for _ in range(5))
    le = torch.empty(L + 1, dtype=F64, device=DEV)
    gs, gp = (torch.empty((L, L), dtype=F64, device=DEV) for _ in range(2))

    def spinx(update):
        H.spinx_solve(Gpp, 1.0 / B, Gpp, Gpk, Gkk, 1.0 / B, w, None, 0.01, update, state if update else None,
                      chol if update else None, out64, T_s, T_pp, T_kp, T_pk, T_kk, status)

    def spin():
        H.spin_solve(Gpp, 1.0 / B, Gpk, 1.0 / B, 0.01, 1.0 / B, state, chol, le, gs, gp, status)

    solve = alternate({"spin_solve": spin, "spinx_solve": lambda: spinx(True),
                       "spinx_solve_no_state": lambda: spinx(False)}, repeats, rounds)
    assert int(status.item()) == 0
    solve["spinx_over_spin"] = round(solve["spinx_solve"]["median_us"] / solve["spin_solve"]["median_us"], 2)

    dP, dK = torch.empty_like(P), torch.empty_like(K)
    tmp = [torch.empty_like(P) for _ in range(4)]

    def two():
        H.ts_rotate2(P, T_pp, K, T_kp, L, out=dP)
        H.ts_rotate2(P, T_pk, K, T_kk, L, out=dK)

    def four():
        H.ts_rotate(P, T_pp, L, out=tmp[0])
        H.ts_rotate(K, T_kp, L, out=tmp[1])
        H.ts_rotate(P, T_pk, L, out=tmp[2])
        H.ts_rotate(K, T_kk, L, out=tmp[3])
        torch.add(tmp[0], tmp[1], out=dP)
        torch.add(tmp[2], tmp[3], out=dK)

    rot = alternate({"two_ts_rotate2": two, "four_ts_rotate_two_adds": four}, repeats, rounds)
    rot["four_over_two"] = round(rot["four_ts_rotate_two_adds"]["median_us"] / rot["two_ts_rotate2"]["median_us"], 2)
    two()
    a, b = dP.clone(), dK.clone()
    four()
    rot["max_rel_diff"] = max(float((a - dP).norm() / a.norm()), float((b - dK).norm() / b.norm()))
    return dict(solve=solve, rotations=rot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spinx_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spinx.py needs a GPU (neural_svd_amd has no CPU path)")
    rec = dict(B=a.B, repeats=a.repeats, rounds=a.rounds, device=torch.cuda.get_device_name(0), L={})
    for L in (10, 32, 64):
        rec["L"][str(L)] = bench_L(L, a.B, a.repeats, a.rounds)
        print(f"L={L}", json.dumps(rec["L"][str(L)]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
