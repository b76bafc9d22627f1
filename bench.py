#!/usr/bin/env python3
"""Benchmark of the north-star hot path: NestedLoRA training steps/s on 2D hydrogen, L=16, B=512,
joint nesting (BASELINE.json configs[1]); synthetic Gaussian-sampled coordinate batches, reference
initialisation (random weights of the real architecture).

    python bench.py --gpus N --steps K --warmup W            (N > 1: starts its own N rank processes, one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py ... --full                               (also everything beside the headline: several minutes)
    python bench.py ... --dump-outputs DIR                   (the timed trainer's last-step outputs as DIR/*.npy)

A plain run measures the headline only: set-up, prewarm, W warm-up steps, K timed steps (eager, and at N = 1 also
replayed from a captured HIP graph: `value` is the faster, timing.mode names it), the outputs if asked for, the line.
--full adds the in-run accuracy schedule, `other_configs`, `cpu_baseline`, the side lines and, at N > 1, north_star's
split and the `comm` block. The timed trainers take exactly W + K steps from a fixed seed (the prewarm runs on a
throwaway trainer), so that two runs with the same arguments compute the same thing.

One step = sample x ~ N(0, 16^2 I) on the device -> operator forward (5 stencil evaluations of the
16-headed MLP + FD Hamiltonian) -> EVD loss -> backward -> RMSprop(+cosine LR) -> EMA, all HIP kernels.
N > 1: samples sharded (dp), every rank draws its own 512 rows (weak scaling, global batch 512 N), one
all-reduce of the 2L^2+1 moment floats and a bucketed exchange of the flat gradient per step over RCCL (the exchange
algorithm - all-reduce or reduce-scatter / all-gather, with or without head windows of the backward - is timed briefly
and the fastest one takes the headline run); with --full the `comm` block carries the tuner's table
(`comm.candidates`), the exposed wait of every collective (events on the compute stream) and the same step with the
collectives skipped (`compute_only_ms`), and the other sharding and configs[2] are timed beside it as side fields of
the same JSON line.
Timing: a declared prewarm (>= 1 s of real steps, whatever the step arguments), W warm-up steps, then one block
(--repeats: several) of EXACTLY K steps (barrier + synchronize on both sides, max over ranks); `value` is the median
block.
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense f32-input MFMA peak (= f32 vector peak)
PEAK_HBM_GBS = 8000.0
_KILL_GRACE_S = 10.0  # _launch_ranks: what the other ranks get to exit by themselves after the first one failed
DEGRADED_RC = 3  # exit code of a run that printed a line marked `degraded` (run_main, self_launch)
_PROVISIONAL = {}  # rank 0, N > 1: the line to print if the run dies after its first measured split (main())

CFG = dict(L=16, D=2, m=1024, hidden=(128, 128, 128), B=512, sequential=False, eps=0.01, op_scale=100.0, op_shift=0.0,
           sigma=16.0, fourier_scale=0.1, lr=1e-4, alpha=0.999, ema_decay=0.995, num_iters=500000,
           potential="hydrogen", exp_mask_init=None)
# the other BASELINE.json configs are parity-test cases, not bench lines; --config lets a developer time them
ALT = {
    "cfg1": dict(CFG, B=128, sequential=True),
    "cfg2": CFG,
    "cfg3": dict(CFG, L=32, m=256, B=512, sequential=True, op_scale=1.0, op_shift=16.0, sigma=4.0, fourier_scale=1.0,
                 num_iters=100000, potential="oscillator", exp_mask_init=10.0),
}


def macs_per_sample_head(m, hidden):
    F, dims = 2 * m, list(hidden) + [1]
    M = F * dims[0] + sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    return M, F * dims[0]


def algorithmic_flops(cfg, B):
    """2 B L (E M + M + (M - M1)) per step; forward kernel: 2 B L E M."""
    M, M1 = macs_per_sample_head(cfg["m"], cfg["hidden"])
    E = 1 + 2 * cfg["D"] if cfg["eps"] > 0 else 2 + cfg["D"]  # stencil points, or the streams of the exact-Laplacian jet
    return 2.0 * B * cfg["L"] * (E * M + M + (M - M1)), 2.0 * B * cfg["L"] * E * M


def host_cpu_info():
    """(model name, physical cores, logical CPUs) from /proc/cpuinfo."""
    model, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif not k and phys is not None:
                cores.add((phys, core))
                phys = core = None
        if phys is not None:
            cores.add((phys, core))
    except OSError:
        pass
    logical = os.cpu_count() or 1
    return model, (len(cores) or logical), logical


def _cpu_port_step(cfg):
    """one-step closure of oracle/torch_port.py (eager-PyTorch restatement of the reference's op sequence, shown in
    the build container to run within 10 % of the imported reference: oracle/time_port_vs_reference.py)"""
    from oracle import nsvd_oracle as O
    from oracle import torch_port as TP
    p = O.init_params(cfg["L"], cfg["D"], cfg["m"], cfg["hidden"], cfg["fourier_scale"], seed=0)
    prob = O.Problem(potential=O.POT_HYDROGEN, charge_or_k=1.0, eps=cfg["eps"], op_scale=cfg["op_scale"],
                     op_shift=cfg["op_shift"], sigma=cfg["sigma"])
    v, M = (O.sequential_nesting_masks(cfg["L"]) if cfg["sequential"] else O.joint_nesting_masks(cfg["L"], 1))
    st = TP.PortStep(p, prob, v, M, lr=cfg["lr"], alpha=cfg["alpha"], ema_decay=cfg["ema_decay"],
                     num_iters=cfg["num_iters"])
    g = torch.Generator().manual_seed(0)

    def one_step():
        x = cfg["sigma"] * torch.randn(cfg["B"], cfg["D"], generator=g)
        t0 = time.perf_counter()
        st.step(x)
        return time.perf_counter() - t0
    return one_step


def cpu_baseline(seconds_budget=28.0, min_steps=24, max_steps=200):
    """Time the reference's CPU path (its eager-PyTorch op sequence, oracle/torch_port.py) on the host cores:
    configs[0] (the reference's own CPU-runnable case, B=128 sequential) and configs[1] (the headline workload),
    3 warm-up + >= 24 timed full optimiser steps each (up to 200, about 10 s per config), median.
    Bounded sample: ~25 s of CPU work."""
    model, physical, logical = host_cpu_info()
    t_start = time.perf_counter()
    step2 = _cpu_port_step(ALT["cfg2"])
    # eager PyTorch on a many-core host is fastest well below the logical CPU count: calibrate the intra-op
    # thread count on the headline workload (first call per setting also warms the thread pool)
    cands = sorted({c for c in (8, 16, 32, 64, physical, logical) if c <= logical})
    best, threads = None, cands[0]
    for c in cands:
        torch.set_num_threads(c)
        step2()
        t = min(step2(), step2())
        if best is None or t < best:
            best, threads = t, c
        if time.perf_counter() - t_start > 0.4 * seconds_budget:
            break
    torch.set_num_threads(threads)
    res = {}
    for name, stepf in (("cfg2", step2), ("cfg1", _cpu_port_step(ALT["cfg1"]))):
        for _ in range(3):
            stepf()
        times, t_cfg = [], time.perf_counter()
        while len(times) < min_steps or (len(times) < max_steps and
                                         time.perf_counter() - t_cfg < 0.35 * seconds_budget):
            times.append(stepf())
        times.sort()
        res[name] = dict(steps_per_s=round(1.0 / times[len(times) // 2], 3), timed_steps=len(times),
                         ms_median=round(1e3 * times[len(times) // 2], 2), ms_min=round(1e3 * times[0], 2),
                         ms_max=round(1e3 * times[-1], 2))
    return dict(value=res["cfg2"]["steps_per_s"], unit="steps/s", cores=threads, kind="port",
                threads=threads, physical_cores=physical, logical_cpus=logical, cpu_model=model,
                torch_version=torch.__version__,
                configs={"configs[1] hydrogen L=16 B=512 joint (headline workload)": res["cfg2"],
                         "configs[0] hydrogen L=16 B=128 sequential (reference CPU case)": res["cfg1"]},
                sample=f"{res['cfg2']['timed_steps']} / {res['cfg1']['timed_steps']} timed full optimiser steps (after 3 "
                       f"warm-up) of the headline workload / of configs[0], median; intra-op threads calibrated over {cands} -> {threads} (of {physical} "
                       f"physical cores / {logical} logical CPUs); torch {torch.__version__} CPU eager")


def make_trainer(cfg, par, comm, dev, path, dp_exchange="allreduce", grad_windows=None, grad_buckets=4, sync=False,
                 device_schedule=False):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.trainer import FusedTrainer
    osc = cfg["potential"] == "oscillator"
    shape = H.ModelShape(L=cfg["L"], D=cfg["D"], m=cfg["m"], hidden=cfg["hidden"], has_exp_mask=osc)
    prob = H.make_problem(H.POT_HARMONIC if osc else H.POT_HYDROGEN, 1.0, cfg["eps"], cfg["op_scale"], cfg["op_shift"],
                          cfg["sigma"])
    tr = FusedTrainer(shape, prob, cfg["B"], parallelism=par, sequential=cfg["sequential"], lr=cfg["lr"],
                      rmsprop_decay=cfg["alpha"], ema_decay=cfg["ema_decay"], num_iters=cfg["num_iters"],
                      sampling_scale=cfg["sigma"], fourier_scale=cfg["fourier_scale"],
                      exp_mask_init=cfg["exp_mask_init"], seed=0, device=dev, path=path, comm=comm,
                      dp_exchange=dp_exchange, grad_windows=grad_windows, grad_buckets=grad_buckets,
                      sync_collectives=sync, device_schedule=device_schedule)
    return tr, shape, prob


class GraphStepper:
    """tr.step()-compatible driver of a captured HIP graph of two steps (trainer.GraphedSteps): step() is called once
    per optimiser step and replays the graph on every second call, so that a block of K steps is exactly K steps (an odd
    remainder is an eager step). Bit-identical to eager stepping (tests/test_graph_gpu.py)."""

    def __init__(self, tr):
        self.tr, self.gs, self.pending = tr, tr.capture_graph(2), 0

    def step(self):
        self.pending += 1
        if self.pending == 2:
            self.gs.replay()
            self.pending = 0

    def flush(self):
        if self.pending:
            self.tr.step()
            self.pending = 0


def run_timed_graph(tr, steps, warmup, repeats, prewarm_s, stepper=None):
    """run_timed's protocol with the steps replayed from a HIP graph (single GPU); prewarm_s None: no prewarm;
    stepper: a GraphStepper of `tr` captured beforehand"""
    g = stepper or GraphStepper(tr)
    t0 = time.perf_counter()
    n_pre = 0
    while prewarm_s is not None:
        g.gs.replay(25)
        n_pre += 50
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= prewarm_s:
            break
    for _ in range(warmup):
        g.step()
    g.flush()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            g.step()
        g.flush()
        torch.cuda.synchronize()
        blocks.append(time.perf_counter() - t1)
    return blocks, n_pre


def measure_accuracy(cfg, dev, path, graph=True):
    """The other half of BASELINE.json's metric, measured in THIS run: the reference's full schedule
    (scripts/exps/pde/hydrogen.sh:12-56: cfg['num_iters'] RMSprop steps, cosine learning rate, EMA) on the headline
    workload, then its evaluation - Rayleigh quotients diag(quad) / diag(cov) of the EMA model on the uniform grid
    arange(-50, 50, 0.1)^2 (methods/spectrum.py:74-86, main_pde.py:121-130) - against the analytic 2D hydrogen spectrum
    -Z^2 / (4 (n + 1/2)^2) x operator_scale, degeneracy 2n + 1 (ground_truths.py:120-132)."""
    import numpy as np
    from neural_svd_amd.operators import Hydrogen2D
    tr, _, _ = make_trainer(cfg, "dp", None, dev, path, device_schedule=graph)
    n = cfg["num_iters"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if graph:
        gs = tr.capture_graph(2)
        done = tr.t
        gs.replay((n - done) // 2)
        for _ in range(n - tr.t):
            tr.step()
    else:
        for _ in range(n):
            tr.step()
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    assert tr.t == n
    t1 = time.perf_counter()
    sp = tr.spectrum(50.0, 0.1, use_ema=True)
    t_eval = time.perf_counter() - t1
    ev = sp["eigvals"].numpy()
    gt = cfg["op_scale"] * -Hydrogen2D(1.0).get_eigvals(cfg["L"])
    rel = np.abs(ev - gt) / np.abs(gt)
    return dict(value=round(float(rel.mean()), 5), max=round(float(rel.max()), 5), after_steps=n,
                train_seconds=round(t_train, 2), train_steps_per_s=round(n / t_train, 1),
                eval_seconds=round(t_eval, 2), eval_grid_points=int(round(100.0 / 0.1)) ** 2,
                eigvals=[round(float(v), 4) for v in ev], ground_truth=[round(float(v), 4) for v in gt],
                final_loss=float(tr.loss[0]), stepping="hip_graph_replay" if graph else "eager")


def run_timed(tr, comm, steps, warmup, repeats, prewarm_s, events_every=0):
    """prewarm (>= prewarm_s seconds of real steps: the GPU clock ramp and every lazy allocation are behind us
    whatever --steps/--warmup are), `warmup` untimed steps, then `repeats` blocks of EXACTLY `steps` steps, each
    bracketed by barrier + synchronize on both sides and reduced with MAX over ranks. Returns the per-block
    seconds, the bracketed kernel durations (ms) and the prewarm actually spent. prewarm_s None: no prewarm (the
    caller has run one: prewarm())."""
    from neural_svd_amd import hip_ops as H
    t0 = time.perf_counter()
    n_pre = 0
    while prewarm_s is not None:
        for _ in range(50):
            tr.step()
        n_pre += 50
        torch.cuda.synchronize()
        done = time.perf_counter() - t0 >= prewarm_s
        if comm is not None:  # every rank must leave the loop after the same number of (collective) steps
            done = comm.max_float(0.0 if done else 1.0) == 0.0
        if done:
            break
    prewarm = time.perf_counter() - t0
    for _ in range(warmup):
        tr.step()
    torch.cuda.synchronize()
    n_ev = (steps + events_every - 1) // events_every if events_every else 0
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(n_ev * repeats)]
    blocks = []
    for r in range(repeats):
        if comm is not None:
            comm.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(steps):
            if events_every and i % events_every == 0:
                H.profile_next_forward(*ev[r * n_ev + i // events_every])
            tr.step()
        torch.cuda.synchronize()
        if comm is not None:
            comm.barrier()
        el = time.perf_counter() - t1
        blocks.append(comm.max_float(el) if comm is not None else el)
    kms = sorted(a.elapsed_time(b) for a, b in ev)
    return blocks, kms, prewarm, n_pre


def prewarm(cfg, par, comm, dev, path, seconds, **kw):
    """>= `seconds` of real steps on a throwaway trainer of the timed configuration: the GPU clock ramp and every
    first-use cost are behind us, while the timed trainers take a fixed number of steps (warm-up + timed), so that what
    they compute is the same from run to run. -> (seconds spent, steps)"""
    t, _, _ = make_trainer(cfg, par, comm, dev, path, **kw)
    _, _, spent, n = run_timed(t, comm, 0, 0, 0, seconds)
    del t
    return spent, n


DUMP_BYTES = 64 << 20  # --dump-outputs: at most this much in all


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each (name, tensor) as out_dir/<name>.npy, float32 (float64 stays float64). An array that would
    take the total past DUMP_BYTES is written as a fixed, seeded sample of its flattened elements, with their flat
    indices beside it (<name>_index.npy, float64)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BYTES
    for name, t in arrays:
        a = t.detach().cpu().numpy()
        if a.dtype != np.float64:
            a = a.astype(np.float32)
        left -= 128  # the .npy header
        if a.nbytes > left:
            left -= 128
            n = max(0, min(a.size, left // (a.itemsize + 8)))
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=n, replace=False))
            a = a.reshape(-1)[idx]
            np.save(os.path.join(out_dir, f"{name}_index.npy"), idx.astype(np.float64))
            left -= idx.size * 8
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        left -= a.nbytes


def trainer_outputs(tr):
    """what a caller of the training step receives after its last step: the loss vector {loss, operator term,
    metric term}, f and Tf of the step's batch, the trainable parameters and their EMA shadow (flattened in state_dict
    order)"""
    P = tr.P
    flat = lambda buf: torch.cat([v.reshape(-1) for v in P.views(buf)])  # noqa: E731
    return [("loss", tr.loss), ("f", tr.f_g), ("Tf", tr.Tf_g), ("params", flat(P.flat)), ("ema_params", flat(P.ema))]


def summarize(blocks, steps, world, batch=None):
    """value = world x steps / median block: per-GPU batches stepped on per second over all GPUs (weak scaling: at
    N = 1 exactly optimiser steps/s). batch (rows per GPU): also the unambiguous rates of a multi-GPU line."""
    b = sorted(blocks)
    med = b[len(b) // 2] if len(b) % 2 else 0.5 * (b[len(b) // 2 - 1] + b[len(b) // 2])
    d = dict(value=round(world * steps / med, 3), ms_per_step=round(1e3 * med / steps, 4),
             ms_per_step_min=round(1e3 * b[0] / steps, 4), ms_per_step_max=round(1e3 * b[-1] / steps, 4),
             blocks=len(b))
    if batch is not None:
        d.update(optimizer_steps_per_s=round(steps / med, 3), samples_per_s=round(world * batch * steps / med, 1),
                 global_batch=world * batch)
    return d


def _launch_ranks(n, argv, timeout, extra_env=None):
    """start n rank processes of this script, wait for all of them; -> (return code, rank 0's stdout, error text)"""
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this host driver
        env.update(extra_env or {})
        # (the script this process was started as: a test may wrap bench.py to inject a failing rank)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(sys.argv[0])] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    # rank 0's output is drained while the ranks run: a chatty library (NCCL_DEBUG=INFO writes to stdout) must not fill
    # the pipe and block the rank that holds the result
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    deadline = time.time() + timeout
    rc, err = 0, None
    pending = set(range(n))
    while pending and err is None:
        for r in list(pending):
            code = procs[r].poll()
            if code is None:
                continue
            pending.discard(r)
            if code != 0:
                rc, err = (code if code > 0 else 1), f"rank {r} exited with code {code}"
                break
        if err is None and time.time() > deadline:
            rc, err = 124, f"ranks still running after {timeout:.0f} s"
        if pending and err is None:
            time.sleep(0.2)
    if err is not None:
        # a short grace for the surviving ranks: the rank that holds the provisional line prints it as it dies
        # (run_main), usually within a moment of the first casualty
        grace = time.time() + _KILL_GRACE_S
        while time.time() < grace and any(q.poll() is None for q in procs):
            time.sleep(0.1)
        for q in procs:  # exactly the processes started above
            if q.poll() is None:
                q.kill()
        for q in procs:
            q.wait()
        # rank 0's drained stdout is kept: a rank that died after its first measured split has printed a line marked
        # `degraded` (run_main) which self_launch relays once its ladder is exhausted
        reader.join(timeout=30)
        return rc, "".join(chunks), err
    reader.join(timeout=30)
    out = "".join(chunks)
    if not [ln for ln in out.splitlines() if ln.startswith("{")]:
        return 1, out, "rank 0 printed no JSON line"
    return 0, out, None


def visible_gpus():
    """GPUs a rank process could open, WITHOUT initialising any GPU runtime in this (launcher) process: the visibility
    variables if set, else the render nodes of the amdgpu driver; None when neither says anything (the ranks then fail
    by themselves with a clear message, which the launcher relays)."""
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([t for t in v.split(",") if t.strip() != ""])
    try:
        return len([f for f in os.listdir("/dev/dri") if f.startswith("renderD")])
    except OSError:
        return 0 if not os.path.exists("/dev/kfd") else None


def self_launch(args, argv):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes of this script (one per GPU,
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment), relay rank 0's JSON line, fail if any rank fails.
    Runs BEFORE anything touches the GPU in this process (a process that has initialised the GPU must not spawn the
    ranks by exec, and has no business holding a context on device 0 while they run).
    If the run with the auto-tuned sharding / exchange fails (a rank dies, or hangs in a collective: the process
    group's timeout turns a hang into an exit), the ranks are started again, at most twice: with the plainest RCCL
    sequence (samples sharded, one backward window, one bucketed all-reduce, no side measurements), then with the
    head-sharded step over gloo (0.5 MB per step through the host: RCCL itself is what failed). The line then carries
    `launcher_retry` with the reasons: a number from a plain exchange plus the reason beats no line."""
    n = args.gpus
    if os.environ.get("NSVD_FORCE_DEVICE") is None:
        have = visible_gpus()  # from the environment / the device nodes: no HIP or HSA call in the launcher
        if have is not None and have < n:
            raise SystemExit(f"--gpus {n}: only {have} GPU(s) visible")
    ladder = [("as given: " + " ".join(argv), [], {})]
    if args.config in ALT and args.dp_exchange == "auto" and args.parallelism in ("auto", "dp"):
        plain = ["--parallelism", "dp", "--dp-exchange", "allreduce", "--grad-windows", "1", "--grad-buckets", "1",
                 "--sync", "--no-extras"]
        ladder.append((" ".join(plain), plain, {}))
        if os.environ.get("NSVD_DIST_BACKEND", "nccl") != "gloo":
            hp_gloo = ["--parallelism", "hp", "--sync", "--no-extras"]
            ladder.append((" ".join(hp_gloo) + "  [NSVD_DIST_BACKEND=gloo]", hp_gloo, {"NSVD_DIST_BACKEND": "gloo"}))
    shares = {1: [1.0], 2: [0.6, 0.4], 3: [0.5, 0.25, 0.25]}[len(ladder)]
    failures, degraded = [], None
    for (label, extra, env), share in zip(ladder, shares):
        if failures:
            sys.stderr.write(f"bench.py: {failures[-1]['failed_with']}; starting the ranks again: {label}\n")
        rc, out, err = _launch_ranks(n, argv + extra, args.launch_timeout * share, env)
        if err is None:
            line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
            if failures:
                d = json.loads(line)
                d["launcher_retry"] = {"failed_attempts": failures, "this_line": label}
                line = json.dumps(d)
            print(line)
            return
        failures.append({"attempt": label, "failed_with": err})
        if degraded is None:
            for ln in out.splitlines():
                if ln.startswith("{") and '"degraded"' in ln:
                    degraded = (label, ln)
    sys.stderr.write(f"bench.py: {failures[-1]['failed_with']}\n" + (out[-2000:] if out and degraded is None else ""))
    if degraded is not None:
        # every attempt failed, but one got as far as a measured split before it died: that line (it says `degraded`)
        # beats no line - and the exit code still says the run failed
        d = json.loads(degraded[1])
        d["launcher_retry"] = {"failed_attempts": failures, "this_line": degraded[0] + "  [degraded: died after this split]"}
        print(json.dumps(d))
        sys.stdout.flush()
        raise SystemExit(DEGRADED_RC)
    raise SystemExit(rc or 1)


def _timed_blocks(step, steps, warmup, repeats, prewarm_s, bracket=None, every=4, comm=None):
    """the protocol of run_timed for a plain callable: prewarm, warm-up, `repeats` blocks of exactly `steps` steps
    (comm: barrier + synchronize on both sides of a block, max over ranks); bracket(ev0, ev1) arms the one-shot kernel
    bracket before every `every`-th step"""
    t0 = time.perf_counter()
    n_pre = 0
    while True:
        for _ in range(10):
            step()
        n_pre += 10
        torch.cuda.synchronize()
        done = time.perf_counter() - t0 >= prewarm_s
        if comm is not None:  # every rank must leave the loop after the same number of (collective) steps
            done = comm.max_float(0.0 if done else 1.0) == 0.0
        if done:
            break
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    evs, blocks = [], []
    for _ in range(repeats):
        if comm is not None:
            comm.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(steps):
            if bracket is not None and i % every == 0:
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                bracket(*e)
                evs.append(e)
            step()
        torch.cuda.synchronize()
        if comm is not None:
            comm.barrier()
        el = time.perf_counter() - t1
        blocks.append(comm.max_float(el) if comm is not None else el)
    kms = sorted(a.elapsed_time(b) for a, b in evs)
    return blocks, kms, n_pre


def bench_widened(args, as_dict=False):
    """--config cfg4 / cfg5: the widened rows of SURVEY 8(f), one GPU, through this package's mirrors of the reference
    API (the step the reference's scripts would run), with the dominant contraction bracketed by events inside the C
    call. cfg4 = BASELINE configs[3]: dense PSD kernel operator on 10 000 points, L = 64, B = 8192 indices,
    NestedLoRA.compute_loss_kernel + RMSprop (reference methods/nestedlora.py:230-252; no reference operator exists).
    cfg5 = BASELINE configs[4]: CDK step on synthetic (1024, 512) features: two towers 512 -> 8192 -> 512
    (BatchNorm, lrelu0.2), l2_ball normalisation, NestedLoRAForCDK loss L = 512 + constant mode, SGD momentum
    (reference examples/cdk/sketchy/main_sketchy.py:180-212)."""
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd import parallel
    world = int(os.environ.get("WORLD_SIZE", "1")) if args.gpus > 1 else 1
    rank = int(os.environ.get("RANK", "0")) if world > 1 else 0
    local_rank = int(os.environ.get("NSVD_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0"))) if world > 1 else 0
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    comm = parallel.Communicator.from_env(dev, backend=os.environ.get("NSVD_DIST_BACKEND"),
                                          timeout_s=args.collective_timeout) if world > 1 else None
    steps = min(args.steps, 200)
    warmup = min(args.warmup, 20)
    repeats = args.repeats or 5
    comm_block = None
    strong = False  # cfg5 on several ranks splits the work of ONE step: value = steps / time, not N x that
    if args.config == "cfg4":
        from neural_svd_amd.kernel_ops import FusedKernelTrainer, synthetic_psd_kernel
        N, D, L = 10000, 16, 64
        B = (args.batch_size or 8192) * world  # weak scaling: 8192 indices per GPU; heads sharded over the ranks
        op = synthetic_psd_kernel(N, 256, D, 0, dev)
        # the whole step as a fixed sequence of C-ABI calls on flat buffers (kernel_ops.FusedKernelTrainer): model
        # evaluation, Kf = K[x][:, x] f / B, moments, then d loss / d f + backward + RMSprop inside the backward kernels
        fk = FusedKernelTrainer(op, L=L, m=64, hidden=(128, 128), batch_size=B, sequential=False, lr=1e-4,
                                rmsprop_decay=0.99, rmsprop_eps=1e-8, fourier_scale=0.05, seed=0, comm=comm)
        last = {}

        def step():
            last["loss"] = fk.step()[0]
        # the launch nsvd_profile_next_forward brackets first in a step is the model evaluation - which IS this step's
        # dominant kernel (rocprofv3: 560 us of the 1.6 ms, the gathered-row contraction ka_gemm_kernel 99 us):
        # 2 B L M flops, M = MACs per sample and head of the 128 -> 128 -> 128 -> 1 network behind 2 x 64 features
        kflops = 2.0 * B * (L // world) * (128 * 128 + 128 * 128 + 128)
        kname = "pmlp_plain_stream_fwd_kernel"  # (pmlp_plain_fwd.h; up to round 4: pmlp_fused_fwd_kernel<4, 0, 0, 1>)
        # the step's algorithmic FLOPs: model evaluation + its backward (W_1^T dz_1, dW_1, dW_0: three 128 x 128
        # products per sample and head) + the row's own B x B . B x L contraction
        step_flops_cfg4 = kflops + 2.0 * B * (L // world) * 3 * 128 * 128 + 2.0 * B * B * (L // world)
        workload = (f"configs[3]: dense PSD kernel operator K = A A^T / 256 + 1e-3 I on N = {N} points in R^16, "
                    f"L = {L}, batch {B} indices with replacement, NestedLoRA.compute_loss_kernel(split_batch=False) "
                    f"on a 2 x 128 softplus ParallelMLP, RMSprop")
        metric = "training steps/sec, synthetic dense kernel operator L=64 B=8192 (NestedLoRA kernel path)"
        kernel_apply_gflop = 2.0 * B * B * L / 1e9  # the B x B . B x L contraction of this row
        note = (f"[the row's own contraction: {kernel_apply_gflop:.2f} GFLOP per step in ka_gemm_kernel, "
                "profiles/*_kernel_stats_cfg4.csv] Kf = K[x][:, x] f / B by nsvd_kernel_apply (batch scattered into the index space, gathered rows of K "
                "against it on the fp32 MFMA); model forward / backward on the E = 1 MFMA kernels; d loss / d f and the "
                "RMSprop step inside the backward kernels (nsvd_model_backward_evd_step): no torch autograd, no torch.optim")
    else:
        import torch.nn as nn
        from neural_svd_amd.cdk import HeteroNetwork, NestedLoRAForCDK, get_mlp
        B, d0, d1, d2, L = args.batch_size or 1024, 512, 8192, 512, 512
        torch.manual_seed(0)
        sizes = [d0, d1, d2]
        model = HeteroNetwork([get_mlp(sizes, nonlinearity="lrelu0.2"), get_mlp(sizes, nonlinearity="lrelu0.2")],
                              [nn.Identity(), nn.Identity()], mu=16.0, regularize_mode="l2_ball").to(dev)
        method = NestedLoRAForCDK(model, neigs=L, step=1, sequential=False, set_first_mode_const=True).to(dev)
        from neural_svd_amd.cdk import FusedCdkStep
        x, y = torch.randn(B, d0, device=dev), torch.randn(B, d0, device=dev)
        last = {}
        # the whole step - towers, normalisation, loss, clip_grad_norm_(1.0), SGD momentum, cosine schedule - is ONE C
        # call (nsvd_cdk_step) on the modules' own parameters
        if comm is None:
            fused = FusedCdkStep(method, lr=5e-3, momentum=0.9, max_grad_norm=1.0, t_max=10 * 30, batch_size=B,
                                 use_amp=args.amp, amp_dtype=getattr(args, "amp_dtype", "bfloat16"))
        else:
            # several ranks: the towers' hidden width sharded (cdk.ShardedCdkStep): the SAME batch and the same
            # arithmetic, the work of a step split N ways - strong scaling; two collectives per step
            from neural_svd_amd.cdk import ShardedCdkStep
            strong = True
            fused = fk = ShardedCdkStep(method, comm, lr=5e-3, momentum=0.9, max_grad_norm=1.0, t_max=10 * 30,
                                        batch_size=B, use_amp=args.amp)

        def step():
            last["loss"] = fused.step(x, y)[0]
        # the bracketed launch (nsvd_profile_next_forward): the first contraction Y1 = X W1^T + b1 - float32: one tower's
        # (tower_gemm_nt_kernel, fp32 MFMA); mixed precision: BOTH towers' in one launch (gemm16_kernel, bf16 MFMA)
        nt_l = 2 if (args.amp and comm is None) else 1  # towers per bracketed launch (mixed precision, one GPU: both)
        kflops = 2.0 * B * d0 * (d1 // world) * nt_l
        fused_col = bool(args.amp) and H.tower_mixed_fused(B, d0, d1 // world, d2, 0.2)
        if not args.amp:
            kname = "tower_gemm_nt_kernel"
        elif fused_col:
            # the wide layer with BatchNorm inside the contraction (csrc/tower_col.h): A1 = lrelu(BN1(X W1^T + b1)) in
            # one launch, whole columns per workgroup
            kname = f"nsvd_tcol::tower_col_kernel<false, {B // 128}, "
        else:
            # gemm16.h launch(): the two-workgroups-per-CU form takes launches of >= 512 tiles, gemm16_kernel the rest
            tiles = nt_l * (B // 256) * ((d1 // world) // 128)
            kname = ("nsvd_g16::gemm16b_kernel" if tiles >= 512 and os.environ.get("NSVD_G16_FORM", "")[:1] != "a"
                     else "nsvd_g16::gemm16_kernel") + "<false, false, true>"
        # algorithmic bytes of that launch: X and W1 read once, the (B, d1) output written once (bfloat16 / float32)
        kbytes = ((B * d0 + d0 * (d1 // world)) * (2 if args.amp else 4) + B * (d1 // world) * (2 if args.amp else 4)) * nt_l
        # the STEP against its roofs (one GPU): 2 towers x 5 contractions + the loss's; bytes of the wide tensors and
        # the parameters, each counted once per kernel that must touch it (the narrow end, < 5 %, left out):
        #   optimiser 22 B/param (p, momentum read + written, gradient read, bfloat16 copy written; float32: 20),
        #   gradients written 4 B/param, bfloat16 weights read 3 x 2 B/param, A1 written + read by three consumers,
        #   dY1 written + read, X cast and read twice (float32 mode: Y1, A1, dA1, dY1 and their transposes, 4 B each)
        n_par = 2 * (d0 * d1 + d1 * d2)
        step_flops = 2 * 5 * 2.0 * B * d0 * d1 + 2 * 2.0 * B * (d2 + 1) * (d2 + 1) * 3
        if args.amp:
            step_bytes = n_par * (22 + 4 + 6) + 2 * B * d1 * 2 * (4 + 2) + 2 * B * d0 * (4 + 2 + 2 * 2)
        else:
            step_bytes = n_par * (20 + 4 + 3 * 4) + 2 * B * d1 * 4 * (2 + 3 + 2 + 3) + 2 * B * d0 * 4 * 3
        workload = (f"configs[4]: CDK step on synthetic features x, y ~ randn({B}, {d0}): two towers {d0} -> {d1} -> "
                    f"{d2} (Linear-BatchNorm-lrelu0.2-Linear-BatchNorm), l2_ball mu = 16, NestedLoRAForCDK L = {L} + "
                    f"constant mode, joint nesting, SGD lr 5e-3 momentum 0.9")
        metric = "training steps/sec, CDK two-tower step L=512 B=1024 (NestedLoRA CDK path)"
        if args.amp and getattr(args, "amp_dtype", "bfloat16") == "float16":
            metric += (" [mixed precision: float16 operands, wide activations and their gradients (the reference's autocast "
                       "dtype), f16 MFMA with float32 accumulation, float32 statistics / loss / parameter gradients / "
                       "update, torch.cuda.amp.GradScaler's loss scaling, skipped steps and scheduler gate on the device "
                       "(examples/cdk/sketchy/main_sketchy.py:161,182,194-208); pinned to the float64 oracle with the same "
                       "roundings and scaler arithmetic - parity unpinned vs the reference, whose autocast cannot run "
                       "without a CUDA device]")
        elif args.amp:
            metric += (" [mixed precision: bfloat16 operands, wide activations and their gradients, bf16 MFMA with "
                       "float32 accumulation, float32 statistics / loss / parameter gradients / update - this build's own "
                       "mode, DIFFERENT arithmetic from the Sketchy script's float16 autocast + GradScaler "
                       "(examples/cdk/sketchy/main_sketchy.py:161,182), pinned to the float64 oracle with the same "
                       "roundings, not to a reference fixture]")
        note = ("one C call per step (nsvd_cdk_step): towers on csrc/tower.hip (five contractions + BatchNorm strip "
                "kernels each way; mixed precision: csrc/gemm16.h, both towers per launch, no transposed or re-cast "
                "copies, the narrow end on csrc/cdk_narrow.hip), normalisation, CDK loss, global gradient-norm clip and "
                "SGD momentum (scripts/exps/sketchy.sh: --optimizer sgd --momentum 0.9 --clip_grad_norm); no torch "
                "autograd, no torch.optim")
    use_ev = not args.no_kernel_events
    blocks, kms, n_pre = _timed_blocks(step, steps, warmup, repeats, args.prewarm_seconds,
                                       H.profile_next_forward if use_ev else None, comm=comm)
    summ = summarize(blocks, steps, 1 if strong else world)
    if comm is not None and args.full:
        # where the sharded step's time goes: the exposed collectives, and the step without them
        fk.probe = parallel.CommProbe(dev)
        for _ in range(50):
            step()
        waits = fk.probe.summary()
        fk.probe = None
        comm.barrier()
        comm.stub = True
        bl, _, _ = _timed_blocks(step, steps, warmup, 3, 0.2, None, comm=comm)
        comm.stub = False
        co = summarize(bl, steps, 1 if strong else world)
        comm_block = {"backend": comm.backend,
                      "exchange": ("all-reduce of the two towers' partial second-layer products (2, B, d2) + all-reduce "
                                   "of one float (gradient norm) per step" if strong else
                                   "one blocking all-gather of [f | Kf] per step"),
                      "exchange_bytes": (2 * B * d2 * 4 + 8) if strong else 2 * B * L * 4,
                      "exposed_wait_us_per_step": {k: round(v, 2) for k, v in waits.items()},
                      "compute_only_ms": co["ms_per_step"], "step_ms": summ["ms_per_step"],
                      "rccl_ranks": comm.count_ranks()}
    if rank != 0:
        comm.close()
        return
    roof = None
    if kms:
        kavg = sum(kms) / len(kms)
        ach = kflops / (kavg * 1e-3) / 1e12
        peak = 2500.0 if (args.config == "cfg5" and args.amp) else PEAK_FP32_MFMA_TFLOPS  # dense bf16 MFMA: the guide
        roof = dict(bound="mfma", achieved=round(ach, 3), peak=peak, unit="TFLOP/s",
                    frac=round(ach / peak, 4), traffic=None, kernel=kname,
                    kernel_avg_us=round(kavg * 1e3, 2), kernel_med_us=round(kms[len(kms) // 2] * 1e3, 2),
                    kernel_launches_timed=len(kms), kernel_flops=kflops)
        if args.config == "cfg5":
            # this launch's arithmetic intensity sits next to the ridge of the bf16 roofline (2500 TFLOP/s over
            # 8 TB/s = 312 FLOP/B): both bounds are reported, `bound` names the one whose floor is higher
            hbm_frac = kbytes / (kavg * 1e-3) / 1e9 / PEAK_HBM_GBS
            roof.update(algorithmic_bytes=int(kbytes), flops_per_byte=round(kflops / kbytes, 1),
                        hbm_GBps=round(kbytes / (kavg * 1e-3) / 1e9, 1), hbm_frac=round(hbm_frac, 4),
                        mfma_frac=roof["frac"])
            if kbytes / (PEAK_HBM_GBS * 1e9) > kflops / (peak * 1e12):
                roof.update(bound="hbm", achieved=roof["hbm_GBps"], peak=PEAK_HBM_GBS, unit="GB/s", frac=round(hbm_frac, 4))
            if comm is None:
                # the step: HBM-bound by a wide margin in mixed precision (its bytes at 8 TB/s take twice as long as its
                # FLOPs at the bf16 MFMA peak), MFMA-bound in float32
                st_s = summ["ms_per_step"] * 1e-3
                t_hbm, t_mfma = step_bytes / (PEAK_HBM_GBS * 1e9), step_flops / (peak * 1e12)
                roof["step"] = dict(bound="hbm" if t_hbm > t_mfma else "mfma", algorithmic_bytes=int(step_bytes),
                                    flops=step_flops, hbm_GBps=round(step_bytes / st_s / 1e9, 1),
                                    hbm_frac=round(t_hbm / st_s, 4), mfma_frac=round(t_mfma / st_s, 4))
                roof["step_frac"] = roof["step"]["hbm_frac"] if t_hbm > t_mfma else roof["step"]["mfma_frac"]
        elif comm is None:
            roof["step_frac"] = round(step_flops_cfg4 / (summ["ms_per_step"] * 1e-3) / 1e12 / peak, 4)
    out = {"metric": metric, "value": summ["value"], "unit": "steps/s", "n_gpus": world, "steps": steps, "warmup": warmup,
           "ms_per_step": summ["ms_per_step"], "higher_is_better": True, "scaling": "strong" if strong else "weak",
           "vs_baseline": None,
           "dtype": (("f16" if getattr(args, "amp_dtype", "") == "float16" else "bf16") +
                     " operands / f32 accumulation (tower contractions), f32 elsewhere")
                    if (args.config == "cfg5" and args.amp) else "f32", "data": "synthetic",
           "timing": {"blocks": summ["blocks"], "ms_per_step_min": summ["ms_per_step_min"],
                      "ms_per_step_max": summ["ms_per_step_max"], "prewarm_steps": n_pre},
           "config": {"workload": workload, "note": note, "developer_config": args.config,
                      "not_the_headline_workload": True},
           "final_loss": float(last["loss"]), "roofline": roof, "cpu_baseline": None}
    if args.config == "cfg5" and comm is None and getattr(fused, "scaler", None) is not None:
        out["grad_scaler"] = fused.scaler_state()  # scale, steps taken / skipped over the whole run
    if comm is not None and strong:
        out["config"].update(global_batch=B, parallelism=f"tp{world}",
                             sharding="hidden width of both towers: each GPU owns d1/N rows of Linear1 / BatchNorm1 and "
                                      "the same columns of Linear2; the same batch on every GPU, no gradient traffic")
    elif comm is not None:
        out["config"].update(global_batch=B, parallelism=f"hp{world}",
                             sharding="heads: each GPU owns L/N heads, evaluates them and applies K to them on the "
                                      "whole global batch; one all-gather of f, Kf per step, no gradient traffic")
    if comm is not None:
        out["comm"] = comm_block
    if as_dict:
        return out
    _emit(out)
    if comm is not None:
        comm.close()


def measure_pde_config(cfg, dev, path, steps, warmup, repeats, prewarm_s):
    """One PDE configuration on one GPU with bench.py's protocol (fewer blocks): steps/s, the dominant kernel's event
    bracket and both roofline fractions - the body of an `other_configs` entry."""
    from neural_svd_amd import hip_ops as H
    tr, shape, prob = make_trainer(cfg, "dp", None, dev, path)
    blocks, kms, _, n_pre = run_timed(tr, None, steps, warmup, repeats, prewarm_s, 4)
    d = summarize(blocks, steps, 1, cfg["B"])
    fl_step, fl_fwd = algorithmic_flops(cfg, cfg["B"])
    kname = H.dominant_kernel_name(shape, cfg["B"], path)
    kavg = sum(kms) / len(kms)
    out = dict(value=d["value"], unit="steps/s", ms_per_step=d["ms_per_step"], blocks=d["blocks"], steps=steps,
               global_batch=cfg["B"], final_loss=float(tr.loss[0]), params_finite=bool(torch.isfinite(tr.P.flat).all()),
               path=H.path_name(tr.shape, tr.B, path, prob),
               roofline=dict(bound="mfma", kernel=kname, kernel_avg_us=round(kavg * 1e3, 2),
                             kernel_launches_timed=len(kms), kernel_flops=fl_fwd,
                             achieved=round(fl_fwd / (kavg * 1e-3) / 1e12, 3), peak=PEAK_FP32_MFMA_TFLOPS, unit="TFLOP/s",
                             frac=round(fl_fwd / (kavg * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4),
                             step_flops=fl_step,
                             step_frac=round(fl_step / (d["ms_per_step"] * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)))
    out["timing_mode"] = "eager"
    if out["path"] == "fused_mfma":
        # as the headline does: the same steps replayed from a captured HIP graph (two steps per launch, device-resident
        # schedule; bit-identical to eager stepping) - `value` is the better of the two, named in timing_mode
        try:
            trg, _, _ = make_trainer(cfg, "dp", None, dev, path, device_schedule=True)
            bg, _ = run_timed_graph(trg, steps, warmup, repeats, prewarm_s)
            sg = summarize(bg, steps, 1, cfg["B"])
            out["modes"] = {"eager": dict(value=out["value"], ms_per_step=out["ms_per_step"]),
                            "hip_graph_replay": dict(value=sg["value"], ms_per_step=sg["ms_per_step"],
                                                     params_finite=bool(torch.isfinite(trg.P.flat).all()))}
            if sg["value"] > out["value"] and out["modes"]["hip_graph_replay"]["params_finite"]:
                out["value"], out["ms_per_step"], out["timing_mode"] = sg["value"], sg["ms_per_step"], "hip_graph_replay"
                out["roofline"]["step_frac"] = round(fl_step / (sg["ms_per_step"] * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)
            del trg
        except Exception as e:  # noqa: BLE001
            out["graph_error"] = f"{type(e).__name__}: {e}"
    del tr
    torch.cuda.empty_cache()
    return out


def measure_path_agreement(cfg, dev):
    """In THIS run, HIP kernels only (the float64 oracle is test infrastructure: tests/test_hip_parity.py and
    tests/test_spectrum_parity_gpu.py hold every path to it): f and Tf of the headline model on one batch from the three
    forward paths - native float32 MFMA, the split-bf16 forward (NSVD_PATH_FUSED_BF16X3), and the native kernels in
    exact-Laplacian mode (laplacian_eps = 0: no finite-difference stencil at all; its Tf differs from the stencil's by
    the truncation error, ~3e-5 relative)."""
    from neural_svd_amd import hip_ops as H
    tr, shape, prob = make_trainer(cfg, "dp", None, dev, H.PATH_AUTO)
    x = cfg["sigma"] * torch.randn(cfg["B"], cfg["D"], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    params = tr.P.pack(tr.P.flat, True)

    def fwd(path, eps):
        pr = H.make_problem(H.POT_HARMONIC if cfg["potential"] == "oscillator" else H.POT_HYDROGEN, 1.0, eps,
                            cfg["op_scale"], cfg["op_shift"], cfg["sigma"])
        ws = H.new_workspace(shape, cfg["B"], dev)
        f, Tf = H.operator_forward(shape, params, pr, x, ws, False, path)
        return f.double(), Tf.double()
    f32, T32 = fwd(H.PATH_AUTO, cfg["eps"])
    fb3, Tb3 = fwd(H.PATH_FUSED_BF16X3, cfg["eps"])
    fex, Tex = fwd(H.PATH_AUTO, 0.0)

    def rel(a, b):
        return float((a - b).norm() / b.norm())
    out = dict(f_bf16x3_vs_native=rel(fb3, f32), Tf_bf16x3_vs_native=rel(Tb3, T32),
               f_native_vs_exact_mode=rel(f32, fex), Tf_native_stencil_vs_exact_laplacian=rel(T32, Tex),
               Tf_bf16x3_stencil_vs_exact_laplacian=rel(Tb3, Tex), rows=cfg["B"],
               what="relative l2 differences between the HIP forward paths on one batch of the headline model at its "
                    "initial weights, measured in this run")
    del tr
    torch.cuda.empty_cache()
    return {k: (float(f"{v:.3e}") if isinstance(v, float) else v) for k, v in out.items()}


def measure_other_configs(args, dev):
    """The default single-GPU run also TIMES the other BASELINE.json configurations (about 2-4 s each, after the
    headline): configs[0] (B = 128 sequential), configs[2] per GPU (B = 512) and at its own global batch on one GPU
    (B = 4096), configs[3] (cfg4: dense kernel operator), configs[4] (cfg5) in float32 and in mixed precision. Same
    protocol as the headline with fewer timed steps; never `value`."""
    import copy
    from neural_svd_amd import hip_ops as H
    res = {}
    steps, warmup = 200, 20

    def guard(name, fn):
        try:
            t0 = time.perf_counter()
            res[name] = fn()
            res[name]["measure_seconds"] = round(time.perf_counter() - t0, 1)
        except Exception as e:  # noqa: BLE001
            res[name] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()

    guard("configs[0] hydrogen L=16 B=128 sequential", lambda: measure_pde_config(ALT["cfg1"], dev, H.PATH_AUTO, steps, warmup, 3, 0.3))
    guard("configs[2] oscillator L=32 sequential, B=512 (the per-GPU batch at 8 GPUs)",
          lambda: measure_pde_config(ALT["cfg3"], dev, H.PATH_AUTO, steps, warmup, 3, 0.3))
    guard("configs[2] oscillator L=32 sequential, B=4096 (its global batch on ONE GPU: the N = 1 end of the 1 -> 8 curve)",
          lambda: measure_pde_config(dict(ALT["cfg3"], B=4096), dev, H.PATH_AUTO, 60, 10, 3, 0.3))
    # the reference scripts' OWN head counts (scripts/exps/pde/hydrogen.sh:28 --neigs 36, oscillator.sh:27 --neigs 55) at
    # 512 rows: forward grids of 576 and 880 workgroups on 256 CUs (2.25 and 3.44 rounds: the tail round is partly empty)
    def scripts_shape(cfg):
        d = measure_pde_config(cfg, dev, H.PATH_AUTO, steps, warmup, 3, 0.3)
        wgs = (cfg["B"] // 32) * cfg["L"]
        rounds = -(-wgs // 256)
        d["forward_workgroups"], d["cu_rounds"] = wgs, rounds
        d["tail_quantisation_loss"] = round(1.0 - wgs / (256.0 * rounds), 4)  # share of the CU-rounds left empty
        return d
    guard("reference script shape: hydrogen L=36 B=512 joint (scripts/exps/pde/hydrogen.sh)",
          lambda: scripts_shape(dict(ALT["cfg2"], L=36)))
    guard("reference script shape: oscillator L=55 B=512 sequential (scripts/exps/pde/oscillator.sh)",
          lambda: scripts_shape(dict(ALT["cfg3"], L=55)))
    # hidden widths the fused MFMA kernels are not instantiated for (the reference takes any --mlp_hidden_dims,
    # examples/models/mlp.py:187-221): the generic contractions (gemm_generic.hip); the bracket is the whole forward (all its launches)
    guard("configs[1] with hidden widths (256, 256, 256): generic path",
          lambda: measure_pde_config(dict(ALT["cfg2"], hidden=(256, 256, 256)), dev, H.PATH_AUTO, 100, 10, 3, 0.3))
    guard("configs[1] with hidden widths (64, 64, 64): generic path",
          lambda: measure_pde_config(dict(ALT["cfg2"], hidden=(64, 64, 64)), dev, H.PATH_AUTO, steps, warmup, 3, 0.3))
    for name, config, amp in (("configs[3] dense kernel operator L=64 B=8192 (cfg4)", "cfg4", False),
                              ("configs[4] CDK towers L=512 B=1024 (cfg5), float32", "cfg5", False),
                              ("configs[4] CDK towers L=512 B=1024 (cfg5), mixed precision", "cfg5", True),
                              ("configs[4] CDK towers L=512 B=1024 (cfg5), mixed precision float16 + GradScaler", "cfg5",
                               "float16")):
        a = copy.copy(args)
        a.amp_dtype = "float16" if amp == "float16" else "bfloat16"
        amp = bool(amp)
        a.config, a.amp, a.gpus, a.steps, a.warmup, a.repeats, a.prewarm_seconds = config, amp, 1, 100, 10, 3, 0.3
        a.batch_size, a.no_kernel_events = None, False

        def run(a=a):
            d = bench_widened(a, as_dict=True)
            return dict(value=d["value"], unit=d["unit"], ms_per_step=d["ms_per_step"], steps=d["steps"],
                        blocks=d["timing"]["blocks"], final_loss=d["final_loss"], dtype=d["dtype"], roofline=d["roofline"],
                        metric=d["metric"])
        guard(name, run)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed blocks of --steps steps each (median reported); default: one block, so --steps is the "
                         "number of timed steps (the --full side measurements: about 6000 timed steps in total, "
                         "between 3 and 25 blocks)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: the in-run accuracy schedule, other_configs, the CPU "
                         "baseline, the side lines (bf16x3, other shardings, configs[2]), north_star's split and the "
                         "comm block at N > 1, the per-step loss-sync mode (several minutes); default: the headline "
                         "only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed trainer computed in its last step as "
                         "DIR/<name>.npy (loss, f, Tf, params, ema_params; float32, at most 64 MB); same arguments, "
                         "same inputs")
    ap.add_argument("--prewarm-seconds", type=float, default=1.0,
                    help="real steps run before --warmup, independent of the step arguments (clock ramp)")
    ap.add_argument("--path", default="auto", choices=["auto", "generic", "fused", "bf16x3"],
                    help="bf16x3: developer option, first layer on the bf16 MFMA with three-way split operands "
                         "(NSVD_PATH_FUSED_BF16X3; not the headline path)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-events", action="store_true", help="do not bracket the dominant kernel with events")
    ap.add_argument("--no-extras", action="store_true", help="skip the side measurements (bf16x3 / hp / cfg3 lines)")
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--laplacian-eps", type=float, default=None,
                    help="developer option: override the config's finite-difference eps (<= 0: exact Laplacian)")
    ap.add_argument("--config", default="cfg2", choices=sorted(ALT) + ["cfg4", "cfg5"],
                    help="cfg2 = the headline workload; cfg1 / cfg3: the other PDE configurations; cfg4 / cfg5: the "
                         "widened rows (dense kernel operator step; CDK towers + loss step), one GPU")
    ap.add_argument("--dp-exchange", default="auto", choices=["auto", "allreduce", "rs_ag", "a2a"],
                    help="N > 1, dp: gradient exchange (auto: each candidate is timed briefly, the fastest one takes "
                         "the headline run; all of them are reported in comm.candidates)")
    ap.add_argument("--grad-windows", type=int, default=None,
                    help="N > 1, dp: head windows of the backward (default: chosen per candidate)")
    ap.add_argument("--grad-buckets", type=int, default=4,
                    help="N > 1, dp, one backward window: gradient buckets (default 4; auto tries 4, 2 and 1)")
    ap.add_argument("--sync", action="store_true",
                    help="N > 1: blocking collectives on the compute stream (auto tries both)")
    ap.add_argument("--launch-timeout", type=float, default=1400.0,
                    help="--gpus N > 1 without a launcher: seconds before the rank processes are given up on")
    ap.add_argument("--collective-timeout", type=float, default=240.0,
                    help="N > 1: seconds a rank may sit in one collective before it gives up (the launcher then retries "
                         "with the plain exchange)")
    ap.add_argument("--amp", action="store_true",
                    help="--config cfg5: the mixed-precision mode (tower contractions on bfloat16-rounded operands, "
                         "float32 accumulation: FusedCdkStep(use_amp=True), the counterpart of the reference script's "
                         "default autocast branch); the line says so")
    ap.add_argument("--amp-dtype", default="bfloat16", choices=["bfloat16", "float16"],
                    help="--config cfg5 --amp: the half type. float16 = the reference's autocast dtype, run with its "
                         "GradScaler on the device (loss scaling, skipped steps, scheduler gate: FusedCdkStep)")
    ap.add_argument("--force-exchange", action="store_true",
                    help="developer option, --gpus 1 only: run the multi-GPU exchange sequences in an RCCL world of ONE "
                         "(every collective a real library call on the one GPU; the `comm` block then reads the "
                         "per-collective launch + wait cost with nothing on the wire). Never the headline.")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                    help="N = 1: also time the step replayed from a captured HIP graph (two steps per graph, the per-step "
                         "scalars in a device-resident nsvd_step_state; bit-identical to eager stepping). auto / on: both "
                         "are timed and reported, `value` is the faster (timing.mode says which); off: eager only")
    ap.add_argument("--accuracy", default="auto", choices=["auto", "on", "off"],
                    help="N = 1, headline workload: run the reference's full 500 000-step schedule and its 10^6-point "
                         "evaluation in this run (about 2.5 minutes) and report rel_eigenvalue_error as measured; auto = "
                         "on with --full for the headline workload on the default path; off: not measured")
    ap.add_argument("--tune-seconds", type=float, default=240.0,
                    help="N > 1: wall-time cap of the exchange tuner; when it hits, the candidates timed so far decide "
                         "and the table says so")
    ap.add_argument("--parallelism", default="auto", choices=["auto", "dp", "hp"],
                    help="N > 1: dp = samples sharded (moments all-reduce + gradient exchange: north_star's split); hp = "
                         "heads sharded (one all-gather of f, Tf, no gradient traffic) - the same global batch and the "
                         "same global step either way. auto: both are tuned and timed, the faster one takes the "
                         "headline run and the other is reported beside it (`other_sharding`)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: this process becomes the launcher (nothing has touched the GPU yet) and never computes
        return self_launch(args, sys.argv[1:])
    _claim_stdout()
    if args.config in ("cfg4", "cfg5"):
        if args.dump_outputs:
            raise SystemExit("--dump-outputs: the PDE configurations only (cfg1 / cfg2 / cfg3)")
        return bench_widened(args)

    from neural_svd_amd import hip_ops as H
    from neural_svd_amd import parallel

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # NSVD_FORCE_DEVICE / NSVD_DIST_BACKEND: developer aid to exercise the N > 1 code path on a 1-GPU box
    # (all ranks on one device, gloo instead of RCCL); never set by the driver
    if os.environ.get("NSVD_FORCE_DEVICE") is not None:
        local_rank = int(os.environ["NSVD_FORCE_DEVICE"])
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    multi = world > 1 or args.force_exchange
    if args.force_exchange:
        if world != 1:
            raise SystemExit("--force-exchange is a one-GPU developer option")
        import socket
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        os.environ.setdefault("MASTER_PORT", str(sock.getsockname()[1]))
        sock.close()
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    comm = parallel.Communicator.from_env(dev, backend=os.environ.get("NSVD_DIST_BACKEND"),
                                          timeout_s=args.collective_timeout) if multi else None
    if args.force_exchange:
        comm.force_exchange = True

    cfg = dict(ALT[args.config])
    if args.batch_size:
        cfg["B"] = args.batch_size
    if args.laplacian_eps is not None:
        cfg["eps"] = args.laplacian_eps
    headline = args.config == "cfg2" and args.laplacian_eps is None and not args.batch_size
    path = {"auto": H.PATH_AUTO, "generic": H.PATH_GENERIC, "fused": H.PATH_FUSED,
            "bf16x3": H.PATH_FUSED_BF16X3}[args.path]
    repeats = args.repeats or 1  # the headline: --steps timed steps
    side_repeats = args.repeats or max(3, min(25, round(6000 / max(args.steps, 1))))  # tuner and side measurements
    if args.parallelism == "hp" and cfg["L"] < world:
        raise SystemExit(f"hp needs at least one head per rank: L = {cfg['L']} < world size {world}")

    # N > 1: which sharding, which exchange? Every candidate is timed with the same protocol (fewer blocks) and the
    # fastest takes the headline run - the first hardware contact of this code decides, not a guess. What an RCCL
    # world of ONE already says (profiles/r03o_bench_rccl_world1*.json): a blocking collective costs ~16 us before a
    # byte moves, an asynchronous one ~25 us of compute-stream time (two cross-stream events), so fewer, larger
    # collectives compete with more overlap.
    def tune(par_t):
        """-> (best steps/s or None, trainer keywords of the best candidate, report)"""
        if par_t == "dp":
            if args.dp_exchange != "auto":
                return None, dict(dp_exchange=args.dp_exchange, grad_windows=args.grad_windows,
                                  grad_buckets=args.grad_buckets, sync=args.sync), None
            # (exchange, head windows of the backward (None: the trainer's rule), buckets when one window, blocking?)
            cands = [(ex, gw, nb, False) for ex in parallel.DP_EXCHANGES for gw, nb in ((None, 4), (1, 4), (1, 1))]
            cands += [("allreduce", 1, 2, False), ("allreduce", 1, 1, True), ("rs_ag", 1, 1, True), ("a2a", 1, 1, True)]
            named = [(f"{ex}/" + ("auto_windows" if gw is None else f"{gw}_window") +
                      (f"/{nb}_bucket" + ("s" if nb > 1 else "") if gw == 1 else "") + ("/blocking" if sy else ""),
                      dict(dp_exchange=ex, grad_windows=gw, grad_buckets=nb, sync=sy)) for ex, gw, nb, sy in cands]
        else:
            # hp: the all-gather asynchronous (next batch prepared under it) or blocking (next batch rides in the backward)
            if args.sync:
                return None, dict(sync=True), None
            named = [("all_gather/async", dict(sync=False)), ("all_gather/blocking", dict(sync=True))]
        report, best = {}, None
        for name, kw in named:
            # wall-time cap (every rank takes the same decision): the candidates timed so far decide
            if comm.max_float(time.perf_counter() - t_tune0) > args.tune_seconds and best is not None:
                report.setdefault("not_timed_tuner_cap", []).append(name)
                continue
            try:
                t, _, _ = make_trainer(cfg, par_t, comm, dev, path, **kw)
                nwin = len(t._windows)
                if par_t == "dp" and kw["grad_windows"] is None and nwin == 1:
                    del t
                    continue  # same thing as the explicit 1-window candidate
                bl, _, _, _ = run_timed(t, comm, args.steps, args.warmup, max(3, side_repeats // 4), 0.3, 0)
                d = summarize(bl, args.steps, world)
                report[name] = dict(steps_per_s=d["value"], ms_per_step=d["ms_per_step"])
                if name in pre_timed:
                    report[name]["also"] = "north_star_split"
                if par_t == "dp":
                    report[name].update(windows=nwin, buckets=len(t.grad_buckets()))
                if best is None or d["value"] > best[0]:
                    best = (d["value"], kw, name)
                del t
                torch.cuda.empty_cache()
            except Exception as e:  # noqa: BLE001  (constructor refusals are the same on every rank)
                report[name] = {"error": f"{type(e).__name__}: {e}"}
        if best is None:
            return None, {}, report
        report["chosen"] = best[2]
        if "not_timed_tuner_cap" in report:
            report["tuner_capped_after_s"] = args.tune_seconds
        return best[0], best[1], report

    par, tr_kw, cand_report, other_sharding, tuned = args.parallelism, {}, None, None, {}
    t_tune0 = time.perf_counter()
    pre_timed, north_star = set(), None
    if multi and args.full and not args.no_extras:
        # FIRST, whatever wins below: north_star's literal split - samples sharded, ONE all-reduce of the 2L^2+1 moment
        # floats and ONE all-reduce of the flat gradient per step, blocking calls on the compute stream - so that the
        # curve the contract names is on every N > 1 line
        try:
            kw_ns = dict(dp_exchange="allreduce", grad_windows=1, grad_buckets=1, sync=True)
            t, _, _ = make_trainer(cfg, "dp", comm, dev, path, **kw_ns)
            bl, _, _, _ = run_timed(t, comm, args.steps, args.warmup, max(3, side_repeats // 4), 0.3, 0)
            north_star = summarize(bl, args.steps, world, cfg["B"])
            north_star.update(unit="steps/s", parallelism=f"dp{world}", final_loss=float(t.loss[0]),
                              params_finite=bool(torch.isfinite(t.P.flat).all()),
                              exchange="samples sharded; one all-reduce of the 2L^2+1 moments + one all-reduce of the "
                                       "flat gradient per step (one bucket, one backward window), blocking",
                              flags="--parallelism dp --dp-exchange allreduce --grad-windows 1 --grad-buckets 1 --sync")
            pre_timed.add("allreduce/1_window/1_bucket/blocking")
            del t
            torch.cuda.empty_cache()
            if rank == 0 and "value" in north_star:
                # from here on a line exists: should the tuning or a later measurement die (a collective that times out
                # raises on every rank), rank 0 prints THIS - north_star's literal split, measured - instead of nothing
                _PROVISIONAL.clear()
                _PROVISIONAL.update({
                    "metric": f"training steps/sec, 2D hydrogen L=16 B=512 per GPU (NestedLoRA joint nesting, full "
                              f"optimiser step), weak scaling: value = n_gpus x optimiser steps/s of the global batch of "
                              f"{cfg['B'] * world} rows",
                    "value": north_star["value"], "unit": "steps/s", "n_gpus": world, "steps": args.steps,
                    "warmup": args.warmup, "ms_per_step": north_star["ms_per_step"], "higher_is_better": True,
                    "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                    "config": {"workload": "configs[1]: 2D hydrogen, L=16, batch_size=512 per GPU, joint nesting",
                               "global_batch": cfg["B"] * world, "parallelism": f"dp{world}",
                               "sharding": north_star["exchange"]},
                    "optimizer_steps_per_s": north_star["optimizer_steps_per_s"],
                    "samples_per_s": north_star["samples_per_s"], "global_batch": north_star["global_batch"],
                    "final_loss": north_star["final_loss"], "params_finite": north_star["params_finite"],
                    "north_star_split": north_star, "roofline": None, "cpu_baseline": None})
        except Exception as e:  # noqa: BLE001
            north_star = {"error": f"{type(e).__name__}: {e}"}
    if multi:
        pars = [args.parallelism] if args.parallelism != "auto" else \
            (["dp", "hp"] if cfg["L"] >= world else ["dp"])  # (any L >= world: parallel.head_range)
        tuned = {p_: tune(p_) for p_ in pars}
        par = max(pars, key=lambda p_: tuned[p_][0] or 0.0) if len(pars) > 1 else pars[0]
        _, tr_kw, cand_report = tuned[par]
        if len(pars) > 1:  # the sharding that lost: its best candidate is the side line
            o = "hp" if par == "dp" else "dp"
            other_sharding = dict(parallelism=f"{o}{world}", steps_per_s=tuned[o][0], candidates=tuned[o][2])
    elif par == "auto":
        par = "dp"
    exchange, sync = tr_kw.get("dp_exchange", "allreduce"), tr_kw.get("sync", False)
    tr, shape, prob = make_trainer(cfg, par, comm, dev, path, **tr_kw)
    # the same step replayed from a captured HIP graph (N = 1, MFMA path): the learning rate, EMA decay and batch
    # counter live in a device-resident nsvd_step_state advanced by the step's own kernels (trainer.GraphedSteps). Captured
    # before anything is timed: the capture may take the first step eagerly (`lead`), which then counts as warm-up, so
    # that both timed trainers have taken the same number of steps when their timed blocks end
    trg = gstep = None
    lead, graph_err = 0, None
    if not multi and args.graph != "off" and H.path_name(tr.shape, tr.B, path, prob) == "fused_mfma":
        try:
            trg, _, _ = make_trainer(cfg, par, None, dev, path, device_schedule=True)
            gstep = GraphStepper(trg)
            lead = trg.t
        except Exception as e:  # noqa: BLE001
            graph_err = f"{type(e).__name__}: {e}"
            if args.graph == "on":
                raise
            trg = gstep = None
    warmup = max(args.warmup, lead)
    prewarm_spent, n_pre = prewarm(cfg, par, comm, dev, path, args.prewarm_seconds, **tr_kw)

    use_ev = not args.no_kernel_events
    EV_EVERY = 4  # bracket the dominant kernel on every 4th timed step (two event records cost ~2 us)
    blocks, kms, _, _ = run_timed(tr, comm, args.steps, warmup, repeats, None, EV_EVERY if use_ev else 0)
    summ = summarize(blocks, args.steps, world, cfg["B"])
    modes = {"eager": dict(summ, note="three launches per step from Python (ctypes), the per-step scalars as launch "
                                      "arguments" + ("; every 4th step carries the two event records of the kernel "
                                                     "bracket" if use_ev else ""))}
    timing_mode, timed_tr = "eager", tr
    if gstep is not None:
        try:
            bg, _ = run_timed_graph(trg, args.steps, warmup - lead, repeats, None, stepper=gstep)
            sg = summarize(bg, args.steps, 1, cfg["B"])
            modes["hip_graph_replay"] = dict(sg, steps_per_graph=2, final_loss=float(trg.loss[0]),
                                             params_finite=bool(torch.isfinite(trg.P.flat).all()),
                                             note="one hipGraphLaunch per two steps; bit-identical to eager stepping "
                                                  "(tests/test_graph_gpu.py)")
            if sg["value"] > summ["value"]:
                summ, timing_mode, timed_tr = sg, "hip_graph_replay", trg
        except Exception as e:  # noqa: BLE001
            graph_err = f"{type(e).__name__}: {e}"
            if args.graph == "on":
                raise
    if args.dump_outputs:
        if getattr(timed_tr, "_state_sharded", False):
            timed_tr.gather_optimizer_state()  # (a collective: every rank)
        if rank == 0:
            dump_outputs(args.dump_outputs, trainer_outputs(timed_tr))
    if args.full and "hip_graph_replay" in modes:
        # per-step host sync on the loss, as the reference's loop does (loss.item(), operator/__init__.py:74)
        try:
            for _ in range(20):
                trg.step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            nsync = max(200, min(2000, args.steps))
            acc = 0.0
            for _ in range(nsync):
                trg.step()
                acc += float(trg.loss[0])
            el = time.perf_counter() - t1
            modes["eager_with_loss_item_every_step"] = dict(
                value=round(nsync / el, 3), ms_per_step=round(1e3 * el / nsync, 4), steps=nsync,
                note="eager steps + float(loss) after each (the reference's per-step host sync); the loss VALUE is "
                     "produced by the step's own kernels in every mode")
        except Exception as e:  # noqa: BLE001
            graph_err = f"{type(e).__name__}: {e}"
    del trg, gstep, timed_tr
    torch.cuda.empty_cache()
    loss = float(tr.loss[0])
    finite = bool(torch.isfinite(tr.P.flat).all())
    fused_step, tr_hp, n_train, trB, trL = tr.fused_step, tr.hp, tr.P.n_trainable, tr.B, tr.shape.L
    path_name = H.path_name(tr.shape, tr.B, path, prob)
    comm_block = None
    rccl_ranks = comm.count_ranks() if multi else None
    if multi and args.full:
        # where the multi-GPU step's time goes: (1) the exposed wait of every collective, from events on the compute
        # stream around each wait (parallel.CommProbe), over PROBE_STEPS further steps of the same trainer; (2) the
        # same step with every collective skipped (compute_only_ms; replicas drift apart, which timing does not mind)
        PROBE_STEPS = 100
        tr.probe = parallel.CommProbe(dev)
        for _ in range(PROBE_STEPS):
            tr.step()
        waits = tr.probe.summary()
        tr.probe = None
        waits_max = {k: round(comm.max_float(v), 2) for k, v in waits.items()}
        buckets = [int(4 * (hi - lo)) for lo, hi in tr.grad_buckets()] if not tr_hp else []
        nwin = len(tr._windows)
        comm.barrier()
        comm.stub = True
        bl, _, _, _ = run_timed(tr, comm, args.steps, args.warmup, max(3, side_repeats // 4), 0.2, 0)
        comm.stub = False
        co = summarize(bl, args.steps, world, cfg["B"])
        comm_block = {
            "backend": comm.backend, "exchange": ("all_gather of f, Tf" if tr_hp else exchange),
            "collectives": "blocking, on the compute stream" if sync else "asynchronous, waited for as late as possible",
            "backward_windows": nwin, "grad_bucket_bytes": buckets,
            "moment_floats": 2 * cfg["L"] * cfg["L"] + 1,
            "exposed_wait_us_per_step": {k: round(v, 2) for k, v in waits.items()},
            "exposed_wait_us_per_step_max_over_ranks": waits_max,
            "exposed_wait_us_total": round(sum(waits.values()), 2),
            "probe_steps": PROBE_STEPS,
            "compute_only_ms": co["ms_per_step"], "compute_only_steps_per_s": co["value"],
            "step_ms": summ["ms_per_step"],
            "note": "exposed wait = time the compute stream sat idle for that collective (two events around each "
                    "wait on the compute stream, rank 0; max over ranks beside it); compute_only = the same step "
                    "with every collective skipped",
            "candidates": cand_report,
        }
    del tr
    torch.cuda.empty_cache()

    # side measurements (never `value`): same protocol, fewer blocks
    extras = {}

    def side(name, cfg_s, par_s, path_s, note):
        """a side line: the same protocol with fewer blocks. Multi-rank: dp lines run with the headline's chosen
        exchange when that was dp (else the default one), hp lines time the all-gather both ways and keep the faster."""
        same_cfg = cfg_s is cfg
        if not multi:
            variants = [("", {})]
        elif same_cfg and par_s in tuned and tuned[par_s][1]:
            variants = [(tuned[par_s][2]["chosen"] if tuned[par_s][2] else "as given", tuned[par_s][1])]
        elif par_s == "hp":
            variants = [("all_gather/async", dict(sync=False)), ("all_gather/blocking", dict(sync=True))]
        elif "dp" in tuned and tuned["dp"][1]:
            variants = [("configs[1]'s chosen exchange: " + (tuned["dp"][2] or {}).get("chosen", "as given"),
                         tuned["dp"][1])]
        else:
            variants = [("allreduce/auto_windows", {})]
        best, tried = None, {}
        for vname, kw in variants:
            try:
                t, _, _ = make_trainer(cfg_s, par_s, comm, dev, path_s, **kw)
                bl, _, _, _ = run_timed(t, comm, args.steps, args.warmup, max(3, side_repeats // 3), 0.3, 0)
                d = summarize(bl, args.steps, world, cfg_s["B"])
                d.update(unit="steps/s", final_loss=float(t.loss[0]),
                         params_finite=bool(torch.isfinite(t.P.flat).all()), global_batch=cfg_s["B"] * world, note=note)
                fl, _ = algorithmic_flops(cfg_s, cfg_s["B"])
                d["step_tflops_per_gpu"] = round(fl / (d["ms_per_step"] * 1e-3) / 1e12, 3)
                tried[vname] = d["value"]
                if best is None or d["value"] > best["value"]:
                    best = d
                    best["exchange"] = vname
                del t
                torch.cuda.empty_cache()
            except Exception as e:  # noqa: BLE001  (constructor refusals are the same on every rank)
                tried[vname] = f"{type(e).__name__}: {e}"
        if best is None:
            extras[name] = {"error": "; ".join(f"{k}: {v}" for k, v in tried.items())}
            return
        if len(variants) > 1:
            best["variants_steps_per_s"] = tried
        if not multi:
            best.pop("exchange", None)
        extras[name] = best

    if args.full and not args.no_extras and headline and args.path == "auto":
        if world == 1 and args.force_exchange:
            side("sharding_hp", cfg, "hp", path, "heads 'sharded' over a world of one: the all-gather of f, Tf as an "
                                                 "RCCL call with nothing on the wire")
        elif world == 1:
            side("opt_in_path_bf16x3", cfg, "dp", H.PATH_FUSED_BF16X3,
                 "same workload with NSVD_PATH_FUSED_BF16X3: every layer of the forward as three-way split bf16 "
                 "products accumulated in float32 (the stencil columns as centre + even / odd perturbations: "
                 "DESIGN.md 3.5, 3.2) - against float64 its f is closer than the native fp32 MFMA path's and its Tf "
                 "within 1e-5 (the reference's own float32 arithmetic: 4e-2; accuracy_vs_float64 below), same "
                 "backward; not the headline value, which stays native float32 arithmetic")
            try:
                extras["opt_in_path_bf16x3"]["agreement_of_the_hip_paths"] = measure_path_agreement(cfg, dev)
            except Exception as e:  # noqa: BLE001
                extras["opt_in_path_bf16x3"]["agreement_of_the_hip_paths"] = {"error": f"{type(e).__name__}: {e}"}
        else:
            other = "hp" if par == "dp" else "dp"
            if other == "dp" or cfg["L"] >= world:
                side(f"sharding_{other}", cfg, other, path,
                     "same workload and global batch, heads sharded instead of samples: one all-gather of f, Tf per "
                     "step, no gradient traffic (DESIGN.md 6)" if other == "hp" else
                     "same workload and global batch, samples sharded: moments all-reduce + gradient exchange")
                if other_sharding is not None:
                    extras[f"sharding_{other}"]["candidates"] = other_sharding["candidates"]
            # BASELINE configs[2] as BASELINE states it: global batch 4096 at every N (STRONG scaling, 4096 / N rows per
            # GPU): the curve the 1 -> 8 target is named on; optimizer_steps_per_s is the figure (N = 1: other_configs)
            if 4096 % world == 0 and (4096 // world) % 32 == 0:
                c3s = dict(ALT["cfg3"], B=4096 // world)
                side("_strong_dp", c3s, "dp", path, "samples sharded")
                if c3s["L"] >= world:
                    side("_strong_hp", c3s, "hp", path, "heads sharded")
                block = {"workload": "configs[2]: 2D harmonic oscillator, L=32, sequential nesting, GLOBAL batch 4096 "
                                     f"({4096 // world} rows per GPU)", "global_batch": 4096, "n_gpus": world,
                         "scaling": "strong"}
                best = None
                for key, nm in (("_strong_dp", "dp"), ("_strong_hp", "hp")):
                    e = extras.pop(key, None)
                    if e is None:
                        continue
                    if "error" in e:
                        block[nm] = e
                        continue
                    block[nm] = dict(optimizer_steps_per_s=e["optimizer_steps_per_s"], ms_per_step=e["ms_per_step"],
                                     final_loss=e["final_loss"], params_finite=e["params_finite"],
                                     exchange=e.get("exchange"))
                    if best is None or e["optimizer_steps_per_s"] > best[1]:
                        best = (nm, e["optimizer_steps_per_s"])
                if best is not None:
                    block.update(optimizer_steps_per_s=best[1], parallelism=f"{best[0]}{world}")
                extras["strong_scaling_configs2"] = block
            c3 = ALT["cfg3"]
            side("cfg3_dp", c3, "dp", path,
                 "configs[2]: 2D harmonic oscillator, L=32, sequential nesting, 512 rows per GPU (global batch 4096 at "
                 "8 GPUs), samples sharded")
            if c3["L"] >= world:
                side("cfg3_hp", c3, "hp", path, "configs[2], heads sharded")

    if rank != 0:
        if comm is not None:
            comm.close()
        return
    ms_per_step, value = summ["ms_per_step"], summ["value"]
    flops_step, flops_fwd = algorithmic_flops(cfg, cfg["B"])
    roof = None
    if use_ev and kms:
        kavg = sum(kms) / len(kms)
        kname = H.dominant_kernel_name(shape, cfg["B"], path)
        ach = flops_fwd / (kavg * 1e-3) / 1e12
        nh = len(cfg["hidden"])
        alg_mb = 4.0 * (n_train + cfg["B"] * 2 * cfg["m"] + nh * trL * cfg["hidden"][0] * trB + 3 * trB * trL) / 1e6
        traffic, traffic_src, busy = None, "profiles/", None
        try:  # HBM bytes per launch / MFMA-busy fraction from the committed rocprofv3 --pmc passes, same workload only
            tj = json.load(open(os.path.join(ROOT, "profiles", "latest_traffic.json")))
            if tj.get("workload") == "cfg2" and headline and kname.startswith("pmlp_fused_fwd"):
                k = tj["kernels"]["pmlp_fused_fwd"]
                traffic = int(k["hbm_bytes_corrected"])
                busy = k.get("mfma_busy_frac")
                traffic_src = tj.get("source", "profiles/")
        except Exception:  # noqa: BLE001
            traffic = None
        roof = dict(bound="mfma", achieved=round(ach, 3), peak=PEAK_FP32_MFMA_TFLOPS, unit="TFLOP/s",
                    frac=round(ach / PEAK_FP32_MFMA_TFLOPS, 4), traffic=traffic,
                    traffic_note=f"HBM-side bytes per launch (2*FETCH_SIZE + WRITE_SIZE, gfx950 correction) from "
                                 f"{traffic_src}; algorithmic bytes {alg_mb:.1f} MB (parameters + centre features "
                                 f"read once, saved activations + f, Tf, jac written once)",
                    mfma_busy_frac=busy,
                    kernel=kname, kernel_avg_us=round(kavg * 1e3, 2), kernel_med_us=round(kms[len(kms) // 2] * 1e3, 2),
                    kernel_launches_timed=len(kms), kernel_flops=flops_fwd,
                    step_flops=flops_step, step_tflops=round(flops_step / (ms_per_step * 1e-3) / 1e12, 3),
                    step_frac=round(flops_step / (ms_per_step * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4))
    sharding = {"dp": "samples: each GPU draws its own 512 rows; all-reduce of the 2L^2+1 moments, then the flat "
                      "gradient in buckets (head windows of the backward), " +
                      {"allreduce": "optimiser on bucket k under the all-reduce of k+1",
                       "rs_ag": "reduce-scatter, optimiser on this rank's 1/N of each bucket, all-gather of the parameters",
                       "a2a": "slice j of each bucket straight to rank j (all-to-all), optimiser on this rank's 1/N, "
                              "updated slices straight to every rank (all-to-all)"}[exchange],
                "hp": "heads: each GPU owns L/N heads and evaluates them on the whole global batch; one all-gather "
                      "of f,Tf per step, no gradient traffic"}
    out = {
        "metric": "training steps/sec, 2D hydrogen L=16 B=512 (NestedLoRA joint nesting, full optimiser step)",
        "value": value, "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "timing": {"protocol": "prewarm (a throwaway trainer of the same configuration), then --warmup steps, then "
                               "`blocks` timed blocks of exactly --steps steps (barrier + synchronize on both sides, "
                               "max over ranks); value = median block",
                   "mode": timing_mode, "modes": modes,
                   "loss_every_step": "the loss value of every step is produced on the device by the step's own "
                                      "kernels (no extra launch, no host sync in the timed region)",
                   "blocks": summ["blocks"], "ms_per_step_min": summ["ms_per_step_min"],
                   "ms_per_step_max": summ["ms_per_step_max"], "prewarm_s": round(prewarm_spent, 3),
                   "prewarm_steps": n_pre},
        "config": {"workload": "configs[1]: 2D hydrogen, L=16, batch_size=512 per GPU, joint nesting, "
                               "MLP 2048(Fourier m=1024)->128->128->128->1 x16 heads, eps=0.01, RMSprop+cosine+EMA",
                   "global_batch": cfg["B"] * world,
                   "parallelism": (f"{par}{world}" if multi else "dp1"),
                   "sharding": sharding[par] if multi else "single GPU: no exchange",
                   "optimiser": ("RMSprop+EMA step fused into the weight-gradient kernel" if fused_step else
                                 "separate RMSprop+EMA kernel per gradient bucket after its all-reduce"),
                   "path": path_name, "params": n_train * (world if tr_hp else 1)},
        "final_loss": loss, "params_finite": finite,
        "roofline": roof,
    }
    if len(tuned) > 1:
        out["config"]["parallelism_tuned"] = {f"{p_}{world}": tuned[p_][0] for p_ in tuned}
        out["config"]["parallelism_note"] = ("--parallelism auto: both shardings of the same global step were tuned and "
                                             "timed (steps/s above), the faster one ran the headline; the other is the "
                                             f"side line sharding_{'hp' if par == 'dp' else 'dp'}")
    if graph_err is not None:
        out["timing"]["graph_error"] = graph_err
    if multi:
        # what `value` is at N > 1 - said in `metric` itself - and the two unambiguous rates beside it
        out["metric"] = (f"training steps/sec, 2D hydrogen L=16 B=512 per GPU (NestedLoRA joint nesting, full optimiser "
                         f"step), weak scaling: value = n_gpus x optimiser steps/s of the global batch of "
                         f"{cfg['B'] * world} rows = 512-row batches stepped on per second over all GPUs")
        out["value_is"] = (f"n_gpus x optimizer_steps_per_s = per-GPU batches of {cfg['B']} rows stepped on per second "
                           f"over all GPUs (weak scaling: one optimiser step consumes the global batch of "
                           f"{cfg['B'] * world} rows); scaling efficiency = value(N) / (N x value(1))")
        out["optimizer_steps_per_s"] = summ["optimizer_steps_per_s"]
        out["samples_per_s"] = summ["samples_per_s"]
        out["global_batch"] = summ["global_batch"]
        if north_star is not None:
            out["north_star_split"] = north_star
        out["rccl_ranks"] = rccl_ranks
        out["comm"] = comm_block
    else:
        out["optimizer_steps_per_s"] = summ["optimizer_steps_per_s"]
        out["samples_per_s"] = summ["samples_per_s"]
        out["global_batch"] = summ["global_batch"]
    if args.force_exchange:
        out["metric"] += " [developer run: exchange sequences forced on in an RCCL world of one]"
    # the other half of BASELINE.json's metric: eigenvalue error after the reference's full schedule, MEASURED in this
    # run (N = 1, headline workload, default path) or absent - nothing on this line is quoted from an earlier run
    want_acc = headline and not multi and (args.accuracy == "on" or (args.accuracy == "auto" and args.full and
                                                                   not args.force_exchange and args.path == "auto"))
    if want_acc:
        try:
            acc = measure_accuracy(cfg, dev, path, graph=(args.graph != "off" and path_name == "fused_mfma"))
            acc["reference_published"] = {
                "NeuralSVD-jnt 2D hydrogen": "about 1.2e-2 .. 2e-2 (read off figs/hydrogen_eval.png, log scale, +-30 %)",
                "NeuralSVD-seq 2D hydrogen": "about 6e-3 .. 9e-3", "source": "BASELINE.md"}
            out["rel_eigenvalue_error"] = acc
        except Exception as e:  # noqa: BLE001
            out["rel_eigenvalue_error"] = {"error": f"{type(e).__name__}: {e}"}
    if headline:
        out["eigenvalue_parity"] = ("identical weights, identical grid: every one of the 16 Rayleigh quotients of the HIP "
                                    "path within 1e-4 of the float64 oracle's - asserted by "
                                    "tests/test_spectrum_parity_gpu.py in the GPU suite (the oracle is test "
                                    "infrastructure: this script does not import it outside cpu_baseline)")
    if not headline:
        out["metric"] = f"training steps/sec, developer config {args.config} (not the headline workload)"
        out["config"]["workload"] = f"{args.config}: {cfg}"
    if args.path == "bf16x3":
        out["metric"] += " [developer path: layer 0 as bf16x3 split products, fp32 accumulation]"
        out["config"]["layer0"] = ("bf16 MFMA, operands split into 3 bf16 planes, 6 partial products, fp32 "
                                   "accumulate; roofline.frac stays relative to the fp32 MFMA peak")
    out.update(extras)
    if args.full and world == 1 and headline and args.path == "auto" and not args.no_extras and not args.force_exchange:
        out["other_configs"] = measure_other_configs(args, dev)
    if args.full and world == 1 and not args.no_cpu_baseline and args.config == "cfg2" and not args.force_exchange:
        cb = cpu_baseline()
        out["cpu_baseline"] = cb
        out["speedup_vs_cpu_baseline"] = round(value / cb["value"], 1)
    else:
        out["cpu_baseline"] = None
    _emit(out)
    if comm is not None:
        comm.close()



_JSON_FD = None


def _claim_stdout():
    """a process that computes keeps stdout for the ONE JSON line: file descriptor 1 is pointed at stderr for everything
    else - native libraries write to it through C stdio (RCCL prints a five-line version banner there) - and the line
    goes out through a private duplicate of the original descriptor (_emit)"""
    global _JSON_FD
    if _JSON_FD is None:
        sys.stdout.flush()
        _JSON_FD = os.dup(1)
        os.dup2(2, 1)


def _emit(line):
    """the ONE JSON line, the only thing on the process's original stdout (_claim_stdout)"""
    data = (json.dumps(line) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(data.decode())
        sys.stdout.flush()
    else:
        os.write(_JSON_FD, data)


def launcher_worst_case_seconds(launch_timeout, n_attempts=3):
    """upper bound of `python bench.py --gpus N` from its own clocks: the ladder's attempts share --launch-timeout
    (self_launch: 1 / 0.6 + 0.4 / 0.5 + 0.25 + 0.25 of it), each attempt is killed at its share; + the poll interval
    and process start / teardown of every attempt"""
    shares = {1: [1.0], 2: [0.6, 0.4], 3: [0.5, 0.25, 0.25]}[n_attempts]
    return sum(launch_timeout * sh for sh in shares) + n_attempts * (0.2 + _KILL_GRACE_S + 15.0)


def run_main():
    """main(); a multi-rank run that dies after its first measured split still prints that split's line, marked
    `degraded`, and exits with DEGRADED_RC: the line is a measurement, the exit code says the run failed"""
    try:
        main()
    except Exception as e:  # noqa: BLE001
        if _PROVISIONAL:
            _PROVISIONAL["degraded"] = (f"the run died after its first measured split ({type(e).__name__}: {e}); this is "
                                        f"north_star's literal split (samples sharded, one moments all-reduce + one "
                                        f"gradient all-reduce per step, blocking), measured before that")
            _emit(_PROVISIONAL)
            os._exit(DEGRADED_RC)  # (no teardown of a process group whose collectives are failing)
        raise


if __name__ == "__main__":
    run_main()
