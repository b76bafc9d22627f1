"""The optimiser rules of csrc/opt_math.h - SGD with / without momentum, RMSprop with momentum, Adam, and the RMSprop
update the kernels have always run - compiled for the HOST (g++, float32, the same source file through the stand-in
header tests/_opt_math_host/nsvd_common.h) and held to the float64 oracle tests/_optim_oracle.py over 12 scheduled
steps, in the host-scalar form (nsvd_make_opt_hyper) and the device-state form (nsvd_opt_state_derive, Adam's bias
corrections and SGD's first-step flag moving with `step`). Bound: rel < 1e-6 on p, every state slot and the EMA - the
bound tests/test_hip_parity.py holds the float32 RMSprop kernel to, and the one the GPU tests of these rules use.
Compiled with -ffp-contract=off: every float32 operation rounds once, which is what lets the last test restate
nsvd_rmsprop_upd in numpy and ask for its bits."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _optim_oracle as OO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NZERO, STEPS, T_MAX, LR0, ALPHA, DECAY = 10007, 512, 12, 30, 1e-3, 0.999, 0.995
CASES = [("sgd", 0.0), ("sgd", 0.9), ("rmsprop", 0.0), ("rmsprop", 0.9), ("adam", 0.0)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    from neural_svd_amd import _lib  # noqa: F401  (the ctypes mirror of nsvd_opt_config)
    td = str(tmp_path_factory.mktemp("opt_math_host"))
    for src in (os.path.join(ROOT, "neural_svd_amd", "csrc", "opt_math.h"), os.path.join(ROOT, "include", "nsvd.h"),
                os.path.join(ROOT, "tests", "_opt_math_host", "nsvd_common.h"),
                os.path.join(ROOT, "tests", "_opt_math_host", "harness.cpp")):
        shutil.copy(src, td)
    out = os.path.join(td, "libopthost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fPIC", "-shared",
                           os.path.join(td, "harness.cpp"), "-o", out])
    so = C.CDLL(out)
    so.opt_rule_of.argtypes = [C.c_int, C.c_double]
    return so


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal(N).astype(np.float32)
    grads = np.stack([rng.standard_normal(N) * (1.0 + 0.3 * t) for t in range(STEPS)]).astype(np.float32)
    grads[:, 1000:1000 + NZERO] = 0.0  # a block of elements whose gradient is exactly zero throughout
    return p0, grads


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _config(kind, momentum, eps):
    from neural_svd_amd import _lib
    c = _lib.OptConfig()
    c.kind = {"rmsprop": _lib.OPT_RMSPROP, "sgd": _lib.OPT_SGD, "adam": _lib.OPT_ADAM}[kind]
    c.lr, c.alpha, c.eps, c.momentum, c.beta1, c.beta2, c.ema_decay = LR0, ALPHA, eps, momentum, 0.9, 0.999, DECAY
    return c


@pytest.mark.parametrize("use_state", [0, 1])
@pytest.mark.parametrize("with_ema", [True, False])
@pytest.mark.parametrize("kind,momentum", CASES)
def test_host_rules_match_the_oracle(lib, data, kind, momentum, with_ema, use_state):
    p0, grads = data
    eps = 1e-8 if kind == "adam" else 1e-10
    gs = 0.25 if (kind == "adam" and with_ema) else 1.0  # one case with grad_scale on 4 x gradients
    want = OO.run(kind, momentum, p0.astype(np.float64), [g.astype(np.float64) for g in grads], LR0, T_MAX, ALPHA, eps,
                  (0.9, 0.999), DECAY if with_ema else None)
    has_sq, has_mom = OO.uses(kind, momentum)
    p = p0.copy()
    sq = np.zeros(N, np.float32) if has_sq else None
    # SGD's first step must not read the buffer: hand it garbage
    mom = (np.full(N, 7.0, np.float32) if kind == "sgd" else np.zeros(N, np.float32)) if has_mom else None
    ema = p0.copy() if with_ema else None
    lr = (C.c_double * STEPS)(*[OO.cosine_lr(LR0, t, T_MAX) for t in range(STEPS)])
    dec = (C.c_double * STEPS)(*[OO.ema_decay_at(DECAY, t + 1) for t in range(STEPS)])
    g_in = np.ascontiguousarray(grads / np.float32(gs))
    cfg = _config(kind, momentum, eps)
    took = lib.run_rule(C.byref(cfg), C.c_double(0.0), C.c_ulonglong(T_MAX), use_state, lr, dec, C.c_double(gs), N,
                        STEPS, _ptr(g_in), _ptr(p), _ptr(sq), _ptr(mom), _ptr(ema))
    assert took == STEPS
    figures = {"p": rel(p, want.p)}
    if has_sq:
        figures["sq"] = rel(sq, want.sq)
    if has_mom:
        figures["mom"] = rel(mom, want.mom)
    if with_ema:
        figures["ema"] = rel(ema, want.ema)
    print(kind, momentum, with_ema, use_state, figures)
    assert all(v < 1e-6 for v in figures.values()), figures
    z = slice(1000, 1000 + NZERO)
    assert np.array_equal(p[z], p0[z]) and np.isfinite(p).all()
    for s in (sq, mom, ema):
        assert s is None or np.isfinite(s).all()


def test_unknown_kind_has_no_rule(lib):
    from neural_svd_amd import _lib
    assert lib.opt_rule_of(_lib.OPT_RMSPROP, 0.0) == 0 and lib.opt_rule_of(_lib.OPT_RMSPROP, 0.9) == 1
    assert lib.opt_rule_of(_lib.OPT_SGD, 0.0) == 2 and lib.opt_rule_of(_lib.OPT_SGD, 0.5) == 3
    assert lib.opt_rule_of(_lib.OPT_ADAM, 0.0) == 4 and lib.opt_rule_of(_lib.OPT_ADAM, 0.9) == 4
    assert lib.opt_rule_of(3, 0.0) == -1 and lib.opt_rule_of(-1, 0.0) == -1


@pytest.mark.parametrize("has_ema", [1, 0])
def test_rmsprop_upd_keeps_its_bits(lib, data, has_ema):
    """nsvd_rmsprop_upd against the same float32 sequence written here: one rounding per operation, in its order"""
    p0, grads = data
    f = np.float32
    lr, alpha, oma, eps, omd, gs = f(1e-3), f(0.999), f(1.0 - 0.999), f(1e-10), f(1.0 - 0.995), f(0.5)
    hyper = np.array([lr, alpha, oma, eps, omd, gs], np.float32)
    p, sq, ema = p0.copy(), np.zeros(N, np.float32), p0.copy()
    lib.run_rmsprop_upd(_ptr(hyper), has_ema, N, STEPS, _ptr(np.ascontiguousarray(grads)), _ptr(p), _ptr(sq), _ptr(ema))
    rp, rsq, rema = p0.copy(), np.zeros(N, np.float32), p0.copy()
    for t in range(STEPS):
        g = grads[t] * gs
        rsq = alpha * rsq + oma * (g * g)
        avg = np.sqrt(rsq) + eps
        rp = rp - lr * (g / avg)
        if has_ema:
            rema = rema - omd * (rema - rp)
    assert rp.dtype == np.float32 and rsq.dtype == np.float32
    assert np.array_equal(p, rp) and np.array_equal(sq, rsq) and np.array_equal(ema, rema)
