"""CPU-only: every entry point that takes a workspace refuses one that is too small or not 256-byte aligned, and every
workspace size query returns what it returned before the shared arena.

As in test_evd_backward_refusals.py the descriptors are real and the device pointers are made-up (non-null, 256-byte
aligned, distinct) addresses that nothing dereferences: a refused call returns from the host code before any HIP call.
An ACCEPTED call would launch kernels on those addresses, so the module skips itself where a GPU is visible - it runs on
a machine without one and nowhere else.

Each entry point gets one small valid shape; `need` is what its own *_workspace_bytes query returns for it. Two calls:
the workspace one byte short, and a sufficient workspace whose base is off by 128 bytes; both NSVD_EINVAL. The two
entry points of csrc/cdk_loss.hip had no alignment check before csrc/nsvd_common.h's nsvd_ws_ok (found by reading them).

SIZES was RECORDED from a build of the commit that preceded the shared arena (NsvdArena), not from the code under test:
the small shapes of the calls and one larger shape per family (B = 8192, L = 64, D = 3 where they apply)."""
import ctypes as C

import pytest
import torch

from neural_svd_amd import _lib
from neural_svd_amd._lib import EINVAL

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="an accepted call would launch on made-up addresses: no-GPU machines only")

L, D, M_FEATURES, B = 16, 2, 1024, 512
HIDDEN = (128, 128, 128)


def _fake(i):
    """a made-up device address: non-null, 256-byte aligned, distinct per i (16 MB apart)"""
    return 0x7F0000000000 + 0x1000000 * i


WS, WS_NEXT = _fake(60), _fake(80)


def _desc(l=L, d=D, m=M_FEATURES, hidden=HIDDEN):
    s = _lib.ModelDesc()
    s.L, s.D, s.m = l, d, m
    dims = tuple(hidden) + (1,)
    s.nlayers = len(dims)
    for i, h in enumerate(dims):
        s.dims[i] = h
    return s


def _param_set(nlayers, base, fourier=True):
    p = _lib.Params()
    if fourier:
        p.fourier_B = _fake(base)
    for i in range(nlayers):
        p.W[i] = _fake(base + 1 + 2 * i)
        p.b[i] = _fake(base + 2 + 2 * i)
    return p


def _problem():
    q = _lib.Problem()
    q.potential, q.charge_or_k, q.scale_kinetic, q.eps = _lib.POT_HYDROGEN, 1.0, 1.0, 0.01
    q.op_scale, q.sigma, q.hard_mul_const, q.use_importance = 100.0, 16.0, 1.0, _lib.IMP_GAUSSIAN
    return q


def _rmsprop(nlayers):
    o = _lib.Rmsprop()
    o.sq = _param_set(nlayers, 100, fourier=False)
    o.lr, o.alpha, o.eps, o.ema_decay, o.has_ema = 1e-4, 0.99, 1e-8, 0.995, 0
    return o


def _optimizer(nlayers):
    o = _lib.Optimizer()
    o.cfg.kind, o.cfg.lr, o.cfg.alpha, o.cfg.eps, o.cfg.momentum = _lib.OPT_ADAM, 1e-4, 0.99, 1e-8, 0.0
    o.cfg.beta1, o.cfg.beta2 = 0.9, 0.999
    o.sq = _param_set(nlayers, 100, fourier=False)
    o.mom = _param_set(nlayers, 120, fourier=False)
    return o


def _tower(base):
    t = _lib.TowerParams()
    for i, (name, _) in enumerate(_lib.TowerParams._fields_):
        setattr(t, name, _fake(base + i))
    return t


TB, TD = 128, 128  # the towers: B = d0 = d1 = d2 = 128


def _step_desc(b=TB, d0=TD, d1=TD, d2=TD):
    s = _lib.CdkStepDesc()
    s.B, s.d0, s.d1, s.d2 = b, d0, d1, d2
    s.slope, s.bn_eps, s.bn_momentum, s.mu = 0.2, 1e-5, 0.1, 1.0
    s.normalize_mode, s.set_first_mode_const = _lib.NORMALIZE_L2_BALL, 1
    s.lr, s.momentum, s.max_grad_norm, s.first_step, s.gemm_bf16 = 1e-3, 0.9, 2.0, 1, 0
    return s


_R = C.byref
_DESC, _PROB = _desc(), _problem()
_NL = _DESC.nlayers
_PARAMS, _GRADS = _param_set(_NL, 0), _param_set(_NL, 30, fourier=False)
_TOWERS = (_lib.TowerParams * 2)(_tower(100), _tower(120))
_MOMENTA = (_lib.TowerParams * 2)(_tower(140), _tower(160))
_STEP = _step_desc()
_A = [_fake(i) for i in range(20, 40)]  # plain arrays
_AUTO = _lib.PATH_AUTO


def _op_need(lib):
    return lib.nsvd_workspace_bytes(_R(_DESC), B)


def _model_need(lib):
    return lib.nsvd_model_workspace_bytes(_R(_DESC), B)


def _evd(*tail, operator=True, opt=None):
    """the arguments of an EVD-backward entry point around its workspace (partial sums, reduced = 0)"""
    def args(ws, n):
        head = [_R(_DESC), _R(_PARAMS)] + ([_R(_PROB)] if operator else [])
        loss = [_A[0], B, _A[1], _A[2], _lib.MASK_SEQUENTIAL, None, None, _A[3], 0, _A[4], L, 0, 1.0, _A[5], _R(_GRADS)]
        return head + loss + ([_R(opt)] if opt is not None else []) + [ws, n] + list(tail)
    return args


_NO_NEXT = [1, 0, None, None, 0]  # next_seed, next_offset, x_next, ws_next, ws_next_bytes

# name -> (size query of the call's shape, arguments as a function of the workspace pair)
CALLS = {
    "nsvd_operator_features": (_op_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _R(_PROB), _A[0], B, ws, n, 0, _AUTO, None]),
    "nsvd_operator_forward": (_op_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _R(_PROB), _A[0], B, _A[1], _A[2], ws, n, 0,
                                                       _AUTO, None]),
    "nsvd_operator_backward": (_op_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _R(_PROB), _A[0], B, _A[1], _R(_GRADS), ws, n,
                                                        _AUTO, None]),
    "nsvd_operator_sample_features": (_op_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _R(_PROB), 1, 0, _A[0], B, ws, n, 0,
                                                               _AUTO, None]),
    "nsvd_operator_sample_features_dev": (_op_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _R(_PROB), 1, 0, _A[6], _A[0], B,
                                                                   ws, n, 0, _AUTO, None]),
    "nsvd_model_forward": (_model_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _A[0], B, 1.0, _A[1], ws, n, 0, None]),
    "nsvd_model_backward": (_model_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _A[0], B, _A[1], _R(_GRADS), ws, n, None]),
    "nsvd_operator_backward_evd": (_op_need, _evd(_AUTO, None)),
    "nsvd_operator_backward_evd_heads": (_op_need, _evd(_AUTO, 0, L // 2, None)),
    "nsvd_operator_backward_evd_step": (_op_need, _evd(_AUTO, None, opt=_rmsprop(_NL))),
    "nsvd_operator_backward_evd_step_window": (_op_need, _evd(_AUTO, 0, L // 2, 0, None, *_NO_NEXT, None,
                                                              opt=_rmsprop(_NL))),
    "nsvd_operator_backward_evd_step_next": (_op_need, lambda ws, n: _evd(_AUTO, 1, 0, _A[7], WS_NEXT, n + 256, None,
                                                                          opt=_rmsprop(_NL))(ws, n)),
    "nsvd_operator_backward_evd_opt_step": (_op_need, _evd(_AUTO, *_NO_NEXT, None, opt=_optimizer(_NL))),
    "nsvd_model_backward_evd_step": (_model_need, _evd(None, operator=False, opt=_rmsprop(_NL))),
    "nsvd_nef_operator_forward": (_op_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _R(_PROB), _A[0], B, _A[1], _A[2], _A[3],
                                                           _A[4], _A[5], _A[6], _A[7], _A[8], 0.1, ws, n, _AUTO, None]),
    "nsvd_nef_operator_backward": (_op_need, lambda ws, n: [_R(_DESC), _R(_PARAMS), _R(_PROB), _A[0], B, _A[1], _A[2], _A[3],
                                                            _A[4], _A[5], _R(_GRADS), ws, n, _AUTO, None]),
    "nsvd_spin_jac_step": (lambda lib: lib.nsvd_spin_jac_workspace_bytes(_R(_DESC), 64),
                           lambda ws, n: [_R(_DESC), _R(_PARAMS), _A[0], 64, _A[1], 1.0, _A[2], 0.01, _A[3], _R(_GRADS), ws, n,
                                          None]),
    "nsvd_kernel_apply": (lambda lib: lib.nsvd_kernel_apply_workspace_bytes(64, 64, 4),
                          lambda ws, n: [_A[0], 64, 64, _A[1], 64, _A[2], 64, _A[3], 4, 1.0, _A[4], ws, n, None]),
    "nsvd_rbf_apply": (lambda lib: lib.nsvd_rbf_apply_workspace_bytes(64, 64, 3, 4),
                       lambda ws, n: [_A[0], 64, _A[1], 64, 3, _A[2], 4, 0, 1.0, 1.0, _A[3], ws, n, None]),
    "nsvd_rbf_apply_pair": (lambda lib: lib.nsvd_rbf_apply_pair_workspace_bytes(64, 64, 3, 4),
                            lambda ws, n: [_A[0], 64, _A[1], 64, 3, _A[2], _A[3], 4, 0, 1.0, 1.0, 1.0, _A[4], _A[5], ws, n,
                                           None]),
    "nsvd_dot_apply": (lambda lib: lib.nsvd_dot_apply_workspace_bytes(64, 64, 3, 4),
                       lambda ws, n: [_A[0], 64, _A[1], 64, 3, _A[2], 4, 0, 1.0, 1.0, 2, 1.0, _A[3], ws, n, None]),
    "nsvd_dot_apply_pair": (lambda lib: lib.nsvd_dot_apply_pair_workspace_bytes(64, 64, 3, 4),
                            lambda ws, n: [_A[0], 64, _A[1], 64, 3, _A[2], _A[3], 4, 0, 1.0, 1.0, 2, 1.0, 1.0, _A[4], _A[5],
                                           ws, n, None]),
    "nsvd_tsgram_f64": (lambda lib: lib.nsvd_tsgram_f64_workspace_bytes(256, 8),
                        lambda ws, n: [_A[0], 8, _A[1], 8, 256, 8, _A[2], _A[3], ws, n, None]),
    "nsvd_tsgram3_f64": (lambda lib: lib.nsvd_tsgram3_f64_workspace_bytes(256, 8),
                         lambda ws, n: [_A[0], 8, _A[1], 8, 256, 8, _A[2], _A[3], _A[4], ws, n, None]),
    "nsvd_cdk_loss_forward": (lambda lib: lib.nsvd_cdk_workspace_bytes(64, 8, 1),
                              lambda ws, n: [_A[0], _A[1], None, _A[2], _A[3], 64, 8, 1, _A[4], None, None, ws, n, None]),
    "nsvd_cdk_loss_backward": (lambda lib: lib.nsvd_cdk_workspace_bytes(64, 8, 1),
                               lambda ws, n: [_A[0], 64, 8, 1, None, _A[1], _A[2], ws, n, None]),
    "nsvd_tower_forward": (lambda lib: lib.nsvd_tower_workspace_bytes(TB, TD, TD, TD),
                           lambda ws, n: [_A[0], _R(_TOWERS[0]), TB, TD, TD, TD, 0.2, 1e-5, 0.1, 1, 0, _A[1], ws, n, None]),
    "nsvd_tower_forward_phase": (lambda lib: lib.nsvd_tower_workspace_bytes(TB, TD, TD, TD),
                                 lambda ws, n: [_A[0], _R(_TOWERS[0]), TB, TD, TD, TD, 0.2, 1e-5, 0.1, 1, 0, 0, _A[1], ws, n,
                                                None]),
    "nsvd_tower_backward": (lambda lib: lib.nsvd_tower_workspace_bytes(TB, TD, TD, TD),
                            lambda ws, n: [_A[0], _R(_TOWERS[0]), _A[1], TB, TD, TD, TD, 0.2, 0, _R(_MOMENTA[0]), ws, n,
                                           None]),
    "nsvd_cdk_step": (lambda lib: lib.nsvd_cdk_step_workspace_bytes(_R(_STEP)),
                      lambda ws, n: [_R(_STEP), _A[0], _A[1], _TOWERS, _MOMENTA, _A[2], _A[3], _A[4], None, None, ws, n,
                                     None]),
    "nsvd_nef_loss": (lambda lib: lib.nsvd_nef_loss_workspace_bytes(64, 32, 32, 4),
                      lambda ws, n: [_A[0], _A[1], 64, _A[2], _A[3], 32, _A[4], _A[5], 32, 4, 1, 0, _A[6], _A[7], _A[8],
                                     _A[9], ws, n, None]),
    "nsvd_nef_rows_forward": (lambda lib: lib.nsvd_nef_rows_workspace_bytes(64, 4),
                              lambda ws, n: [_A[0], 64, 32, 4, _A[1], _A[2], None, None, None, 0.1, None, 0, ws, n, None]),
    "nsvd_nef_rows_backward": (lambda lib: lib.nsvd_nef_rows_workspace_bytes(64, 4),
                               lambda ws, n: [_A[0], _A[1], 64, 32, 4, _A[2], None, None, _A[3], ws, n, None]),
    "nsvd_retrieval_eval": (lambda lib: lib.nsvd_retrieval_workspace_bytes(8, 64, 16, 4),
                            lambda ws, n: [_A[0], 16, _A[1], 16, 8, 64, 16, _A[2], _A[3], None, 0, 4, None, None, _A[4],
                                           None, None, None, ws, n, None]),
}


def test_every_workspace_entry_point_is_covered():
    """an entry point of _lib.SIGNATURES takes a workspace where a pointer is followed by a size_t that is no element
    count (the optimiser steps and nsvd_to_bf16 take counts)"""
    counts = {"nsvd_rmsprop_ema_step", "nsvd_rmsprop_ema_step_dev", "nsvd_opt_step", "nsvd_opt_step_dev", "nsvd_to_bf16"}
    takes = set()
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        if name not in counts and any(a is C.c_void_p and b is C.c_size_t for a, b in zip(argtypes, argtypes[1:])):
            takes.add(name)
    assert takes == set(CALLS)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_workspace_one_byte_short(name):
    lib = _lib.load()
    need, args = CALLS[name]
    n = need(lib)
    assert n > 0
    assert getattr(lib, name)(*args(WS, n - 1)) == EINVAL


@pytest.mark.parametrize("name", sorted(CALLS))
def test_workspace_base_off_by_128(name):
    lib = _lib.load()
    need, args = CALLS[name]
    n = need(lib)
    assert n > 0
    assert getattr(lib, name)(*args(WS + 128, n + 256)) == EINVAL


def test_next_batch_workspace():
    """nsvd_operator_backward_evd_step_next's second pair, the step's own workspace in order"""
    lib = _lib.load()
    n = _op_need(lib)
    fn = lib.nsvd_operator_backward_evd_step_next
    opt = _rmsprop(_NL)
    for ws_next, n_next in ((WS_NEXT, n - 1), (WS_NEXT + 128, n + 256)):
        assert fn(*_evd(_AUTO, 1, 0, _A[7], ws_next, n_next, None, opt=opt)(WS, n)) == EINVAL


# ---- the towers' tensors: the backward and the step refuse a null one, as the forward does ----------------------------
TOWER_TENSORS = ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2")  # what has a gradient
TOWER_RUNNING = ("rm1", "rv1", "rm2", "rv2")


def _tower_without(base, field):
    t = _tower(base)
    setattr(t, field, None)
    return t


@pytest.mark.parametrize("which", ["params", "grads"])
@pytest.mark.parametrize("field", TOWER_TENSORS)
def test_tower_backward_refuses_a_null_tensor(which, field):
    """(before the towers' one validator the backward checked `grads` alone: a null g2 in `params` went into a kernel
    argument). Everything else about the call is in order: the workspace is large enough and aligned."""
    lib = _lib.load()
    n = lib.nsvd_tower_workspace_bytes(TB, TD, TD, TD)
    p = _tower_without(100, field) if which == "params" else _tower(100)
    g = _tower_without(140, field) if which == "grads" else _tower(140)
    assert lib.nsvd_tower_backward(_A[0], _R(p), _A[1], TB, TD, TD, TD, 0.2, 0, _R(g), WS, n, None) == EINVAL
    if which == "params":  # what the forward already refused
        assert lib.nsvd_tower_forward(_A[0], _R(p), TB, TD, TD, TD, 0.2, 1e-5, 0.1, 0, 0, _A[1], WS, n, None) == EINVAL


@pytest.mark.parametrize("which,field", [("towers", f) for f in TOWER_TENSORS + TOWER_RUNNING] +
                         [("momentum_bufs", f) for f in TOWER_TENSORS])
def test_cdk_step_refuses_a_null_tensor_of_the_second_tower(which, field):
    """the refusal comes before the first launch (the momentum buffers used to be looked at after the towers' backward):
    tower 0 is complete, so a launch on the made-up addresses would return HIP's error, not NSVD_EINVAL. The step updates
    the running statistics, so `towers` needs all twelve tensors."""
    lib = _lib.load()
    n = lib.nsvd_cdk_step_workspace_bytes(_R(_STEP))
    towers = (_lib.TowerParams * 2)(_tower(100), _tower_without(120, field) if which == "towers" else _tower(120))
    momenta = (_lib.TowerParams * 2)(_tower(140),
                                     _tower_without(160, field) if which == "momentum_bufs" else _tower(160))
    assert lib.nsvd_cdk_step(_R(_STEP), _A[0], _A[1], towers, momenta, _A[2], _A[3], _A[4], None, None, WS, n,
                             None) == EINVAL


# ---- the size queries ------------------------------------------------------------------------------------------------
_BIG = _desc(l=64, d=3)  # with B = 8192
_GENERIC = _desc(hidden=(128, 7))
_BIG_SPIN = _desc(l=64, d=3, m=64, hidden=(32, 32))
_BIG_STEP = _step_desc(b=1024, d0=512, d1=2048, d2=512)  # (the towers take B <= 1024)

# key -> (query, arguments); recorded value in SIZES
QUERIES = {
    "workspace": ("nsvd_workspace_bytes", (_DESC, B)),
    "workspace-big": ("nsvd_workspace_bytes", (_BIG, 8192)),
    "workspace-generic": ("nsvd_workspace_bytes", (_GENERIC, B)),
    "model": ("nsvd_model_workspace_bytes", (_DESC, B)),
    "model-big": ("nsvd_model_workspace_bytes", (_BIG, 8192)),
    "model-generic": ("nsvd_model_workspace_bytes", (_GENERIC, B)),
    "spin_jac": ("nsvd_spin_jac_workspace_bytes", (_DESC, 64)),
    "spin_jac-big": ("nsvd_spin_jac_workspace_bytes", (_BIG_SPIN, 8192)),
    "kernel_apply": ("nsvd_kernel_apply_workspace_bytes", (64, 64, 4)),
    "kernel_apply-big": ("nsvd_kernel_apply_workspace_bytes", (16384, 8192, 64)),
    "rbf_apply": ("nsvd_rbf_apply_workspace_bytes", (64, 64, 3, 4)),
    "rbf_apply-big": ("nsvd_rbf_apply_workspace_bytes", (8192, 8192, 3, 64)),
    "rbf_apply_pair": ("nsvd_rbf_apply_pair_workspace_bytes", (64, 64, 3, 4)),
    "rbf_apply_pair-big": ("nsvd_rbf_apply_pair_workspace_bytes", (8192, 8192, 3, 64)),
    "dot_apply": ("nsvd_dot_apply_workspace_bytes", (64, 64, 3, 4)),
    "dot_apply-big": ("nsvd_dot_apply_workspace_bytes", (8192, 8192, 3, 64)),
    "dot_apply_pair": ("nsvd_dot_apply_pair_workspace_bytes", (64, 64, 3, 4)),
    "dot_apply_pair-big": ("nsvd_dot_apply_pair_workspace_bytes", (8192, 8192, 3, 64)),
    "tsgram": ("nsvd_tsgram_f64_workspace_bytes", (256, 8)),
    "tsgram-big": ("nsvd_tsgram_f64_workspace_bytes", (8192, 64)),
    "tsgram3": ("nsvd_tsgram3_f64_workspace_bytes", (256, 8)),
    "tsgram3-big": ("nsvd_tsgram3_f64_workspace_bytes", (8192, 64)),
    "cdk": ("nsvd_cdk_workspace_bytes", (64, 8, 1)),
    "cdk-no-first-mode": ("nsvd_cdk_workspace_bytes", (64, 8, 0)),
    "cdk-big": ("nsvd_cdk_workspace_bytes", (8192, 64, 1)),
    "tower": ("nsvd_tower_workspace_bytes", (TB, TD, TD, TD)),
    "tower-big": ("nsvd_tower_workspace_bytes", (1024, 512, 2048, 512)),
    "cdk_step": ("nsvd_cdk_step_workspace_bytes", (_STEP,)),
    "cdk_step-big": ("nsvd_cdk_step_workspace_bytes", (_BIG_STEP,)),
    "nef_loss": ("nsvd_nef_loss_workspace_bytes", (64, 32, 32, 4)),
    "nef_loss-big": ("nsvd_nef_loss_workspace_bytes", (8192, 4096, 4096, 64)),
    "nef_rows": ("nsvd_nef_rows_workspace_bytes", (64, 4)),
    "nef_rows-big": ("nsvd_nef_rows_workspace_bytes", (8192, 64)),
    "retrieval": ("nsvd_retrieval_workspace_bytes", (8, 64, 16, 4)),
    "retrieval-big": ("nsvd_retrieval_workspace_bytes", (8192, 8192, 64, 100)),
}


def _query(lib, key):
    name, args = QUERIES[key]
    return getattr(lib, name)(*[_R(a) if isinstance(a, C.Structure) else a for a in args])


# recorded from the preceding build (see the module docstring)
SIZES = {
    "workspace": 92536832,
    "workspace-big": 6664749056,
    "workspace-generic": 51740672,
    "model": 62187776,
    "model-big": 1881190656,
    "model-generic": 17137664,
    "spin_jac": 41488640,
    "spin_jac-big": 285411328,
    "kernel_apply": 32768,
    "kernel_apply-big": 20971520,
    "rbf_apply": 33792,
    "rbf_apply-big": 10616832,
    "rbf_apply_pair": 66560,
    "rbf_apply_pair-big": 104988672,
    "dot_apply": 35072,
    "dot_apply-big": 10780672,
    "dot_apply_pair": 70144,
    "dot_apply_pair-big": 105447424,
    "tsgram": 4096,
    "tsgram-big": 8388608,
    "tsgram3": 6144,
    "tsgram3-big": 12582912,
    "cdk": 401920,
    "cdk-no-first-mode": 135680,
    "cdk-big": 19017984,
    "tower": 985088,
    "tower-big": 91246592,
    "cdk_step": 3810560,
    "cdk_step-big": 235131904,
    "nef_loss": 768,
    "nef_loss-big": 2130944,
    "nef_rows": 256,
    "nef_rows-big": 66048,
    "retrieval": 4608,
    "retrieval-big": 67141888,
}


def test_every_size_query_is_recorded():
    assert {name for name, _ in QUERIES.values()} == {n for n in _lib.SIGNATURES if n.endswith("workspace_bytes")}
    assert set(SIZES) == set(QUERIES)


@pytest.mark.parametrize("key", sorted(QUERIES))
def test_workspace_bytes_unchanged(key):
    assert SIZES[key] > 0 and _query(_lib.load(), key) == SIZES[key]
