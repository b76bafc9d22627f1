"""CPU-only: what the seven EVD-backward entry points REFUSE, and with which code.

Every call here is refused by the host code of csrc/operator_api.hip before it reaches a HIP call, so the descriptors are
real and the device pointers are made-up (non-null, 256-byte aligned) addresses that nothing dereferences. Only refused
calls belong in this file: an accepted one would launch kernels on those addresses.

The codes of the first table are the documented contract of include/nsvd.h. Those of the second table (the optimiser
descriptors' conversion, the next-batch checks, null problems) and of the third (two violations at once: which refusal
comes first) were RECORDED from the build that preceded the shared call record / prologue helpers of operator_api.hip,
not derived from the code under test: they pin the order of refusals that refactor had to keep."""
import ctypes as C

import pytest

from neural_svd_amd import _lib
from neural_svd_amd._lib import EINVAL, EUNSUPPORTED

L, D, M_FEATURES, B = 16, 2, 1024, 512
FUSED_HIDDEN, OTHER_HIDDEN = (128, 128, 128), (128, 7)  # the MFMA kernels take the first shape only


def _fake(i):
    """a made-up device address: non-null, 256-byte aligned, distinct per i"""
    return 0x7F0000000000 + 0x100000 * i


def _desc(hidden=FUSED_HIDDEN, d=D):
    s = _lib.ModelDesc()
    s.L, s.D, s.m = L, d, M_FEATURES
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


def _rmsprop(nlayers, state=None, has_ema=False, ema=True):
    o = _lib.Rmsprop()
    o.sq = _param_set(nlayers, 100, fourier=False)
    if has_ema and ema:
        o.ema = _param_set(nlayers, 140, fourier=False)
    o.lr, o.alpha, o.eps, o.ema_decay, o.has_ema = 1e-4, 0.99, 1e-8, 0.995, int(has_ema)
    o.state = state
    return o


def _optimizer(nlayers, kind=_lib.OPT_ADAM, momentum=0.0, state=None, mom=True):
    o = _lib.Optimizer()
    o.cfg.kind, o.cfg.lr, o.cfg.alpha, o.cfg.eps, o.cfg.momentum = kind, 1e-4, 0.99, 1e-8, momentum
    o.cfg.beta1, o.cfg.beta2 = 0.9, 0.999
    o.sq = _param_set(nlayers, 100, fourier=False)
    if mom:
        o.mom = _param_set(nlayers, 120, fourier=False)
    o.state = state
    return o


# the arguments of each entry point, in the order of include/nsvd.h
_LOSS = ["x", "B", "f", "Tf", "mask_kind", "v", "M", "moments", "moments_reduced", "evd_scratch", "L_total", "l_offset",
         "grad_scale", "loss", "grads"]
_OPERATOR = ["desc", "params", "prob"] + _LOSS
_NEXT = ["next_seed", "next_offset", "x_next", "ws_next", "ws_next_bytes"]
ENTRY = {
    "evd": ("nsvd_operator_backward_evd", _OPERATOR + ["ws", "ws_bytes", "path", "stream"]),
    "heads": ("nsvd_operator_backward_evd_heads", _OPERATOR + ["ws", "ws_bytes", "path", "l_begin", "l_count", "stream"]),
    "step": ("nsvd_operator_backward_evd_step", _OPERATOR + ["opt", "ws", "ws_bytes", "path", "stream"]),
    "step_window": ("nsvd_operator_backward_evd_step_window",
                    _OPERATOR + ["opt", "ws", "ws_bytes", "path", "l_begin", "l_count", "last_window", "ev_after_chain"] +
                    _NEXT + ["stream"]),
    "step_next": ("nsvd_operator_backward_evd_step_next", _OPERATOR + ["opt", "ws", "ws_bytes", "path"] + _NEXT + ["stream"]),
    "opt_step": ("nsvd_operator_backward_evd_opt_step", _OPERATOR + ["opt", "ws", "ws_bytes", "path"] + _NEXT + ["stream"]),
    "model": ("nsvd_model_backward_evd_step", ["desc", "params"] + _LOSS + ["opt", "ws", "ws_bytes", "stream"]),
}
WS, WS_NEXT = _fake(60), _fake(80)


def _call(entry, hidden=FUSED_HIDDEN, d=D, **over):
    """the entry point on a well-formed call (reduced=0 with partial sums: every path takes it) changed by `over`;
    ws_bytes / ws_next_bytes default to what the shape needs. Descriptors may be given as ctypes structs or None."""
    lib = _lib.load()
    name, order = ENTRY[entry]
    desc = _desc(hidden, d)
    nl = desc.nlayers
    need = (lib.nsvd_model_workspace_bytes if entry == "model" else lib.nsvd_workspace_bytes)(C.byref(desc), B)
    a = dict(desc=desc, params=_param_set(nl, 0), prob=_problem(), x=_fake(20), B=B, f=_fake(21), Tf=_fake(22),
             mask_kind=_lib.MASK_SEQUENTIAL, v=None, M=None, moments=_fake(23), moments_reduced=0, evd_scratch=_fake(24),
             L_total=L, l_offset=0, grad_scale=1.0, loss=_fake(25), grads=_param_set(nl, 30, fourier=False),
             opt=_optimizer(nl) if entry == "opt_step" else _rmsprop(nl), ws=WS, ws_bytes=need, path=_lib.PATH_AUTO,
             l_begin=0, l_count=L // 2, last_window=0, ev_after_chain=None, next_seed=1, next_offset=0,
             x_next=_fake(26) if entry == "step_next" else None, ws_next=WS_NEXT if entry == "step_next" else None,
             ws_next_bytes=need if entry == "step_next" else 0, stream=None)
    a.update(over)
    args = [C.byref(v) if isinstance(v, C.Structure) else v for v in (a[k] for k in order)]
    return getattr(lib, name)(*args)


DIRECT = dict(moments=None, moments_reduced=0, evd_scratch=None)

# (id, entry, changes, code): include/nsvd.h's contract
DOCUMENTED = [
    ("evd-null-grads", "evd", dict(grads=None), EINVAL),
    ("evd-mask-kind-3", "evd", dict(mask_kind=3), EINVAL),
    ("evd-custom-mask-without-v-M", "evd", dict(mask_kind=_lib.MASK_CUSTOM), EINVAL),
    ("evd-ws-misaligned", "evd", dict(ws=WS + 4), EINVAL),
    ("evd-ws-too-small", "evd", dict(ws_bytes=16), EINVAL),
    ("evd-l-offset-past-L-total", "evd", dict(L_total=16, l_offset=1), EINVAL),
    ("evd-generic-direct-mode", "evd", dict(path=_lib.PATH_GENERIC, **DIRECT), EINVAL),
    ("evd-generic-head-sharding", "evd", dict(path=_lib.PATH_GENERIC, L_total=32), EUNSUPPORTED),
    ("evd-fused-on-other-shape", "evd", dict(hidden=OTHER_HIDDEN, path=_lib.PATH_FUSED), EUNSUPPORTED),
    ("heads-no-heads", "heads", dict(l_count=0), EINVAL),
    ("heads-generic-window", "heads", dict(path=_lib.PATH_GENERIC, l_count=8), EUNSUPPORTED),
    ("step-null-opt", "step", dict(opt=None), EINVAL),
    ("step_next-one-workspace", "step_next", dict(ws_next=WS), EINVAL),
    ("step_next-generic", "step_next", dict(path=_lib.PATH_GENERIC), EUNSUPPORTED),
    ("step_window-generic", "step_window", dict(path=_lib.PATH_GENERIC), EUNSUPPORTED),
    ("opt_step-unknown-kind", "opt_step", dict(opt=_optimizer(4, kind=9)), EINVAL),
    ("model-other-shape", "model", dict(hidden=OTHER_HIDDEN, opt=_rmsprop(3)), EUNSUPPORTED),
]

# recorded from the preceding build (see the module docstring)
RECORDED = [
    ("step-state-misaligned", "step", dict(opt=_rmsprop(4, state=_fake(50) + 4)), EINVAL),
    ("step-generic-with-state", "step", dict(opt=_rmsprop(4, state=_fake(50)), path=_lib.PATH_GENERIC), EUNSUPPORTED),
    ("step-ema-set-empty", "step", dict(opt=_rmsprop(4, has_ema=True, ema=False)), EINVAL),
    ("model-state-misaligned", "model", dict(opt=_rmsprop(4, state=_fake(50) + 4)), EINVAL),
    ("model-neither-opt-nor-grads", "model", dict(opt=None, grads=None), EINVAL),
    ("opt_step-state-misaligned", "opt_step", dict(opt=_optimizer(4, state=_fake(50) + 4)), EINVAL),
    ("opt_step-rmsprop-rule-with-state", "opt_step",
     dict(opt=_optimizer(4, kind=_lib.OPT_RMSPROP, state=_fake(50))), EUNSUPPORTED),
    ("opt_step-adam-mom-set-empty", "opt_step", dict(opt=_optimizer(4, mom=False)), EINVAL),
    ("opt_step-generic-next-batch", "opt_step",
     dict(path=_lib.PATH_GENERIC, x_next=_fake(26), ws_next=WS_NEXT, ws_next_bytes=1 << 40), EUNSUPPORTED),
    ("step_window-next-without-workspace", "step_window", dict(x_next=_fake(26)), EINVAL),
    ("step_window-next-workspace-misaligned", "step_window",
     dict(x_next=_fake(26), ws_next=WS_NEXT + 4, ws_next_bytes=1 << 40), EINVAL),
    ("opt_step-next-workspace-too-small", "opt_step", dict(x_next=_fake(26), ws_next=WS_NEXT, ws_next_bytes=16), EINVAL),
    ("step_next-null-x-next", "step_next", dict(x_next=None), EINVAL),
    ("step_window-null-prob", "step_window", dict(prob=None), EINVAL),
    ("step_next-null-prob", "step_next", dict(prob=None), EINVAL),
    ("opt_step-null-prob", "opt_step", dict(prob=None), EINVAL),
    ("evd-null-prob", "evd", dict(prob=None), EINVAL),
]

# two violations at once: the refusal that comes first decides (recorded from the preceding build)
ORDER = [
    ("null-grads+mask-kind", "evd", dict(grads=None, mask_kind=3), EINVAL),
    ("ws-too-small+fused-on-other-shape", "evd", dict(hidden=OTHER_HIDDEN, path=_lib.PATH_FUSED, ws_bytes=16), EINVAL),
    # the model description is judged before a missing problem ...
    ("too-many-dimensions+null-prob", "evd", dict(d=13, prob=None, ws_bytes=1 << 40), EUNSUPPORTED),
    # ... the optimiser descriptor behind the inputs (mask_kind) and before the workspace ...
    ("mask-kind+rmsprop-rule-with-state", "opt_step",
     dict(mask_kind=3, opt=_optimizer(4, kind=_lib.OPT_RMSPROP, state=_fake(50))), EINVAL),
    ("rmsprop-rule-with-state+ws-too-small", "opt_step",
     dict(ws_bytes=16, opt=_optimizer(4, kind=_lib.OPT_RMSPROP, state=_fake(50))), EUNSUPPORTED),
    # ... the next batch's workspace before the step's, and both before the path ...
    ("next-workspace-too-small+generic", "step_next", dict(ws_next_bytes=16, path=_lib.PATH_GENERIC), EINVAL),
    ("ws-too-small+generic", "step_window", dict(ws_bytes=16, path=_lib.PATH_GENERIC), EINVAL),
    # ... the path before the head range, the head range before what only the fused kernels do
    ("fused-on-other-shape+l-offset", "evd",
     dict(hidden=OTHER_HIDDEN, path=_lib.PATH_FUSED, L_total=16, l_offset=1), EUNSUPPORTED),
    ("generic-window+l-offset", "heads", dict(path=_lib.PATH_GENERIC, l_count=8, L_total=16, l_offset=1), EINVAL),
]


def _cases(table):
    return [pytest.param(entry, over, code, id=name) for name, entry, over, code in table]


@pytest.mark.parametrize("entry,over,code", _cases(DOCUMENTED))
def test_documented_refusals(entry, over, code):
    assert _call(entry, **over) == code


@pytest.mark.parametrize("entry,over,code", _cases(RECORDED))
def test_descriptor_and_next_batch_refusals(entry, over, code):
    assert _call(entry, **over) == code


@pytest.mark.parametrize("entry,over,code", _cases(ORDER))
def test_order_of_refusals(entry, over, code):
    assert _call(entry, **over) == code
