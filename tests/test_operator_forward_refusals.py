"""CPU-only: what the forward-family entry points REFUSE, and with which code.

The entry points are nsvd_operator_forward, nsvd_operator_features, nsvd_operator_sample_features,
nsvd_operator_sample_features_dev, nsvd_operator_backward, nsvd_model_forward and nsvd_model_backward. As in
test_evd_backward_refusals.py every call here is refused by the host code of csrc/operator_api.hip before it reaches a
HIP call, so the descriptors are real and the device pointers are made-up (non-null, 256-byte aligned) addresses that
nothing dereferences. Only refused calls belong in this file: an accepted one would launch kernels on those addresses, so
the module skips itself where a GPU is visible.

The entry points take DIFFERENT subsets of the checks (nsvd_operator_features and nsvd_operator_backward do not judge
the problem, nsvd_operator_features asks the parameter set for fourier_B only, ...), which is why a case that one entry
point refuses is missing for another: there it is accepted. Every code below was RECORDED from the build that preceded
the shared call record / prologue of these entry points, not derived from the code under test; the last table (two
violations at once) pins the order of the refusals."""
import ctypes as C

import pytest
import torch

from neural_svd_amd import _lib
from neural_svd_amd._lib import EINVAL, EUNSUPPORTED

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="an accepted call would launch on made-up addresses: no-GPU machines only")

L, D, M_FEATURES, B = 16, 2, 1024, 512
FUSED_HIDDEN, OTHER_HIDDEN = (128, 128, 128), (128, 7)  # the MFMA kernels take the first shape only


def _fake(i):
    """a made-up device address: non-null, 256-byte aligned, distinct per i"""
    return 0x7F0000000000 + 0x100000 * i


def _desc(hidden=FUSED_HIDDEN, d=D, **fields):
    s = _lib.ModelDesc()
    s.L, s.D, s.m = L, d, M_FEATURES
    dims = tuple(hidden) + (1,)
    s.nlayers = len(dims)
    for i, h in enumerate(dims):
        s.dims[i] = h
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _param_set(nlayers, base, fourier=True, drop_w=None):
    p = _lib.Params()
    if fourier:
        p.fourier_B = _fake(base)
    for i in range(nlayers):
        p.W[i] = _fake(base + 1 + 2 * i)
        p.b[i] = _fake(base + 2 + 2 * i)
    if drop_w is not None:
        p.W[drop_w] = None
    return p


def _problem(**fields):
    q = _lib.Problem()
    q.potential, q.charge_or_k, q.scale_kinetic, q.eps = _lib.POT_HYDROGEN, 1.0, 1.0, 0.01
    q.op_scale, q.sigma, q.hard_mul_const, q.use_importance = 100.0, 16.0, 1.0, _lib.IMP_GAUSSIAN
    for k, v in fields.items():
        setattr(q, k, v)
    return q


# the arguments of each entry point, in the order of include/nsvd.h
_OP = ["desc", "params", "prob"]
_TAIL = ["ws", "ws_bytes", "save", "path", "stream"]
ENTRY = {
    "forward": ("nsvd_operator_forward", _OP + ["x", "B", "f", "Tf"] + _TAIL),
    "features": ("nsvd_operator_features", _OP + ["x", "B"] + _TAIL),
    "sample": ("nsvd_operator_sample_features", _OP + ["seed", "offset", "x", "B"] + _TAIL),
    "sample_dev": ("nsvd_operator_sample_features_dev", _OP + ["seed", "offset", "state", "x", "B"] + _TAIL),
    "backward": ("nsvd_operator_backward", _OP + ["x", "B", "df", "grads", "ws", "ws_bytes", "path", "stream"]),
    "model_forward": ("nsvd_model_forward", ["desc", "params", "x", "B", "c", "f", "ws", "ws_bytes", "save", "stream"]),
    "model_backward": ("nsvd_model_backward", ["desc", "params", "x", "B", "df", "grads", "ws", "ws_bytes", "stream"]),
}
OPERATOR = ("forward", "features", "sample", "sample_dev", "backward")
WS, STATE = _fake(60), _fake(50)


def _call(entry, hidden=FUSED_HIDDEN, d=D, desc_fields=None, prob_fields=None, **over):
    """the entry point on a well-formed call changed by `over`; ws_bytes defaults to what the shape needs. Descriptors
    may be given as ctypes structs or None."""
    lib = _lib.load()
    name, order = ENTRY[entry]
    desc = _desc(hidden, d, **(desc_fields or {}))
    nl = desc.nlayers
    need = (lib.nsvd_model_workspace_bytes if entry.startswith("model") else lib.nsvd_workspace_bytes)(C.byref(desc), B)
    a = dict(desc=desc, params=_param_set(nl, 0), prob=_problem(**(prob_fields or {})), x=_fake(20), B=B, f=_fake(21),
             Tf=_fake(22), df=_fake(23), grads=_param_set(nl, 30, fourier=False), seed=1, offset=0, state=STATE, c=1.0,
             ws=WS, ws_bytes=need, save=1, path=_lib.PATH_AUTO, stream=None)
    a.update(over)
    args = [C.byref(v) if isinstance(v, C.Structure) else v for v in (a[k] for k in order)]
    return getattr(lib, name)(*args)


# ---- one violation per call ------------------------------------------------------------------------------------------
# each null argument (the stream may be null: the default stream)
NULLS = {
    "forward": ["desc", "params", "prob", "x", "f", "Tf", "ws"],
    "features": ["desc", "params", "prob", "x", "ws"],
    "sample": ["desc", "params", "prob", "x", "ws"],
    "sample_dev": ["desc", "params", "prob", "state", "x", "ws"],
    "backward": ["desc", "params", "prob", "x", "df", "grads", "ws"],
    "model_forward": ["desc", "params", "x", "f", "ws"],
    "model_backward": ["desc", "params", "x", "df", "grads", "ws"],
}
SINGLE = [(f"{e}-null-{k}", e, {k: None}, EINVAL) for e, names in NULLS.items() for k in names]
# what every entry point checks: B, the model description, the workspace
for _e in ENTRY:
    SINGLE += [
        (f"{_e}-B-zero", _e, dict(B=0), EINVAL),
        (f"{_e}-B-negative", _e, dict(B=-32), EINVAL),
        (f"{_e}-desc-no-layers", _e, dict(desc_fields=dict(nlayers=0)), EINVAL),
        (f"{_e}-desc-box-without-limit", _e, dict(desc_fields=dict(box_mask=1, box_lim=0.0)), EINVAL),
        (f"{_e}-too-many-dimensions", _e, dict(d=65 if _e.startswith("model") else 13, ws_bytes=1 << 40), EUNSUPPORTED),
        (f"{_e}-ws-misaligned", _e, dict(ws=WS + 4, ws_bytes=1 << 40), EINVAL),
        (f"{_e}-ws-too-small", _e, dict(ws_bytes=16), EINVAL),
        (f"{_e}-null-fourier_B", _e, dict(params=_param_set(4, 0, fourier=False)), EINVAL),
    ]
# the whole parameter set (nsvd_operator_features and the samplers ask for fourier_B only)
for _e in ("forward", "backward", "model_forward", "model_backward"):
    SINGLE += [
        (f"{_e}-params-null-W1", _e, dict(params=_param_set(4, 0, drop_w=1)), EINVAL),
        (f"{_e}-exp-mask-without-scales", _e, dict(desc_fields=dict(has_exp_mask=1)), EINVAL),
    ]
for _e in ("backward", "model_backward"):
    SINGLE += [(f"{_e}-grads-null-W1", _e, dict(grads=_param_set(4, 30, fourier=False, drop_w=1)), EINVAL)]
# the problem (nsvd_operator_features and nsvd_operator_backward do not judge it)
for _e in ("forward", "sample", "sample_dev"):
    SINGLE += [
        (f"{_e}-unknown-potential", _e, dict(prob_fields=dict(potential=99)), EINVAL),
        (f"{_e}-unknown-importance", _e, dict(prob_fields=dict(use_importance=7)), EINVAL),
        (f"{_e}-exact-above-small-stencil", _e, dict(d=5, prob_fields=dict(eps=0.0)), EUNSUPPORTED),
    ]
# the path
for _e in OPERATOR:
    SINGLE += [
        (f"{_e}-generic-exact-with-eps", _e, dict(path=_lib.PATH_GENERIC_EXACT), EUNSUPPORTED),
        (f"{_e}-fused-on-other-shape", _e, dict(hidden=OTHER_HIDDEN, path=_lib.PATH_FUSED), EUNSUPPORTED),
        (f"{_e}-bf16x3-on-other-shape", _e, dict(hidden=OTHER_HIDDEN, path=_lib.PATH_FUSED_BF16X3), EUNSUPPORTED),
        (f"{_e}-bf16x3-D4", _e, dict(d=4, path=_lib.PATH_FUSED_BF16X3), EUNSUPPORTED),
        (f"{_e}-bf16x3-D5", _e, dict(d=5, path=_lib.PATH_FUSED_BF16X3), EUNSUPPORTED),
    ]
# eps <= 0 on the generic kernels (nsvd_operator_backward takes it: what it reads was saved by the forward)
for _e in ("forward", "features", "sample", "sample_dev"):
    SINGLE += [
        (f"{_e}-generic-eps-zero", _e, dict(path=_lib.PATH_GENERIC, prob_fields=dict(eps=0.0)), EUNSUPPORTED),
        (f"{_e}-generic-eps-negative", _e, dict(path=_lib.PATH_GENERIC, prob_fields=dict(eps=-1.0)), EUNSUPPORTED),
        (f"{_e}-auto-eps-zero-on-other-shape", _e, dict(hidden=OTHER_HIDDEN, prob_fields=dict(eps=0.0)), EUNSUPPORTED),
    ]
SINGLE += [("sample_dev-state-misaligned", "sample_dev", dict(state=STATE + 4), EINVAL)]

# ---- two violations at once: the refusal that comes first decides -----------------------------------------------------
_EXACT_EPS = dict(path=_lib.PATH_GENERIC_EXACT)            # NSVD_EUNSUPPORTED on its own
_FUSED_OTHER = dict(hidden=OTHER_HIDDEN, path=_lib.PATH_FUSED)  # NSVD_EUNSUPPORTED on its own
_BAD_PROB = dict(prob_fields=dict(potential=99))           # NSVD_EINVAL on its own (where the problem is judged)
ORDER = [
    # the model description is judged before anything else ...
    ("forward-too-many-dimensions+null-prob", "forward", dict(d=13, prob=None), EUNSUPPORTED),
    ("features-too-many-dimensions+null-x", "features", dict(d=13, x=None), EUNSUPPORTED),
    ("sample-too-many-dimensions+null-params", "sample", dict(d=13, params=None), EUNSUPPORTED),
    ("backward-too-many-dimensions+null-prob", "backward", dict(d=13, prob=None), EUNSUPPORTED),
    ("model_forward-too-many-dimensions+null-x", "model_forward", dict(d=65, x=None), EUNSUPPORTED),
    ("model_backward-too-many-dimensions+null-grads", "model_backward", dict(d=65, grads=None), EUNSUPPORTED),
    # ... except nsvd_operator_sample_features_dev's state
    ("sample_dev-null-state+too-many-dimensions", "sample_dev", dict(state=None, d=13), EINVAL),
    ("sample_dev-state-misaligned+too-many-dimensions", "sample_dev", dict(state=STATE + 4, d=13), EINVAL),
    # null arguments and B before the problem and the path
    ("forward-null-Tf+exact-above-small-stencil", "forward", dict(Tf=None, d=5, prob_fields=dict(eps=0.0)), EINVAL),
    ("forward-B-zero+generic-exact-with-eps", "forward", dict(B=0, **_EXACT_EPS), EINVAL),
    ("sample-null-x+generic-exact-with-eps", "sample", dict(x=None, **_EXACT_EPS), EINVAL),
    ("features-null-fourier_B+fused-on-other-shape", "features",
     dict(params=_param_set(3, 0, fourier=False), **_FUSED_OTHER), EINVAL),
    ("backward-null-df+fused-on-other-shape", "backward", dict(df=None, **_FUSED_OTHER), EINVAL),
    # the problem before the exact-path status, that before the parameter set, the workspace and the path
    ("forward-unknown-potential+generic-exact-with-eps", "forward", dict(**_BAD_PROB, **_EXACT_EPS), EINVAL),
    ("sample-unknown-potential+generic-exact-with-eps", "sample", dict(**_BAD_PROB, **_EXACT_EPS), EINVAL),
    ("forward-exact-above-small-stencil+null-params", "forward",
     dict(d=5, prob_fields=dict(eps=0.0), params=None), EUNSUPPORTED),
    ("forward-generic-exact-with-eps+null-params", "forward", dict(params=None, **_EXACT_EPS), EUNSUPPORTED),
    ("forward-generic-exact-with-eps+ws-too-small", "forward", dict(ws_bytes=16, **_EXACT_EPS), EUNSUPPORTED),
    ("sample-generic-exact-with-eps+ws-too-small", "sample", dict(ws_bytes=16, **_EXACT_EPS), EUNSUPPORTED),
    ("sample_dev-generic-exact-with-eps+ws-misaligned", "sample_dev",
     dict(ws=WS + 4, ws_bytes=1 << 40, **_EXACT_EPS), EUNSUPPORTED),
    # nsvd_operator_features and nsvd_operator_backward ask the exact-path status LAST: the workspace comes first
    ("features-ws-too-small+generic-exact-with-eps", "features", dict(ws_bytes=16, **_EXACT_EPS), EINVAL),
    ("backward-ws-too-small+generic-exact-with-eps", "backward", dict(ws_bytes=16, **_EXACT_EPS), EINVAL),
    ("backward-null-grads+generic-exact-with-eps", "backward", dict(grads=None, **_EXACT_EPS), EINVAL),
    # the parameter set before the workspace, the workspace before the path
    ("forward-params-null-W1+fused-on-other-shape", "forward",
     dict(params=_param_set(3, 0, drop_w=1), **_FUSED_OTHER), EINVAL),
    ("backward-grads-null-W1+fused-on-other-shape", "backward",
     dict(grads=_param_set(3, 30, fourier=False, drop_w=1), **_FUSED_OTHER), EINVAL),
    ("forward-ws-too-small+fused-on-other-shape", "forward", dict(ws_bytes=16, **_FUSED_OTHER), EINVAL),
    ("features-ws-misaligned+fused-on-other-shape", "features", dict(ws=WS + 4, ws_bytes=1 << 40, **_FUSED_OTHER), EINVAL),
    ("sample-ws-too-small+fused-on-other-shape", "sample", dict(ws_bytes=16, **_FUSED_OTHER), EINVAL),
    ("backward-ws-too-small+fused-on-other-shape", "backward", dict(ws_bytes=16, **_FUSED_OTHER), EINVAL),
    ("forward-ws-too-small+generic-eps-zero", "forward",
     dict(ws_bytes=16, path=_lib.PATH_GENERIC, prob_fields=dict(eps=0.0)), EINVAL),
    ("model_forward-null-params+ws-too-small", "model_forward", dict(params=None, ws_bytes=16), EINVAL),
]


def _cases(table):
    return [pytest.param(entry, over, code, id=name) for name, entry, over, code in table]


@pytest.mark.parametrize("entry,over,code", _cases(SINGLE))
def test_single_refusals(entry, over, code):
    assert _call(entry, **over) == code


@pytest.mark.parametrize("entry,over,code", _cases(ORDER))
def test_order_of_refusals(entry, over, code):
    assert _call(entry, **over) == code
