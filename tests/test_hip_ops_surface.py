"""CPU-only checks of the Python boundary in neural_svd_amd/hip_ops.py: one call path into the C ABI (`_call`), the
device guard on every wrapper that reaches it, and the helpers that turn tensors and shapes into C arguments (`_ws`,
`_desc`). Nothing here launches a kernel: the refusals come before any address is taken."""
import inspect
import types

import pytest
import torch

from neural_svd_amd import _lib
from neural_svd_amd import hip_ops as H

NEWLY_GUARDED = ("rbf_apply_pair", "evd_gather_heads", "evd_gather_head_blocks")


def _names(code: types.CodeType) -> set:
    """the global / attribute names a code object reads, nested code objects (lambdas, comprehensions) included"""
    out = set(code.co_names)
    for c in code.co_consts:
        if isinstance(c, types.CodeType):
            out |= _names(c)
    return out


def _unwrapped(fn):
    while hasattr(fn, "__wrapped__"):
        fn = fn.__wrapped__
    return fn


def _module_functions():
    return {n: f for n, f in vars(H).items() if inspect.isfunction(f) and f.__module__ == H.__name__}


def _launchers():
    """names of the module-level functions that reach `_call`: directly, or through a private helper that does"""
    fns = {n: _names(_unwrapped(f).__code__) for n, f in _module_functions().items()}
    reach = {"_call"}
    while True:
        more = {n for n, names in fns.items() if n.startswith("_") and n not in reach and names & reach}
        if not more:
            break
        reach |= more
    return reach, {n for n, names in fns.items() if not n.startswith("_") and names & reach}


def test_every_launching_wrapper_is_guarded():
    helpers, public = _launchers()
    # the helpers the shared bodies live in are found, and so are the wrappers that only reach `_call` through them
    assert {"_apply", "_apply_pair", "_gram", "_eigfunc_eval", "_eigfunc_accumulate"} <= helpers
    assert {"operator_forward", "rbf_apply", "tsgram3_f64", "eigfunc3_eval", "cdk_step", "retrieval_eval"} <= public
    assert set(NEWLY_GUARDED) <= public
    assert len(public) >= 60
    fns = _module_functions()
    unguarded = sorted(n for n in public if not hasattr(fns[n], "__wrapped__"))
    assert not unguarded, f"launching wrappers without @_on_tensor_device: {unguarded}"
    for n in NEWLY_GUARDED:
        assert hasattr(fns[n], "__wrapped__"), n
    # the wrappers of the tensor-level binding's launches are among them (every tb.<op> site has its `_call` twin)
    assert {n for n, f in fns.items() if not n.startswith("_") and n != "torch_binding"
            and "torch_binding" in _names(_unwrapped(f).__code__)} <= public


def test_the_stream_is_read_in_one_place():
    readers = sorted(n for n, f in _module_functions().items() if "_stream" in _names(_unwrapped(f).__code__))
    assert readers == ["_call"]
    for cls in (H._DeviceSchedule, H.StepState, H.OptState, H.GradScaler):
        for n, f in vars(cls).items():
            if inspect.isfunction(f):
                assert "_stream" not in _names(f.__code__), f"{cls.__name__}.{n}"


def test_ws_checks_and_counts_bytes():
    with pytest.raises(_lib.NsvdError, match="ws_next must live on the GPU"):
        H._ws(torch.zeros(1024, dtype=torch.uint8), "ws_next")
    with pytest.raises(_lib.NsvdError, match="ws must live on the GPU"):
        H._ws(torch.zeros(1024, dtype=torch.uint8))
    with pytest.raises(_lib.NsvdError, match="scratch must live on the GPU"):
        H._ws(torch.zeros(8), "scratch", optional=True)
    assert H._ws(None, optional=True) == (None, 0)

    class SaysItIsOnTheGpu(torch.Tensor):  # so that the byte count needs no device: the address goes nowhere
        is_cuda = True
    t = torch.zeros(64, dtype=torch.float32)
    assert H._ws(t.as_subclass(SaysItIsOnTheGpu)) == (t.data_ptr(), 256)  # numel() alone would say 64
    with pytest.raises(_lib.NsvdError, match="ws must be contiguous"):
        H._ws(torch.zeros(8, 8).t().as_subclass(SaysItIsOnTheGpu))


def test_desc_is_built_once_per_shape():
    a = H.ModelShape(L=4, D=3, m=16, hidden=(32, 24), has_exp_mask=True, box_mask=H.BOX_EXP, box_lim=2.5)
    b = H.ModelShape(L=4, D=3, m=16, hidden=[32, 24], has_exp_mask=True, box_mask=H.BOX_EXP, box_lim=2.5)
    assert a == b and H._desc(a)._obj is H._desc(b)._obj
    d, fresh = H._desc(a)._obj, a.desc()
    assert fresh is not d and a.desc() is not fresh  # ModelShape.desc() keeps returning a struct of the caller's own
    for got in (d, fresh):
        assert (got.L, got.D, got.m, got.nlayers, list(got.dims)[:3]) == (4, 3, 16, 3, [32, 24, 1])
        assert (got.has_exp_mask, got.box_mask, got.box_lim) == (1, H.BOX_EXP, 2.5)
    assert H._desc(H.ModelShape(L=5, D=3, m=16, hidden=(32, 24)))._obj is not d
    too_deep = H.ModelShape(L=4, D=2, m=16, hidden=(8,) * _lib.NSVD_MAX_LAYERS)
    for build in (too_deep.desc, lambda: H._desc(too_deep), lambda: H.workspace_bytes(too_deep, 32)):
        with pytest.raises(_lib.NsvdError, match=f"at most {_lib.NSVD_MAX_LAYERS} layers"):
            build()


def test_u64_wraps_as_the_masks_did():
    assert H._u64(-1) == 2 ** 64 - 1 and H._u64(2 ** 64 + 5) == 5 and H._u64(7) == 7
