"""Tensor-level wrappers over the C ABI (``include/nsvd.h``): validation, pointers, current stream.

PyTorch is used here only as plumbing (device memory + the current HIP stream). Every function
requires contiguous float32 tensors on a GPU and raises otherwise - there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (MASK_CUSTOM, MASK_JOINT, MASK_SEQUENTIAL, PATH_AUTO, PATH_FUSED, PATH_FUSED_BF16X3,  # noqa: F401
                   PATH_GENERIC, PATH_GENERIC_EXACT, GT_HYDROGEN2D, GT_HARMONIC2D, GT_WELL2D, GT_HYDROGEN3D,
                   BOX_EXP, BOX_NONE, BOX_SQRT, IMP_GAUSSIAN, IMP_NONE, IMP_UNIFORM, POT_HARMONIC, POT_HYDROGEN, POT_ZERO, POT_COSINE, POT_H2_ION, POT_SIN_OF_COS, POT_MOLECULE, OP_SCHROEDINGER, OP_FOKKER_PLANCK,
                   ModelDesc, NsvdError, Params, Problem, check)


# ---- which binding carries the hot-path calls: ctypes (default) or the tensor-level torch extension -----------------
_TB = None
_TB_SHAPES: dict = {}


def torch_binding():
    """The tensor-level binding neural_svd_amd/_nsvd_torch.so (csrc/torch_binding.cpp: tensors checked in C++, current
    HIP stream taken in C++, the same C ABI underneath) when NSVD_BINDING=torch, else None. Like the ctypes binding it
    fails loudly when its shared object is missing."""
    global _TB
    if os.environ.get("NSVD_BINDING", "ctypes") != "torch":
        return None
    if _TB is None:
        import importlib.util
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_nsvd_torch.so")
        if not os.path.exists(path):
            raise NsvdError(f"{path} not found: NSVD_BINDING=torch needs the torch binding built "
                            f"(`make -C neural_svd_amd/csrc torch_binding`, or __graft_entry__.build())")
        _lib.load()  # libnsvd_hip.so first: the extension links against it
        spec = importlib.util.spec_from_file_location("_nsvd_torch", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if mod.abi_version() != _lib.ABI_VERSION:
            raise NsvdError("torch binding built against another ABI version; rebuild the extension")
        _TB = mod
    return _TB


def _tb_shape(shape: "ModelShape"):
    sh = _TB_SHAPES.get(shape)
    if sh is None:
        sh = _TB_SHAPES[shape] = _TB.Shape(shape.L, shape.D, shape.m, list(shape.dims), bool(shape.has_exp_mask),
                                               int(shape.box_mask), float(shape.box_lim))
    return sh


def _tb_params(shape: "ModelShape", params: Params):
    """the extension's ParamSet twin of a packed parameter set (built once, from the tensors pack_params pinned)"""
    ps = getattr(params, "_tb", None)
    if ps is None:
        ws, bs, fB, sc = params._keepalive
        ps = params._tb = _TB.ParamSet(_tb_shape(shape), list(ws), list(bs), fB, sc)
    return ps


def _tb_problem(prob: Problem):
    q = getattr(prob, "_tb", None)
    if q is None:
        if prob.pot_table and getattr(prob, "_pot_table", None) is None:
            # the binding takes the table as a tensor: a struct whose pointer was set by hand would silently become a
            # null-table problem here - make_problem(pot_table=) is the way in for both bindings
            raise NsvdError("Problem.pot_table was set directly: build the problem with make_problem(pot_table=tensor) "
                            "so that the tensor binding receives the table too")
        q = prob._tb = _TB.Problem(prob.potential, prob.charge_or_k, prob.eps, prob.op_scale, prob.op_shift, prob.sigma,
                                   prob.scale_kinetic, prob.hard_mul_const, int(prob.use_importance),
                                   int(prob.operator_kind), prob.fp_scale, [float(c) for c in prob.pot_coef],
                                   int(prob.n_particles), int(prob.n_nuclei), float(prob.pot_const),
                                   getattr(prob, "_pot_table", None))
    return q


def _ptr(t: Optional[torch.Tensor], name: str = "tensor", dtype: torch.dtype = torch.float32) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise NsvdError(f"{name} must live on the GPU (got {t.device}); neural_svd_amd has no CPU path")
    if t.dtype != dtype:
        raise NsvdError(f"{name} must be {str(dtype).replace('torch.', '')} (got {t.dtype})")
    if not t.is_contiguous():
        raise NsvdError(f"{name} must be contiguous")
    return t.data_ptr()


def _ws(t: Optional[torch.Tensor], name: str = "ws", optional: bool = False) -> Tuple[Optional[int], int]:
    """(address, bytes) of a workspace or scratch tensor of any dtype: on the GPU and contiguous, as `_ptr` asks of
    every other tensor; (None, 0) for an absent optional one. Size and alignment are the library's to judge."""
    if t is None and optional:
        return None, 0
    if not t.is_cuda:
        raise NsvdError(f"{name} must live on the GPU (got {t.device}); neural_svd_amd has no CPU path")
    if not t.is_contiguous():
        raise NsvdError(f"{name} must be contiguous")
    return t.data_ptr(), t.nbytes


def _u64(v) -> int:
    """a seed or counter as the uint64 the entry points take"""
    return int(v) & (2 ** 64 - 1)


def _stream() -> int:
    """The current HIP stream of the CURRENT device. Read by `_call` alone; every wrapper that reaches `_call` carries
    `@_on_tensor_device` on its def (tests/test_hip_ops_surface.py), which makes the tensors' device the current one
    first (the C library never calls hipSetDevice)."""
    return torch.cuda.current_stream().cuda_stream


_ENTRY: dict = {}


def _call(name: str, *args) -> None:
    """The one way into a launching entry point: nsvd_<name>(*args, current stream), its return code checked. (The
    typed function is kept by name and `check` entered on failure only: this frame is on the path of every step.)"""
    fn = _ENTRY.get(name)
    if fn is None:
        full = "nsvd_" + name  # (the dense pair's entry points are libnsvd_dense.so's: include/nsvd_dense.h)
        fn = _ENTRY[name] = getattr(_lib.load_dense() if full in _lib.DENSE_SIGNATURES else _lib.load(), full)
    rc = fn(*args, _stream())
    if rc != 0:
        check(rc, "nsvd_" + name)


def _on_tensor_device(fn):
    """Run ``fn`` with the device of its GPU tensor arguments as the current device (so that `_stream()` is a stream
    of THAT device and the kernels launch where the pointers live); tensors of one call must share a device."""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        dev = None
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, (tuple, list)):
                cand = [t for t in a if isinstance(t, torch.Tensor)]
            else:
                cand = [a] if isinstance(a, torch.Tensor) else []
            for t in cand:
                if not t.is_cuda:
                    continue
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise NsvdError(f"{fn.__name__}: tensors on different devices ({dev} and {t.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return guarded


@dataclass(frozen=True)
class ModelShape:
    """Shape of WaveFunctions(ParallelMLP(FourierFeatures)); ``hidden`` excludes the final width 1.
    box_mask / box_lim: the Dirichlet box mask (BOX_SQRT / BOX_EXP on [-box_lim, box_lim]^D), alone or inside the
    exponential mask; it has no parameters."""
    L: int
    D: int
    m: int
    hidden: Tuple[int, ...]
    has_exp_mask: bool = False
    box_mask: int = 0
    box_lim: float = 0.0

    def __post_init__(self):
        object.__setattr__(self, "hidden", tuple(self.hidden))  # a list would leave the shape unhashable (_desc)

    @property
    def dims(self) -> Tuple[int, ...]:
        return tuple(self.hidden) + (1,)

    def desc(self) -> ModelDesc:
        d = ModelDesc()
        d.L, d.D, d.m = self.L, self.D, self.m
        dims = self.dims
        if len(dims) > _lib.NSVD_MAX_LAYERS:
            raise NsvdError(f"at most {_lib.NSVD_MAX_LAYERS} layers are supported")
        d.nlayers = len(dims)
        for i, h in enumerate(dims):
            d.dims[i] = h
        d.has_exp_mask = int(self.has_exp_mask)
        d.box_mask = int(self.box_mask)
        d.box_lim = float(self.box_lim)
        return d

    def param_shapes(self) -> List[Tuple[int, ...]]:
        """Trainable tensors in the reference's parameter order: ws..., bs..., [scales]."""
        shapes, prev = [], 2 * self.m
        for h in self.dims:
            shapes.append((self.L, h, prev))
            prev = h
        for h in self.dims:
            shapes.append((self.L, h, 1))
        if self.has_exp_mask:
            shapes.append((self.L,))
        return shapes


_DESCS: dict = {}


def _desc(shape: ModelShape):
    """byref of shape's nsvd_model_desc, built once per shape (frozen here, const in every entry point)"""
    ref = _DESCS.get(shape)
    if ref is None:
        ref = _DESCS[shape] = C.byref(shape.desc())
    return ref


def make_problem(potential: int, charge_or_k: float, eps: float, op_scale: float, op_shift: float, sigma: float,
                 scale_kinetic: float = 1.0, hard_mul_const: float = 1.0, use_importance: bool = True,
                 importance_kind: Optional[int] = None, operator_kind: int = OP_SCHROEDINGER, fp_scale: float = 0.0,
                 pot_coef: Sequence[float] = (), n_particles: int = 0, pot_table: Optional[torch.Tensor] = None,
                 n_nuclei: int = 0, pot_const: float = 0.0) -> Problem:
    """importance_kind (IMP_NONE / IMP_GAUSSIAN / IMP_UNIFORM) names the density when given; otherwise use_importance
    chooses between none and the Gaussian. ``sigma`` is the sampling scale of either density. ``pot_coef``: cs of
    POT_COSINE / POT_SIN_OF_COS (one per input dimension) or (R,) of POT_H2_ION; ``operator_kind`` OP_FOKKER_PLANCK
    (with POT_SIN_OF_COS) applies fp_scale (Lap f + grad V . grad f + f Lap V) instead of the Hamiltonian.
    ABI 5: ``n_particles`` electrons share the D coordinates (0 is read as 1); ``pot_table`` is a float32 DEVICE tensor,
    kept alive by the returned object - cs[0..D) of POT_COSINE / POT_SIN_OF_COS above 4 input dimensions, or the
    ``n_nuclei`` rows (R_0, .., R_{d-1}, Z) of POT_MOLECULE, whose nuclear repulsion energy is ``pot_const``."""
    p = Problem()
    p.potential = int(potential)
    p.charge_or_k = float(charge_or_k)
    p.scale_kinetic = float(scale_kinetic)
    p.eps = float(eps)
    p.op_scale = float(op_scale)
    p.op_shift = float(op_shift)
    p.sigma = float(sigma)
    p.hard_mul_const = float(hard_mul_const)
    if importance_kind is None:
        importance_kind = IMP_GAUSSIAN if use_importance else IMP_NONE
    if int(importance_kind) not in (IMP_NONE, IMP_GAUSSIAN, IMP_UNIFORM):
        raise NsvdError(f"importance_kind {importance_kind}: IMP_NONE, IMP_GAUSSIAN or IMP_UNIFORM")
    p.use_importance = int(importance_kind)
    if len(pot_coef) > 4:
        raise NsvdError(f"pot_coef: at most 4 coefficients (the stencil's input dimensions), got {len(pot_coef)}")
    p.operator_kind = int(operator_kind)
    p.fp_scale = float(fp_scale)
    for i, c in enumerate(pot_coef):
        p.pot_coef[i] = float(c)
    p.n_particles = int(n_particles)
    p.n_nuclei = int(n_nuclei)
    p.pot_const = float(pot_const)
    if pot_table is not None:
        p.pot_table = _ptr(pot_table, "pot_table")
        p.pot_table_len = int(pot_table.numel())
        p._pot_table = pot_table  # the struct holds a raw address: pin the tensor to it
    return p


def pack_params(shape: ModelShape, ws: Sequence[torch.Tensor], bs: Sequence[torch.Tensor],
                fourier_B: Optional[torch.Tensor], scales: Optional[torch.Tensor]) -> Params:
    """Fill an ``nsvd_params`` struct after checking every tensor against ``shape``."""
    dims = shape.dims
    if len(ws) != len(dims) or len(bs) != len(dims):
        raise NsvdError("number of weight/bias tensors does not match the model shape")
    p = Params()
    if fourier_B is not None:
        if tuple(fourier_B.shape) != (shape.D, shape.m):
            raise NsvdError(f"fourier_B must be {(shape.D, shape.m)}, got {tuple(fourier_B.shape)}")
        p.fourier_B = _ptr(fourier_B, "fourier_B")
    prev = 2 * shape.m
    for i, h in enumerate(dims):
        if tuple(ws[i].shape) != (shape.L, h, prev):
            raise NsvdError(f"W[{i}] must be {(shape.L, h, prev)}, got {tuple(ws[i].shape)}")
        if ws[i].numel() != 0 and bs[i].numel() != shape.L * h:
            raise NsvdError(f"b[{i}] must have {shape.L * h} elements")
        p.W[i] = _ptr(ws[i], f"W[{i}]")
        p.b[i] = _ptr(bs[i], f"b[{i}]")
        prev = h
    if shape.has_exp_mask:
        if scales is None or scales.numel() != shape.L:
            raise NsvdError("scales (L,) required when has_exp_mask")
        p.scales = _ptr(scales, "scales")
    # the struct only holds raw addresses: pin the tensors to it so a temporary (e.g. `fB.to(dev)`)
    # cannot be freed and recycled by the caching allocator while the struct is still in use
    p._keepalive = (list(ws), list(bs), fourier_B, scales)
    return p


def workspace_bytes(shape: ModelShape, B: int) -> int:
    n = _lib.load().nsvd_workspace_bytes(_desc(shape), int(B))
    if n == 0:
        raise NsvdError("nsvd_workspace_bytes: invalid model description")
    return int(n)


def path_name(shape: ModelShape, B: int, path: int = PATH_AUTO, prob: Optional[Problem] = None) -> str:
    """"fused_mfma" / "generic" / "generic_exact" (PATH_GENERIC_EXACT with eps <= 0) (/ "unsupported": e.g. the
    exact-Laplacian mode on a shape the MFMA path does not take, under any path value but PATH_GENERIC_EXACT)."""
    if prob is not None:
        return _lib.load().nsvd_path_name_for(_desc(shape), C.byref(prob), int(B), int(path)).decode()
    return _lib.load().nsvd_path_name(_desc(shape), int(B), int(path)).decode()


def step_emits_planes(shape: ModelShape, B: int, path: int) -> bool:
    """Does a fused training step on this shape and path leave the bf16 planes of the updated weights for the next
    forward (operator_forward(planes_ready=True))? PATH_FUSED_BF16X3, MFMA shapes, no batch slices."""
    return bool(_lib.load().nsvd_step_emits_planes(_desc(shape), int(B), int(path)))


def new_workspace(shape: ModelShape, B: int, device) -> torch.Tensor:
    return torch.empty(workspace_bytes(shape, B), dtype=torch.uint8, device=device)


@_on_tensor_device
def fourier_features(x: torch.Tensor, fourier_B: torch.Tensor, eps: float, nstencil: int) -> torch.Tensor:
    B, D = x.shape
    m = fourier_B.shape[1]
    R = nstencil * B
    out = torch.empty((2 * m, R), dtype=torch.float32, device=x.device)
    _call("fourier_features", _ptr(x, "x"), _ptr(fourier_B, "fourier_B"), _ptr(out), B, D, m, float(eps), int(nstencil), R)
    return out


@_on_tensor_device
def fourier_features_jets(x: torch.Tensor, fourier_B: torch.Tensor) -> torch.Tensor:
    """The jet of the Fourier map as PATH_GENERIC_EXACT lays it out: (2m, (D + 2) B) - block 0 [sin | cos](x B), block
    1 + d the derivative along x_d, block D + 1 the Laplacian (nsvd_fourier_features_jets)."""
    B, D = x.shape
    m = fourier_B.shape[1]
    if tuple(fourier_B.shape) != (D, m):
        raise NsvdError(f"fourier_B must be ({D}, m), got {tuple(fourier_B.shape)}")
    R = (D + 2) * B
    out = torch.empty((2 * m, R), dtype=torch.float32, device=x.device)
    _call("fourier_features_jets", _ptr(x, "x"), _ptr(fourier_B, "fourier_B"), _ptr(out), B, D, m, R)
    return out


@_on_tensor_device
def softplus_jets_inplace(z: torch.Tensor, B: int, D: int) -> torch.Tensor:
    """z (rows, (D + 2) B), the jet of a hidden layer's pre-activations, becomes the jet of its activations in place
    (nsvd_softplus_jets_inplace); returns z."""
    if z.dim() != 2 or z.shape[1] != (D + 2) * B:
        raise NsvdError(f"z must be (rows, {(D + 2) * B}), got {tuple(z.shape)}")
    _call("softplus_jets_inplace", _ptr(z, "z"), z.shape[0], int(B), int(D))
    return z


@_on_tensor_device
def operator_forward(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, ws: torch.Tensor,
                     save_for_backward: bool = True, path: int = PATH_AUTO,
                     out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                     features_ready: bool = False, planes_ready: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Tf, f = operator(model, x, importance). Returns (f, Tf), each (B, L).
    planes_ready (PATH_FUSED_BF16X3): the bf16 planes of the current weights are in `ws` already, left there by the
    fused training step that produced these weights (step_emits_planes; include/nsvd.h: NSVD_W_PLANES_READY)."""
    B = x.shape[0]
    if x.dim() != 2 or x.shape[1] != shape.D:
        raise NsvdError(f"x must be (B, {shape.D})")
    if ((B % 32 != 0 or B > 8192) and not save_for_backward and not features_ready and B > 0 and path != PATH_GENERIC
            and path_name(shape, 32, path, prob) == "fused_mfma"):
        # EVALUATION batches of any size on a model the MFMA kernels take (they want a multiple of 32 rows, at most
        # 8192 of them without a backward layout): in pieces of <= 8192 rows, the last one padded with copies of its
        # last row, and the padding dropped again - a row never sees its neighbours (bit-exact row equivariance is a
        # test). The exact-Laplacian mode exists on that path only; in stencil mode it keeps the reference's validation
        # batches (not multiples of 32 rows) on the fast kernels (the generic ones compute the same even / odd stencil
        # with FMA GEMMs, several times slower).
        fs, Tfs = [], []
        wsc = None
        for i in range(0, B, 8192):
            xc = x[i:i + 8192]
            n = xc.shape[0]
            npad = (n + 31) // 32 * 32
            if npad != n:
                xc = torch.cat([xc, xc[-1:].expand(npad - n, -1)])
            if wsc is None or wsc.numel() < workspace_bytes(shape, npad):
                wsc = new_workspace(shape, npad, x.device)
            fp, Tfp = operator_forward(shape, params, prob, xc.contiguous(), wsc, False, path)
            fs.append(fp[:n])
            Tfs.append(Tfp[:n])
        fa, Tfa = torch.cat(fs), torch.cat(Tfs)
        if out is not None:
            out[0].copy_(fa)
            out[1].copy_(Tfa)
            return out
        return fa, Tfa
    if out is None:
        f = torch.empty((B, shape.L), dtype=torch.float32, device=x.device)
        Tf = torch.empty_like(f)
    else:
        f, Tf = out
    flags = int(save_for_backward) | (_lib.FEATURES_READY if features_ready else 0) | \
        (_lib.W_PLANES_READY if planes_ready else 0)
    tb = torch_binding()
    if tb is not None:
        tb.operator_forward(_tb_shape(shape), _tb_params(shape, params), _tb_problem(prob), x, f, Tf, ws, flags, int(path))
        return f, Tf
    _call("operator_forward", _desc(shape), C.byref(params), C.byref(prob), _ptr(x, "x"), B, _ptr(f, "f"),
          _ptr(Tf, "Tf"), *_ws(ws), flags, int(path))
    return f, Tf


@_on_tensor_device
def operator_features(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, ws: torch.Tensor,
                      save_for_backward: bool = True, path: int = PATH_AUTO) -> None:
    """Weight-independent prologue of operator_forward (Fourier features of x into ws)."""
    _call("operator_features", _desc(shape), C.byref(params), C.byref(prob), _ptr(x, "x"), x.shape[0], *_ws(ws),
          int(save_for_backward), int(path))


def _sample_features(shape, params, prob, seed, offset, state, x, ws, save_for_backward, path) -> None:
    """operator_sample_features (state None) / _dev: one entry point of the tensor binding, two of the C ABI"""
    tb = torch_binding()
    if tb is not None:
        tb.operator_sample_features(_tb_shape(shape), _tb_params(shape, params), _tb_problem(prob), _u64(seed),
                                    _u64(offset), state.buf if state is not None else None, x, ws,
                                    bool(save_for_backward), int(path))
        return
    _call("operator_sample_features" if state is None else "operator_sample_features_dev", _desc(shape),
          C.byref(params), C.byref(prob), _u64(seed), _u64(offset), *(() if state is None else (state.ptr,)),
          _ptr(x, "x"), x.shape[0], *_ws(ws), int(bool(save_for_backward)), int(path))


@_on_tensor_device
def operator_sample_features(shape: ModelShape, params: Params, prob: Problem, seed: int, offset: int,
                             x: torch.Tensor, ws: torch.Tensor, save_for_backward: bool = True,
                             path: int = PATH_AUTO) -> None:
    """x <- sigma * N(0, 1) (counter-based, keyed by seed / offset) and its features into ws, one launch."""
    _sample_features(shape, params, prob, seed, offset, None, x, ws, save_for_backward, path)


@_on_tensor_device
def operator_sample_features_dev(shape: ModelShape, params: Params, prob: Problem, seed: int, offset_base: int,
                                 state: "StepState", x: torch.Tensor, ws: torch.Tensor,
                                 save_for_backward: bool = True, path: int = PATH_AUTO) -> None:
    """operator_sample_features whose batch counter is offset_base + state.step, read on the device."""
    _sample_features(shape, params, prob, seed, offset_base, state, x, ws, save_for_backward, path)


@_on_tensor_device
def operator_backward(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, df: torch.Tensor,
                      grads: Params, ws: torch.Tensor, path: int = PATH_AUTO) -> None:
    B = x.shape[0]
    if tuple(df.shape) != (B, shape.L):
        raise NsvdError(f"df must be {(B, shape.L)}")
    tb = torch_binding()
    if tb is not None:
        tb.operator_backward(_tb_shape(shape), _tb_params(shape, params), _tb_problem(prob), x, df,
                             _tb_params(shape, grads), ws, int(path))
        return
    _call("operator_backward", _desc(shape), C.byref(params), C.byref(prob), _ptr(x, "x"), B, _ptr(df, "df"),
          C.byref(grads), *_ws(ws), int(path))


@_on_tensor_device
def model_forward(shape: ModelShape, params: Params, x: torch.Tensor, hard_mul_const: float,
                  ws: torch.Tensor, save_for_backward: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B = x.shape[0]
    if out is None:
        out = torch.empty((B, shape.L), dtype=torch.float32, device=x.device)
    _call("model_forward", _desc(shape), C.byref(params), _ptr(x, "x"), B, float(hard_mul_const), _ptr(out), *_ws(ws),
          int(save_for_backward))
    return out


@_on_tensor_device
def model_backward(shape: ModelShape, params: Params, x: torch.Tensor, dout: torch.Tensor, grads: Params,
                   ws: torch.Tensor) -> None:
    _call("model_backward", _desc(shape), C.byref(params), _ptr(x, "x"), x.shape[0], _ptr(dout, "dout"),
          C.byref(grads), *_ws(ws))


def evd_scratch(B: int, L: int, device) -> torch.Tensor:
    n = int(_lib.load().nsvd_evd_scratch_bytes(int(B), int(L)))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device)


@_on_tensor_device
def evd_moments(f: torch.Tensor, Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                moments: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """moments = [lam_f1 (L*L) | lam_f2 (L*L) | mean_b sum_l v_l f Tf]  with f1, f2 = chunk(f, 2)."""
    B, L = f.shape
    if moments is None:
        moments = torch.empty(2 * L * L + 1, dtype=torch.float32, device=f.device)
    if scratch is None:
        scratch = evd_scratch(B, L, f.device)
    tb = torch_binding()
    if tb is not None:
        tb.evd_moments(f, Tf, int(mask_kind), v, moments, scratch)
        return moments
    _call("evd_moments", _ptr(f, "f"), _ptr(Tf, "Tf"), B, L, int(mask_kind), _ptr(v, "v"), _ptr(moments, "moments"),
          _ws(scratch, "scratch")[0])
    return moments


@_on_tensor_device
def evd_loss_grad(f: torch.Tensor, Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                  M: Optional[torch.Tensor], moments: torch.Tensor, grad_scale: float = 1.0, want_grad: bool = True,
                  loss: Optional[torch.Tensor] = None,
                  df: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    B, L = f.shape
    if loss is None:
        loss = torch.empty(3, dtype=torch.float32, device=f.device)
    if want_grad and df is None:
        df = torch.empty_like(f)
    tb = torch_binding()
    if tb is not None:
        tb.evd_loss_grad(f, Tf, int(mask_kind), v, M, moments, float(grad_scale), loss, df if want_grad else None)
        return loss, (df if want_grad else None)
    _call("evd_loss_grad", _ptr(f, "f"), _ptr(Tf, "Tf"), B, L, int(mask_kind), _ptr(v, "v"), _ptr(M, "M"),
          _ptr(moments, "moments"), float(grad_scale), _ptr(loss, "loss"), _ptr(df, "df") if want_grad else None)
    return loss, (df if want_grad else None)


@_on_tensor_device
def evd_loss_fused(f: torch.Tensor, Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                   M: Optional[torch.Tensor], moments: torch.Tensor, loss: torch.Tensor, df: Optional[torch.Tensor],
                   scratch: torch.Tensor, grad_scale: float = 1.0) -> None:
    """moments + loss + d loss / d f in one call (single GPU: nothing is exchanged in between)."""
    B, L = f.shape
    _call("evd_loss_fused", _ptr(f, "f"), _ptr(Tf, "Tf"), B, L, int(mask_kind), _ptr(v, "v"), _ptr(M, "M"),
          float(grad_scale), _ptr(moments, "moments"), _ptr(loss, "loss"), _ptr(df, "df"), _ws(scratch, "scratch")[0])


@_on_tensor_device
def evd_partial(f: torch.Tensor, Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                scratch: torch.Tensor) -> None:
    B, L = f.shape
    _call("evd_partial", _ptr(f, "f"), _ptr(Tf, "Tf"), B, L, int(mask_kind), _ptr(v, "v"), _ws(scratch, "scratch")[0])


@_on_tensor_device
def evd_gather_heads(gathered: torch.Tensor, f: torch.Tensor, Tf: torch.Tensor, mask_kind: int,
                     v: Optional[torch.Tensor], scratch: Optional[torch.Tensor] = None) -> None:
    """gathered (world, 2, B, L_local) packed [f | Tf] blocks of the ranks -> f, Tf (B, world * L_local); with
    scratch also the partial moments of evd_partial(f, Tf) (same bits), in one launch."""
    W, two, B, Ll = gathered.shape
    if two != 2 or tuple(f.shape) != (B, W * Ll) or tuple(Tf.shape) != (B, W * Ll):
        raise NsvdError("evd_gather_heads: gathered (world, 2, B, L_local), f / Tf (B, world * L_local)")
    _call("evd_gather_heads", _ptr(gathered, "gathered"), int(W), int(B), int(Ll), int(mask_kind), _ptr(v, "v"),
          _ptr(f, "f"), _ptr(Tf, "Tf"), _ws(scratch, "scratch", True)[0])


@_on_tensor_device
def evd_gather_head_blocks(gathered: torch.Tensor, L: int, f: torch.Tensor, Tf: torch.Tensor, mask_kind: int,
                           v: Optional[torch.Tensor], scratch: Optional[torch.Tensor] = None) -> None:
    """gathered (world, 2 * B * ceil(L / world)): rank w's block begins with its packed f (B, n_w) | Tf (B, n_w),
    n_w = L // world + (w < L % world) -> f, Tf (B, L) (+ the partial moments with scratch): any L >= world."""
    W = gathered.shape[0]
    B = f.shape[0]
    Lb = -(-int(L) // W)
    if gathered.dim() != 2 or gathered.shape[1] != 2 * B * Lb or tuple(f.shape) != (B, L) or tuple(Tf.shape) != (B, L):
        raise NsvdError("evd_gather_head_blocks: gathered (world, 2 B ceil(L / world)), f / Tf (B, L)")
    _call("evd_gather_head_blocks", _ptr(gathered, "gathered"), int(W), int(B), int(L), int(mask_kind), _ptr(v, "v"),
          _ptr(f, "f"), _ptr(Tf, "Tf"), _ws(scratch, "scratch", True)[0])


def _evd_check(complaint: str, shape: ModelShape, x: torch.Tensor, f: torch.Tensor, Tf: torch.Tensor,
               moments: Optional[torch.Tensor]) -> None:
    """The shape check the EVD-backward wrappers share: Tf like f, L_total >= shape.L, 2 L_total^2 + 1 moments;
    `complaint` names the caller (who checks what is its own behind this, with the same words)."""
    B, L_total = x.shape[0], f.shape[1]
    if tuple(Tf.shape) != (B, L_total) or L_total < shape.L or \
            (moments is not None and moments.numel() != 2 * L_total * L_total + 1):
        raise NsvdError(complaint)


def _evd_args(shape: ModelShape, params: Params, prob: Optional[Problem], x, f, Tf, mask_kind, v, M, moments,
              moments_reduced, evd_scratch, l_offset, grad_scale, loss, grads: Optional[Params]) -> tuple:
    """The arguments every EVD-backward entry point begins with (include/nsvd.h): desc, params, prob (the model's own
    entry point, prob None, has none), x .. loss, grads."""
    return (_desc(shape), C.byref(params)) + ((C.byref(prob),) if prob is not None else ()) + (
        _ptr(x, "x"), x.shape[0], _ptr(f, "f"), _ptr(Tf, "Tf"), int(mask_kind), _ptr(v, "v"), _ptr(M, "M"),
        _ptr(moments, "moments"), int(bool(moments_reduced)), _ws(evd_scratch, "evd_scratch", True)[0],
        int(f.shape[1]), int(l_offset), float(grad_scale), _ptr(loss, "loss"),
        C.byref(grads) if grads is not None else None)


def _next_args(next_seed: int, next_offset: int, x_next: Optional[torch.Tensor], ws_next: Optional[torch.Tensor]) -> tuple:
    """next_seed, next_offset, x_next, ws_next, ws_next_bytes of the entry points a next batch can ride in"""
    return (_u64(next_seed), _u64(next_offset), _ptr(x_next, "x_next"), *_ws(ws_next, "ws_next", True))


@_on_tensor_device
def operator_backward_evd(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, f: torch.Tensor,
                          Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor], M: Optional[torch.Tensor],
                          moments: torch.Tensor, moments_reduced: bool, evd_scratch: Optional[torch.Tensor],
                          loss: torch.Tensor, grads: Params, ws: torch.Tensor, grad_scale: float = 1.0,
                          path: int = PATH_AUTO, l_offset: int = 0) -> None:
    """loss gradient + operator backward in one call (d loss / d f is never materialised).
    f, Tf: (B, L_total) with L_total >= shape.L; this model owns heads [l_offset, l_offset + shape.L)."""
    _evd_check("operator_backward_evd: f/Tf must be (B, L_total), moments 2*L_total^2+1", shape, x, f, Tf, moments)
    _call("operator_backward_evd",
          *_evd_args(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads), *_ws(ws), int(path))


def backward_head_window_ok(shape: ModelShape, prob: Problem, B: int, path: int, l_count: int) -> bool:
    return bool(_lib.load().nsvd_backward_head_window_ok(_desc(shape), C.byref(prob), int(B), int(path), int(l_count)))


@_on_tensor_device
def operator_backward_evd_heads(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, f: torch.Tensor,
                                Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                                M: Optional[torch.Tensor], moments: torch.Tensor, moments_reduced: bool,
                                evd_scratch: Optional[torch.Tensor], loss: torch.Tensor, grads: Params,
                                ws: torch.Tensor, l_begin: int, l_count: int, grad_scale: float = 1.0,
                                path: int = PATH_AUTO, l_offset: int = 0) -> None:
    """operator_backward_evd for the heads [l_begin, l_begin + l_count) only (the other gradients are untouched)."""
    _evd_check("operator_backward_evd_heads: f/Tf must be (B, L_total), moments 2*L_total^2+1", shape, x, f, Tf, moments)
    _call("operator_backward_evd_heads",
          *_evd_args(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads), *_ws(ws), int(path), int(l_begin), int(l_count))


class _DeviceSchedule:
    """What StepState and OptState share: the device buffer of the library's struct (host mirror `_mirror`), and the
    library's nsvd_`_entry`_init (with the subclass' `_init_args`) / nsvd_`_entry`_begin on it."""
    _mirror: type = None
    _entry: str = ""

    def __init__(self, device, step: int):
        self.buf = torch.zeros(C.sizeof(self._mirror) // 8, dtype=torch.int64, device=device)
        self.reset(step)

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr()

    def reset(self, step: int) -> None:
        with torch.cuda.device(self.buf.device):
            _call(self._entry + "_init", self.ptr, *self._init_args(int(step)))

    def begin(self) -> None:
        """cur <- the scheduled values of step `step` (loop bodies whose first backward kernel does not do it)"""
        with torch.cuda.device(self.buf.device):
            _call(self._entry + "_begin", self.ptr)

    def read(self):
        """host copy, as the `_lib` mirror of the struct (synchronises)"""
        return self._mirror.from_buffer_copy(self.buf.cpu().numpy().tobytes())


class StepState(_DeviceSchedule):
    """The device-resident schedule state (include/nsvd.h: nsvd_step_state): step counter, CosineAnnealingLR /
    RMSprop / torch_ema constants and the scheduled values of the step being taken, in DEVICE memory - what lets a
    captured training step replay along the schedule (examples/operator/__init__.py:69-73)."""
    _mirror, _entry = _lib.StepState, "step_state"

    def __init__(self, device, lr0: float, T_max: int, alpha: float, eps: float, ema_decay: float, eta_min: float = 0.0,
                 step: int = 0):
        self.args = (float(lr0), float(eta_min), int(T_max), float(alpha), float(eps), float(ema_decay))
        super().__init__(device, step)

    def _init_args(self, step: int) -> tuple:
        return self.args + (step,)


def rmsprop_state(sq: Params, ema: Optional[Params], lr: float, alpha: float, eps: float,
                  ema_decay: float = 0.0, state: Optional[StepState] = None) -> _lib.Rmsprop:
    """nsvd_rmsprop for operator_backward_evd_step; sq / ema are pack_params() sets in the parameters' layouts.
    state: the device-resident schedule - lr / ema_decay are then read (and advanced) on the device."""
    o = _lib.Rmsprop()
    o.sq = sq
    if ema is not None:
        o.ema = ema
    o.lr, o.alpha, o.eps, o.ema_decay = float(lr), float(alpha), float(eps), float(ema_decay)
    o.has_ema = int(ema is not None)
    o.state = state.ptr if state is not None else None
    o._keepalive = (sq, ema, state)
    return o


def _tb_rmsprop(shape: ModelShape, opt: "_lib.Rmsprop"):
    sq, ema, state = opt._keepalive
    return _TB.Rmsprop(_tb_params(shape, sq), _tb_params(shape, ema) if ema is not None else None, opt.lr, opt.alpha,
                       opt.eps, opt.ema_decay, state.buf if state is not None else None)


def _tb_evd_step(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                 grad_scale, loss, grads, opt, ws, path, x_next, ws_next, next_seed, next_offset) -> None:
    """operator_backward_evd_step / _step_next through the tensor-level binding (one entry point there: x_next or None)"""
    _TB.operator_backward_evd_step(_tb_shape(shape), _tb_params(shape, params), _tb_problem(prob), x, f, Tf,
                                   int(mask_kind), v, M, moments, bool(moments_reduced), evd_scratch, int(l_offset),
                                   float(grad_scale), loss, _tb_params(shape, grads) if grads is not None else None,
                                   _tb_rmsprop(shape, opt), ws, int(path), x_next, ws_next,
                                   _u64(next_seed), _u64(next_offset))


@_on_tensor_device
def operator_backward_evd_step(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, f: torch.Tensor,
                               Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                               M: Optional[torch.Tensor], moments: torch.Tensor, moments_reduced: bool,
                               evd_scratch: Optional[torch.Tensor], loss: torch.Tensor, grads: Optional[Params],
                               opt: "_lib.Rmsprop", ws: torch.Tensor, grad_scale: float = 1.0,
                               path: int = PATH_AUTO, l_offset: int = 0) -> None:
    """operator_backward_evd + RMSprop/EMA step inside the weight-gradient kernel; params are updated in place."""
    _evd_check("operator_backward_evd_step: f/Tf must be (B, L_total), moments 2*L_total^2+1", shape, x, f, Tf, moments)
    if torch_binding() is not None:
        _tb_evd_step(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads, opt, ws, path, None, None, 0, 0)
        return
    _call("operator_backward_evd_step",
          *_evd_args(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads), C.byref(opt), *_ws(ws), int(path))


@_on_tensor_device
def operator_backward_evd_step_window(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor,
                                      f: torch.Tensor, Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                                      M: Optional[torch.Tensor], moments: Optional[torch.Tensor], moments_reduced: bool,
                                      evd_scratch: Optional[torch.Tensor], loss: torch.Tensor, opt: "_lib.Rmsprop",
                                      ws: torch.Tensor, l_begin: int, l_count: int, last_window: bool,
                                      ev_after_chain: Optional["torch.cuda.Event"] = None, next_seed: int = 0,
                                      next_offset: int = 0, x_next: Optional[torch.Tensor] = None,
                                      ws_next: Optional[torch.Tensor] = None, grad_scale: float = 1.0,
                                      path: int = PATH_AUTO, l_offset: int = 0) -> None:
    """operator_backward_evd_step for the heads [l_begin, l_begin + l_count) of ONE fused step taken as several head
    windows (nsvd_operator_backward_evd_step_window: include/nsvd.h). Launches on the CURRENT stream; ev_after_chain is
    recorded between the window's two launches."""
    ev = None
    if ev_after_chain is not None:
        if ev_after_chain.cuda_event == 0:  # torch creates the hipEvent lazily, at the first record
            ev_after_chain.record()
        ev = ev_after_chain.cuda_event
    _call("operator_backward_evd_step_window",
          *_evd_args(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, None), C.byref(opt), *_ws(ws), int(path), int(l_begin), int(l_count),
          int(bool(last_window)), ev, *_next_args(next_seed, next_offset, x_next, ws_next))


@_on_tensor_device
def operator_backward_evd_step_next(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor,
                                    f: torch.Tensor, Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                                    M: Optional[torch.Tensor], moments: torch.Tensor, moments_reduced: bool,
                                    evd_scratch: Optional[torch.Tensor], loss: torch.Tensor, grads: Optional[Params],
                                    opt: "_lib.Rmsprop", ws: torch.Tensor, next_seed: int, next_offset: int,
                                    x_next: torch.Tensor, ws_next: torch.Tensor, grad_scale: float = 1.0,
                                    path: int = PATH_AUTO, l_offset: int = 0) -> None:
    """operator_backward_evd_step + operator_sample_features(next batch) in the same launches (MFMA path only)."""
    complaint = "operator_backward_evd_step_next: f/Tf (B, L_total), moments 2*L_total^2+1, x_next like x"
    _evd_check(complaint, shape, x, f, Tf, moments)
    if tuple(x_next.shape) != tuple(x.shape):
        raise NsvdError(complaint)
    if torch_binding() is not None:
        _tb_evd_step(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads, opt, ws, path, x_next, ws_next, next_seed, next_offset)
        return
    _call("operator_backward_evd_step_next",
          *_evd_args(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads), C.byref(opt), *_ws(ws), int(path),
          *_next_args(next_seed, next_offset, x_next, ws_next))


def optimizer_state(cfg: "_lib.OptConfig", sq: Optional[Params], mom: Optional[Params], ema: Optional[Params],
                    steps_taken: int = 0, lr: Optional[float] = None, ema_decay: Optional[float] = None,
                    state: Optional["OptState"] = None) -> "_lib.Optimizer":
    """nsvd_optimizer for operator_backward_evd_opt_step; sq / mom / ema are pack_params() sets in the parameters'
    layouts (None for slots the rule has none of); lr / ema_decay: the step's scheduled values when they differ from
    cfg's; state: the device-resident schedule - the step's scalars are then derived (and advanced) on the device."""
    o = _lib.Optimizer()
    o.cfg = cfg
    if lr is not None:
        o.cfg.lr = float(lr)
    if ema_decay is not None:
        o.cfg.ema_decay = float(ema_decay)
    if sq is not None:
        o.sq = sq
    if mom is not None:
        o.mom = mom
    if ema is not None:
        o.ema = ema
    o.has_ema = int(ema is not None)
    o.steps_taken = int(steps_taken)
    o.state = state.ptr if state is not None else None
    o._keepalive = (sq, mom, ema, state)
    return o


@_on_tensor_device
def operator_backward_evd_opt_step(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor,
                                   f: torch.Tensor, Tf: torch.Tensor, mask_kind: int, v: Optional[torch.Tensor],
                                   M: Optional[torch.Tensor], moments: Optional[torch.Tensor], moments_reduced: bool,
                                   evd_scratch: Optional[torch.Tensor], loss: torch.Tensor, grads: Optional[Params],
                                   opt: "_lib.Optimizer", ws: torch.Tensor, grad_scale: float = 1.0,
                                   path: int = PATH_AUTO, l_offset: int = 0, next_seed: int = 0, next_offset: int = 0,
                                   x_next: Optional[torch.Tensor] = None, ws_next: Optional[torch.Tensor] = None) -> None:
    """operator_backward_evd_step for any optimiser rule (nsvd_operator_backward_evd_opt_step); with x_next / ws_next
    the next batch's draw and features ride along as in operator_backward_evd_step_next (MFMA path only)."""
    complaint = "operator_backward_evd_opt_step: f/Tf (B, L_total), moments 2*L_total^2+1, x_next like x"
    _evd_check(complaint, shape, x, f, Tf, moments)
    if x_next is not None and (ws_next is None or tuple(x_next.shape) != tuple(x.shape)):
        raise NsvdError(complaint)
    _call("operator_backward_evd_opt_step",
          *_evd_args(shape, params, prob, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads), C.byref(opt), *_ws(ws), int(path),
          *_next_args(next_seed, next_offset, x_next, ws_next))


@_on_tensor_device
def model_backward_evd_step(shape: ModelShape, params: Params, x: torch.Tensor, f: torch.Tensor, Tf: torch.Tensor,
                            mask_kind: int, v: Optional[torch.Tensor], M: Optional[torch.Tensor],
                            moments: torch.Tensor, moments_reduced: bool, evd_scratch: Optional[torch.Tensor],
                            loss: torch.Tensor, grads: Optional[Params], opt: Optional["_lib.Rmsprop"],
                            ws: torch.Tensor, grad_scale: float = 1.0, l_offset: int = 0) -> None:
    """EVD loss gradient + backward of the plain model evaluation (+ the optimiser step when opt is given) after
    model_forward(save_for_backward=True); Tf is the operator output computed from f (no gradient through it).
    f, Tf: (B, L_total) over ALL heads; shape describes the heads [l_offset, l_offset + shape.L) (head sharding)."""
    B, L = f.shape
    if tuple(Tf.shape) != (B, L) or L < l_offset + shape.L or x.shape[0] != B or moments.numel() != 2 * L * L + 1:
        raise NsvdError("model_backward_evd_step: f, Tf (B, L_total); moments 2 L_total^2 + 1")
    _call("model_backward_evd_step",
          *_evd_args(shape, params, None, x, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch, l_offset,
                     grad_scale, loss, grads), C.byref(opt) if opt is not None else None, *_ws(ws))


def model_workspace(shape: ModelShape, B: int, device) -> torch.Tensor:
    """workspace of model_forward / model_backward alone (no stencil rows; input dimension up to 64)."""
    n = _lib.load().nsvd_model_workspace_bytes(_desc(shape), int(B))
    if n == 0:
        raise NsvdError("nsvd_model_workspace_bytes: invalid model description")
    return torch.empty(n, dtype=torch.uint8, device=device)


@_on_tensor_device
def kernel_apply(K: torch.Tensor, N: int, rows: torch.Tensor, cols: torch.Tensor, f: torch.Tensor, scale: float,
                 ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Kf = scale * K[rows][:, cols] @ f on the MFMA. K: (N_rows >= N, ldk) float32 with ldk >= N rounded up to 64;
    rows (B1), cols (B2): int64; f: (B2, L). Returns (B1, L)."""
    if K.dim() != 2 or not K.is_cuda or K.dtype != torch.float32 or K.stride(1) != 1:
        raise NsvdError("kernel_apply: K must be a 2-D float32 GPU tensor with unit column stride")
    for t, n in ((rows, "rows"), (cols, "cols")):
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
            raise NsvdError(f"kernel_apply: {n} must be a contiguous 1-D int64 GPU tensor")
    B1, B2 = rows.numel(), cols.numel()
    if f.dim() != 2 or f.shape[0] != B2:
        raise NsvdError("kernel_apply: f must be (len(cols), L)")
    L = f.shape[1]
    if ws is None:
        ws = torch.empty(_lib.load().nsvd_kernel_apply_workspace_bytes(int(N), B1, L), dtype=torch.uint8, device=f.device)
    if out is None:
        out = torch.empty((B1, L), dtype=torch.float32, device=f.device)
    _call("kernel_apply", K.data_ptr(), K.stride(0), int(N), rows.data_ptr(), B1, cols.data_ptr(), B2, _ptr(f, "f"), L,
          float(scale), _ptr(out, "out"), *_ws(ws))
    return out


def kernel_apply_pair_workspace(N1: int, N2: int, B1: int, B2: int, L: int, device) -> torch.Tensor:
    """workspace of kernel_apply_pair: with B1p, N2p, Lp = B1, N2, L rounded up to 64 and (RG, CG) =
    kernel_apply_pair_partition(...), 4 * (Lp N2p + Lp B1p + CG B1p Lp + RG N2p Lp) bytes, each term rounded up to 256"""
    n = _lib.load_dense().nsvd_kernel_apply_pair_workspace_bytes(int(N1), int(N2), int(B1), int(B2), int(L))
    if n == 0:
        raise NsvdError(f"nsvd_kernel_apply_pair_workspace_bytes: every size must be positive "
                        f"(N1={N1} N2={N2} B1={B1} B2={B2} L={L})")
    return torch.empty(n, dtype=torch.uint8, device=device)


def kernel_apply_pair_partition(N1: int, N2: int, B1: int, B2: int, L: int) -> Tuple[int, int]:
    """(row groups, column groups) of an nsvd_kernel_apply_pair call of that shape: the runs of 64-row tiles of the
    batch and of columns of A that workgroups own = the partial copies of A[rows, :]^T f and of out_x. Host only."""
    rg, cg = C.c_int(0), C.c_int(0)
    check(_lib.load_dense().nsvd_kernel_apply_pair_partition(int(N1), int(N2), int(B1), int(B2), int(L), C.byref(rg),
                                                       C.byref(cg)), "nsvd_kernel_apply_pair_partition")
    return rg.value, cg.value


@_on_tensor_device
def kernel_apply_pair(A: torch.Tensor, N1: int, N2: int, rows: torch.Tensor, cols: torch.Tensor, g: torch.Tensor,
                      f: torch.Tensor, scale_g: float, scale_f: float, ws: Optional[torch.Tensor] = None,
                      out_x: Optional[torch.Tensor] = None, out_y: Optional[torch.Tensor] = None):
    """Both halves of an SVD step on a stored matrix in one pass (nsvd_kernel_apply_pair), no transposed copy:
    out_x = scale_g * A[rows][:, cols] @ g ("A g", (B1, L)) and out_y = scale_f * A[rows][:, cols]^T @ f ("A^T f",
    (B2, L)). A: (>= N1, lda) float32 on the GPU with unit column stride, lda >= N2 rounded up to 64; rows (B1),
    cols (B2): int64; g: (B2, L), f: (B1, L). Returns (out_x, out_y)."""
    name = "kernel_apply_pair"
    if A.dim() != 2 or not A.is_cuda or A.dtype != torch.float32 or A.stride(1) != 1:
        raise NsvdError(f"{name}: A must be a 2-D float32 GPU tensor with unit column stride")
    N1, N2 = int(N1), int(N2)
    if not (0 < N1 <= A.shape[0]) or not (0 < N2 <= A.shape[1]):
        raise NsvdError(f"{name}: (N1, N2) = ({N1}, {N2}) must be positive and within A {tuple(A.shape)}")
    for t, n in ((rows, "rows"), (cols, "cols")):
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
            raise NsvdError(f"{name}: {n} must be a contiguous 1-D int64 GPU tensor")
    B1, B2 = rows.numel(), cols.numel()
    if g.dim() != 2 or g.shape[0] != B2:
        raise NsvdError(f"{name}: g must be (len(cols), L)")
    L = g.shape[1]
    if tuple(f.shape) != (B1, L):
        raise NsvdError(f"{name}: f must be (len(rows), L) with g's L")
    gp, fp = _ptr(g, "g"), _ptr(f, "f")
    if out_x is None:
        out_x = torch.empty((B1, L), dtype=torch.float32, device=g.device)
    elif tuple(out_x.shape) != (B1, L):
        raise NsvdError(f"{name}: out_x must be (len(rows), L)")
    if out_y is None:
        out_y = torch.empty((B2, L), dtype=torch.float32, device=g.device)
    elif tuple(out_y.shape) != (B2, L):
        raise NsvdError(f"{name}: out_y must be (len(cols), L)")
    ox, oy = _ptr(out_x, "out_x"), _ptr(out_y, "out_y")
    if ws is None:
        ws = torch.empty(max(_lib.load_dense().nsvd_kernel_apply_pair_workspace_bytes(N1, N2, B1, B2, L), 256),
                         dtype=torch.uint8, device=g.device)
    _call(name, A.data_ptr(), A.stride(0), N1, N2, rows.data_ptr(), B1, cols.data_ptr(), B2, gp, fp, L, float(scale_g),
          float(scale_f), ox, oy, *_ws(ws))
    return out_x, out_y


RBF_GAUSSIAN, RBF_EXPONENTIAL = 0, 1  # NSVD_RBF_* (include/nsvd.h)


# ---- matrix-free kernel products (csrc/rbf_apply*.hip, dot_apply*.hip): one body per call shape ----------------------
def _apply_workspace(name: str, B1: int, B2: int, D: int, L: int, device) -> torch.Tensor:
    """workspace of entry point nsvd_<name>"""
    n = getattr(_lib.load(), f"nsvd_{name}_workspace_bytes")(int(B1), int(B2), int(D), int(L))
    if n == 0:
        raise NsvdError(f"nsvd_{name}_workspace_bytes: unsupported shape B1={B1} B2={B2} D={D} L={L} "
                        "(row counts and L >= 1, 1 <= D <= 64)")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _apply_pair_partition(name: str, B1: int, B2: int, D: int, L: int) -> Tuple[int, int]:
    rg, cs = C.c_int(0), C.c_int(0)
    check(getattr(_lib.load(), f"nsvd_{name}_partition")(int(B1), int(B2), int(D), int(L), C.byref(rg), C.byref(cs)),
          f"nsvd_{name}_partition")
    return rg.value, cs.value


def _apply_ws(name: str, B1: int, B2: int, D: int, L: int, device) -> torch.Tensor:
    # (an unsupported shape has no workspace: the entry point itself refuses it, with its own code)
    n = getattr(_lib.load(), f"nsvd_{name}_workspace_bytes")(B1, B2, D, L)
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device)


_RBF_PARAMS, _DOT_PARAMS = (float,), (float, float, int)  # (ell) and (gamma, coef0, degree) as the entry points type them


def _apply(name: str, x, y, f, kind: int, params: tuple, ptypes: tuple, scale: float, ws, out) -> torch.Tensor:
    """the one-sided products: nsvd_<name>(x, y, f, kind, *params, scale) -> out"""
    for t, n in ((x, "x"), (y, "y"), (f, "f")):
        if t.dim() != 2:
            raise NsvdError(f"{name}: {n} must be 2-D")
    B1, D = x.shape
    B2, L = f.shape
    if tuple(y.shape) != (B2, D):
        raise NsvdError(f"{name}: y must be (len(f), D) with x's D")
    xp, yp, fp = _ptr(x, "x"), _ptr(y, "y"), _ptr(f, "f")
    if out is None:
        out = torch.empty((B1, L), dtype=torch.float32, device=f.device)
    elif tuple(out.shape) != (B1, L):
        raise NsvdError(f"{name}: out must be (len(x), L)")
    op = _ptr(out, "out")
    if ws is None:
        ws = _apply_ws(name, B1, B2, D, L, f.device)
    params = tuple(t(v) for t, v in zip(ptypes, params))
    tb = torch_binding()
    if tb is not None:
        getattr(tb, name)(x, y, f, int(kind), *params, float(scale), out, ws)
        return out
    _call(name, xp, B1, yp, B2, D, fp, L, int(kind), *params, float(scale), op, *_ws(ws))
    return out


def _apply_pair(name: str, x, y, g, f, kind: int, params: tuple, ptypes: tuple, scale_g: float, scale_f: float, ws,
                out_x, out_y):
    """the two-sided products: nsvd_<name>(x, y, g, f, kind, *params, scale_g, scale_f) -> (out_x, out_y)"""
    for t, n in ((x, "x"), (y, "y"), (g, "g"), (f, "f")):
        if t.dim() != 2:
            raise NsvdError(f"{name}: {n} must be 2-D")
    B1, D = x.shape
    B2, L = g.shape
    if tuple(y.shape) != (B2, D):
        raise NsvdError(f"{name}: y must be (len(g), D) with x's D")
    if tuple(f.shape) != (B1, L):
        raise NsvdError(f"{name}: f must be (len(x), L) with g's L")
    xp, yp, gp, fp = _ptr(x, "x"), _ptr(y, "y"), _ptr(g, "g"), _ptr(f, "f")
    if out_x is None:
        out_x = torch.empty((B1, L), dtype=torch.float32, device=g.device)
    elif tuple(out_x.shape) != (B1, L):
        raise NsvdError(f"{name}: out_x must be (len(x), L)")
    if out_y is None:
        out_y = torch.empty((B2, L), dtype=torch.float32, device=g.device)
    elif tuple(out_y.shape) != (B2, L):
        raise NsvdError(f"{name}: out_y must be (len(y), L)")
    ox, oy = _ptr(out_x, "out_x"), _ptr(out_y, "out_y")
    if ws is None:
        ws = _apply_ws(name, B1, B2, D, L, g.device)
    params = tuple(t(v) for t, v in zip(ptypes, params))
    tb = torch_binding()
    if tb is not None:
        getattr(tb, name)(x, y, g, f, int(kind), *params, float(scale_g), float(scale_f), out_x, out_y, ws)
        return out_x, out_y
    _call(name, xp, B1, yp, B2, D, gp, fp, L, int(kind), *params, float(scale_g), float(scale_f), ox, oy, *_ws(ws))
    return out_x, out_y


def rbf_apply_workspace(B1: int, B2: int, D: int, L: int, device) -> torch.Tensor:
    return _apply_workspace("rbf_apply", B1, B2, D, L, device)


@_on_tensor_device
def rbf_apply(x: torch.Tensor, y: torch.Tensor, f: torch.Tensor, kind: int, ell: float, scale: float,
              ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = scale * sum_j k(|x_i - y_j|) f[j] without the (B1, B2) kernel matrix (nsvd_rbf_apply). kind:
    RBF_GAUSSIAN k = exp(-d^2 / (2 ell^2)), RBF_EXPONENTIAL k = exp(-d / ell). x: (B1, D), y: (B2, D), f: (B2, L)
    contiguous float32 on the GPU; x may be y. Returns (B1, L)."""
    return _apply("rbf_apply", x, y, f, kind, (ell,), _RBF_PARAMS, scale, ws, out)


def rbf_apply_pair_workspace(B1: int, B2: int, D: int, L: int, device) -> torch.Tensor:
    return _apply_workspace("rbf_apply_pair", B1, B2, D, L, device)


def rbf_apply_pair_partition(B1: int, B2: int, D: int, L: int) -> Tuple[int, int]:
    """(row groups, column slices) of an nsvd_rbf_apply_pair call of that shape: the runs of x tiles and of y rows that
    workgroups own = the partial copies of out_y and of out_x that the call reduces. Host only."""
    return _apply_pair_partition("rbf_apply_pair", B1, B2, D, L)


@_on_tensor_device
def rbf_apply_pair(x: torch.Tensor, y: torch.Tensor, g: torch.Tensor, f: torch.Tensor, kind: int, ell: float,
                   scale_g: float, scale_f: float, ws: Optional[torch.Tensor] = None,
                   out_x: Optional[torch.Tensor] = None, out_y: Optional[torch.Tensor] = None):
    """Both halves of a kernel SVD step in one pass (nsvd_rbf_apply_pair), every kernel value evaluated once:
    out_x[i] = scale_g * sum_j k(|x_i - y_j|) g[j] ("K g", (B1, L)) and out_y[j] = scale_f * sum_i k(|x_i - y_j|) f[i]
    ("K^T f", (B2, L)). kind and ell as rbf_apply. x: (B1, D), y: (B2, D), g: (B2, L), f: (B1, L) contiguous float32 on
    the GPU; x may be y and f may be g. Returns (out_x, out_y)."""
    return _apply_pair("rbf_apply_pair", x, y, g, f, kind, (ell,), _RBF_PARAMS, scale_g, scale_f, ws, out_x, out_y)


DOT_POLYNOMIAL, DOT_ARCCOS1 = 0, 1  # NSVD_DOT_* (include/nsvd.h)
DOT_RELU_NNGP, DOT_RELU_NTK = 3, 4   # (2 is unassigned)


def dot_apply_workspace(B1: int, B2: int, D: int, L: int, device) -> torch.Tensor:
    return _apply_workspace("dot_apply", B1, B2, D, L, device)


@_on_tensor_device
def dot_apply(x: torch.Tensor, y: torch.Tensor, f: torch.Tensor, kind: int, gamma: float, coef0: float, degree: int,
              scale: float, ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = scale * sum_j k(x_i, y_j) f[j] without the (B1, B2) kernel matrix (nsvd_dot_apply). kind:
    DOT_POLYNOMIAL k = (gamma x.y + coef0)^degree (integer degree 1..8), DOT_ARCCOS1 k = |x||y| / pi (sin t +
    (pi - t) cos t) with cos t = x.y / (|x||y|) (gamma, coef0, degree ignored), DOT_RELU_NNGP / DOT_RELU_NTK the NNGP
    kernel S_depth / the neural tangent kernel T_depth of a ReLU network with weight variance gamma > 0, bias variance
    coef0 >= 0 and depth 1..8 PASSED AS ``degree`` (the recursion: include/nsvd.h, kernel_ops.DotKernelOperator; the NTK
    kind carries ~2e-4 per level where cos t = +-1 in float32: diagonals, near-parallel rows, D = 1).
    x: (B1, D), y: (B2, D), f: (B2, L) contiguous float32 on the GPU; x may be y. Returns (B1, L)."""
    return _apply("dot_apply", x, y, f, kind, (gamma, coef0, degree), _DOT_PARAMS, scale, ws, out)


def dot_apply_pair_workspace(B1: int, B2: int, D: int, L: int, device) -> torch.Tensor:
    return _apply_workspace("dot_apply_pair", B1, B2, D, L, device)


def dot_apply_pair_partition(B1: int, B2: int, D: int, L: int) -> Tuple[int, int]:
    """(row groups, column slices) of an nsvd_dot_apply_pair call of that shape: the runs of x tiles and of y rows that
    workgroups own = the partial copies of out_y and of out_x that the call reduces. Host only."""
    return _apply_pair_partition("dot_apply_pair", B1, B2, D, L)


@_on_tensor_device
def dot_apply_pair(x: torch.Tensor, y: torch.Tensor, g: torch.Tensor, f: torch.Tensor, kind: int, gamma: float,
                   coef0: float, degree: int, scale_g: float, scale_f: float, ws: Optional[torch.Tensor] = None,
                   out_x: Optional[torch.Tensor] = None, out_y: Optional[torch.Tensor] = None):
    """Both halves of a kernel SVD step in one pass (nsvd_dot_apply_pair), every x_i . y_j formed and mapped once:
    out_x[i] = scale_g * sum_j k(x_i, y_j) g[j] ("K g", (B1, L)) and out_y[j] = scale_f * sum_i k(x_i, y_j) f[i]
    ("K^T f", (B2, L)). kind, gamma, coef0, degree as dot_apply (the deep ReLU kinds: depth as ``degree``).
    x: (B1, D), y: (B2, D), g: (B2, L), f: (B1, L) contiguous float32 on the GPU; x may be y and f may be g.
    Returns (out_x, out_y)."""
    return _apply_pair("dot_apply_pair", x, y, g, f, kind, (gamma, coef0, degree), _DOT_PARAMS, scale_g, scale_f, ws,
                       out_x, out_y)


# ---- the dense side of the Nystrom baseline (csrc/nystrom.hip; the loop is neural_svd_amd/nystrom.py) ---------------
RITZ_BAD_PIVOT, RITZ_SWEEP_CAP = 1, 2  # NSVD_RITZ_* (include/nsvd.h)
NYSTROM_MAX_BLOCK = 80


def _rows_ptr(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """(pointer, row stride) of a 2-D float32 GPU tensor whose rows are contiguous (a column slice of a wider one may
    come in as it is)"""
    if not t.is_cuda:
        raise NsvdError(f"{name} must live on the GPU (got {t.device}); neural_svd_amd has no CPU path")
    if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise NsvdError(f"{name} must be a 2-D float32 tensor with unit column stride and non-overlapping rows")
    return t.data_ptr(), t.stride(0)


def _gram_workspace(fn: str, n: int, m: int, device) -> torch.Tensor:
    b = getattr(_lib.load(), fn + "_workspace_bytes")(int(n), int(m))
    if b == 0:
        raise NsvdError(f"{fn}_workspace_bytes: unsupported shape n={n} m={m} (n >= 1, 1 <= m <= 80)")
    return torch.empty(b, dtype=torch.uint8, device=device)


def _gram(fn: str, X: torch.Tensor, Y: Optional[torch.Tensor], outs, use, ws: Optional[torch.Tensor]):
    """What tsgram_f64 and tsgram3_f64 share. fn: the C function; outs: the caller's out_xtx, out_xty(, out_yty), each
    allocated when None (those with Y only when Y is given) and checked; use: which of them the call is handed.
    Returns them, None where use is False."""
    name, f64 = fn[len("nsvd_"):], torch.float64
    xp, ldx = _rows_ptr(X, "X")
    n, m = X.shape
    yp, ldy = None, 0
    if Y is not None:
        if tuple(Y.shape) != (n, m):
            raise NsvdError(f"{name}: Y must have X's shape")
        yp, ldy = _rows_ptr(Y, "Y")
    elif not use[0]:
        raise NsvdError(f"{name}: nothing to compute")
    names = ("out_xtx", "out_xty", "out_yty")
    outs = [torch.empty((m, m), dtype=f64, device=X.device) if o is None and u and (i == 0 or Y is not None) else o
            for i, (o, u) in enumerate(zip(outs, use))]
    for o, nm in zip(outs, names):
        if o is not None and tuple(o.shape) != (m, m):
            raise NsvdError(f"{name}: {nm} must be (m, m)")
    if ws is None:
        ws = torch.empty(max(getattr(_lib.load(), fn + "_workspace_bytes")(n, m), 256), dtype=torch.uint8,
                         device=X.device)
    outs = [o if u else None for o, u in zip(outs, use)]
    _call(name, xp, ldx, yp, ldy, n, m, *(_ptr(o, nm, f64) for o, nm in zip(outs, names)), *_ws(ws))
    return outs


def tsgram_workspace(n: int, m: int, device) -> torch.Tensor:
    return _gram_workspace("nsvd_tsgram_f64", n, m, device)


@_on_tensor_device
def tsgram_f64(X: torch.Tensor, Y: Optional[torch.Tensor] = None, xtx: bool = True, ws: Optional[torch.Tensor] = None,
               out_xtx: Optional[torch.Tensor] = None, out_xty: Optional[torch.Tensor] = None):
    """(X^T X, X^T Y) as (m, m) float64 from (n, m) float32 blocks (nsvd_tsgram_f64): products and sums in float64, no
    atomics, bit-reproducible. Y None: only X^T X (the second value is None); xtx False: only X^T Y."""
    return tuple(_gram("nsvd_tsgram_f64", X, Y, (out_xtx, out_xty), (xtx, True), ws))


@_on_tensor_device
def ritz_step_f64(S: torch.Tensor, A: Optional[torch.Tensor], status: torch.Tensor,
                  theta: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                  Q: Optional[torch.Tensor] = None, T: Optional[torch.Tensor] = None,
                  C: Optional[torch.Tensor] = None):
    """The m x m solve of one subspace iteration (nsvd_ritz_step_f64), float64: eigh(sym(A)) = Q diag(theta) Q^T with
    theta descending, M = Q^T S Q, resid_k = sqrt(max(M_kk - theta_k^2 (2 - q_k^T C q_k), 0)) (C None: C = I),
    T = Q chol(M)^-1. A None: Q = I, T = chol(S)^-T. status: (1,) int32, RITZ_* bits are OR-ed in (zero it first).
    Returns (theta, resid, Q, T)."""
    if S.dim() != 2 or S.shape[0] != S.shape[1]:
        raise NsvdError("ritz_step_f64: S must be (m, m)")
    m = S.shape[0]
    dev = S.device
    for o, name in ((A, "A"), (C, "C")):
        if o is not None and tuple(o.shape) != (m, m):
            raise NsvdError(f"ritz_step_f64: {name} must be (m, m)")
    theta = torch.empty(m, dtype=torch.float64, device=dev) if theta is None else theta
    resid = torch.empty(m, dtype=torch.float64, device=dev) if resid is None else resid
    Q = torch.empty((m, m), dtype=torch.float64, device=dev) if Q is None else Q
    T = torch.empty((m, m), dtype=torch.float64, device=dev) if T is None else T
    if theta.numel() != m or resid.numel() != m or tuple(Q.shape) != (m, m) or tuple(T.shape) != (m, m):
        raise NsvdError("ritz_step_f64: theta, resid (m); Q, T (m, m)")
    if status.numel() < 1:
        raise NsvdError("ritz_step_f64: status must hold one int32")
    f64 = torch.float64
    _call("ritz_step_f64", _ptr(S, "S", f64), _ptr(A, "A", f64), _ptr(C, "C", f64), m, _ptr(theta, "theta", f64),
          _ptr(resid, "resid", f64), _ptr(Q, "Q", f64), _ptr(T, "T", f64), _ptr(status, "status", torch.int32))
    return theta, resid, Q, T


@_on_tensor_device
def ts_rotate(X: torch.Tensor, T: torch.Tensor, k: Optional[int] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (n, k) = X (n, m) @ T[:, :k] with T (m, m) float64, accumulated in float64 and rounded once to float32
    (nsvd_ts_rotate). out must not alias X."""
    xp, ldx = _rows_ptr(X, "X")
    n, m = X.shape
    if T.dim() != 2 or T.shape[0] != m or T.stride(1) != 1:
        raise NsvdError("ts_rotate: T must be (m, >= k) float64 with unit column stride")
    k = T.shape[1] if k is None else int(k)
    if out is None:
        out = torch.empty((n, max(k, 0)), dtype=torch.float32, device=X.device)
    elif tuple(out.shape) != (n, k):
        raise NsvdError("ts_rotate: out must be (n, k)")
    op, ldo = _rows_ptr(out, "out")
    if out.data_ptr() == X.data_ptr():
        raise NsvdError("ts_rotate: out must not alias X")
    if T.dtype != torch.float64 or not T.is_cuda:
        raise NsvdError("ts_rotate: T must be a float64 GPU tensor")
    _call("ts_rotate", xp, ldx, n, m, T.data_ptr(), T.stride(0), k, op, ldo)
    return out


# ---- the dense side of the truncated-SVD baseline (csrc/nystrom_svd.hip; the loop is neural_svd_amd/nystrom_svd.py) ---
def tsgram3_workspace(n: int, m: int, device) -> torch.Tensor:
    return _gram_workspace("nsvd_tsgram3_f64", n, m, device)


@_on_tensor_device
def tsgram3_f64(X: torch.Tensor, Y: torch.Tensor, ws: Optional[torch.Tensor] = None,
                out_xtx: Optional[torch.Tensor] = None, out_xty: Optional[torch.Tensor] = None,
                out_yty: Optional[torch.Tensor] = None):
    """(X^T X, X^T Y, Y^T Y) as (m, m) float64 from (n, m) float32 blocks in one pass (nsvd_tsgram3_f64): each row tile
    of X and Y is staged once for all three; products and sums in float64, no atomics, bit-reproducible. X may be Y."""
    return tuple(_gram("nsvd_tsgram3_f64", X, Y, (out_xtx, out_xty, out_yty), (True, True, True), ws))


@_on_tensor_device
def svd_ritz_step_f64(PtU: torch.Tensor, RtV: torch.Tensor, Sp: torch.Tensor, Sr: torch.Tensor, status: torch.Tensor,
                      Cu: Optional[torch.Tensor] = None, Cv: Optional[torch.Tensor] = None,
                      sigma: Optional[torch.Tensor] = None, resid_l: Optional[torch.Tensor] = None,
                      resid_r: Optional[torch.Tensor] = None, A: Optional[torch.Tensor] = None,
                      B: Optional[torch.Tensor] = None, Tu: Optional[torch.Tensor] = None,
                      Tv: Optional[torch.Tensor] = None):
    """The m x m solve of one two-sided block iteration (nsvd_svd_ritz_step_f64), float64: with Hl = PtU^T, Hr = RtV,
    (Hl + Hr) / 2 = A diag(sigma) B^T (sigma descending), Mp = B^T Sp B, Mr = A^T Sr A,
    resid_l_k = sqrt(max(Mp_kk - 2 sigma_k (A^T Hl B)_kk + sigma_k^2 (A^T Cu A)_kk, 0)),
    resid_r_k = sqrt(max(Mr_kk - 2 sigma_k (A^T Hr B)_kk + sigma_k^2 (B^T Cv B)_kk, 0)) (Cu / Cv None: the identity),
    Tu = B chol(Mp)^-1, Tv = A chol(Mr)^-1. status: (1,) int32, RITZ_* bits are OR-ed in (zero it first).
    Returns (sigma, resid_l, resid_r, A, B, Tu, Tv)."""
    if PtU.dim() != 2 or PtU.shape[0] != PtU.shape[1]:
        raise NsvdError("svd_ritz_step_f64: PtU must be (m, m)")
    m = PtU.shape[0]
    dev = PtU.device
    for o, name in ((RtV, "RtV"), (Sp, "Sp"), (Sr, "Sr"), (Cu, "Cu"), (Cv, "Cv")):
        if o is not None and tuple(o.shape) != (m, m):
            raise NsvdError(f"svd_ritz_step_f64: {name} must be (m, m)")
    f64 = torch.float64
    sigma, resid_l, resid_r = (torch.empty(m, dtype=f64, device=dev) if o is None else o
                               for o in (sigma, resid_l, resid_r))
    A, B, Tu, Tv = (torch.empty((m, m), dtype=f64, device=dev) if o is None else o for o in (A, B, Tu, Tv))
    if any(o.numel() != m for o in (sigma, resid_l, resid_r)) or any(tuple(o.shape) != (m, m) for o in (A, B, Tu, Tv)):
        raise NsvdError("svd_ritz_step_f64: sigma, resid_l, resid_r (m); A, B, Tu, Tv (m, m)")
    if status.numel() < 1:
        raise NsvdError("svd_ritz_step_f64: status must hold one int32")
    _call("svd_ritz_step_f64", _ptr(PtU, "PtU", f64), _ptr(RtV, "RtV", f64), _ptr(Sp, "Sp", f64), _ptr(Sr, "Sr", f64),
          _ptr(Cu, "Cu", f64), _ptr(Cv, "Cv", f64), m, _ptr(sigma, "sigma", f64), _ptr(resid_l, "resid_l", f64),
          _ptr(resid_r, "resid_r", f64), _ptr(A, "A", f64), _ptr(B, "B", f64), _ptr(Tu, "Tu", f64), _ptr(Tv, "Tv", f64),
          _ptr(status, "status", torch.int32))
    return sigma, resid_l, resid_r, A, B, Tu, Tv


# ---- SpIN on the kernel-operator path (csrc/spin.hip; the step is neural_svd_amd/spin.py) -----------------------------
SPIN_MAX_L = 64


@_on_tensor_device
def spin_solve(sigma_raw: torch.Tensor, sigma_scale: float, pi_raw: torch.Tensor, pi_scale: float, decay: float,
               gpi_scale: float, sigma_avg: torch.Tensor, chol: torch.Tensor, loss_eigvals: torch.Tensor,
               gsigma: torch.Tensor, gpi_scaled: torch.Tensor, status: torch.Tensor) -> None:
    """Steps 2-5 of SpIN's loss in one workgroup, float64 (nsvd_spin_solve): sigma_avg (L, L) float32 is updated IN
    PLACE with sigma_scale * sigma_raw, chol (L, L) float32 = cholesky(sigma_avg + 1e-3 I); loss_eigvals (1 + L) =
    [trace | diag] of Lambda = chol^-1 (pi_scale pi_raw) chol^-T, gsigma and gpi_scaled = gpi_scale * gpi (L, L), all
    float64. status: (1,) int32, RITZ_BAD_PIVOT is OR-ed in on failure (every output is then zero)."""
    L = sigma_avg.shape[0]
    f64 = torch.float64
    for o, name in ((sigma_raw, "sigma_raw"), (pi_raw, "pi_raw"), (sigma_avg, "sigma_avg"), (chol, "chol"),
                    (gsigma, "gsigma"), (gpi_scaled, "gpi_scaled")):
        if tuple(o.shape) != (L, L):
            raise NsvdError(f"spin_solve: {name} must be ({L}, {L})")
    if loss_eigvals.numel() != L + 1 or status.numel() < 1:
        raise NsvdError("spin_solve: loss_eigvals must hold 1 + L float64 values and status one int32")
    _call("spin_solve", _ptr(sigma_raw, "sigma_raw", f64), float(sigma_scale), _ptr(pi_raw, "pi_raw", f64),
          float(pi_scale), L, float(decay), float(gpi_scale), _ptr(sigma_avg, "sigma_avg"), _ptr(chol, "chol"),
          _ptr(loss_eigvals, "loss_eigvals", f64), _ptr(gsigma, "gsigma", f64), _ptr(gpi_scaled, "gpi_scaled", f64),
          _ptr(status, "status", torch.int32))


@_on_tensor_device
def spinx_solve(S_raw: torch.Tensor, s_scale: float, Gpp_raw: torch.Tensor, Gpk_raw: torch.Tensor, Gkk_raw: torch.Tensor,
                g_scale: float, w: torch.Tensor, trace_w: Optional[torch.Tensor], decay: float, update_state: bool,
                sigma_avg: Optional[torch.Tensor], chol: Optional[torch.Tensor], out64: torch.Tensor, T_s: torch.Tensor,
                T_pp: torch.Tensor, T_kp: torch.Tensor, T_pk: torch.Tensor, T_kk: torch.Tensor,
                status: torch.Tensor) -> None:
    """SpINx's loss and its reverse mode on the four raw (L, L) float64 Grams in one workgroup (nsvd_spinx_solve):
    out64 (2 L + 2) = [loss | losses (L + 1) | eigvals (L)], the five (L, L) float64 matrices of the cotangent products
    dP = P T_pp + K T_kp, dK = P T_pk + K T_kk, dPhi = Phi T_s; w (L + 1) float64 loss weights, trace_w (L) float64 or
    None for ones. update_state: sigma_avg (L, L) float32 takes the moving average IN PLACE and chol its factor;
    otherwise neither is touched. S_raw may be Gpp_raw. status: (1,) int32, RITZ_BAD_PIVOT is OR-ed in on failure (every
    output is then zero)."""
    if S_raw.dim() != 2:
        raise NsvdError("spinx_solve: S_raw must be (L, L)")
    L = S_raw.shape[0]
    f64 = torch.float64
    mats = [(S_raw, "S_raw"), (Gpp_raw, "Gpp_raw"), (Gpk_raw, "Gpk_raw"), (Gkk_raw, "Gkk_raw"), (T_s, "T_s"),
            (T_pp, "T_pp"), (T_kp, "T_kp"), (T_pk, "T_pk"), (T_kk, "T_kk")]
    if update_state:
        if sigma_avg is None or chol is None:
            raise NsvdError("spinx_solve: update_state needs sigma_avg and chol")
        mats += [(sigma_avg, "sigma_avg"), (chol, "chol")]
    for o, name in mats:
        if tuple(o.shape) != (L, L):
            raise NsvdError(f"spinx_solve: {name} must be ({L}, {L})")
    if w.numel() != L + 1 or (trace_w is not None and trace_w.numel() != L):
        raise NsvdError("spinx_solve: w must hold L + 1 and trace_w L float64 values")
    if out64.numel() != 2 * L + 2 or status.numel() < 1:
        raise NsvdError("spinx_solve: out64 must hold 2 L + 2 float64 values and status one int32")
    _call("spinx_solve", _ptr(S_raw, "S_raw", f64), float(s_scale), _ptr(Gpp_raw, "Gpp_raw", f64),
          _ptr(Gpk_raw, "Gpk_raw", f64), _ptr(Gkk_raw, "Gkk_raw", f64), float(g_scale), L, _ptr(w, "w", f64),
          _ptr(trace_w, "trace_w", f64), float(decay), 1 if update_state else 0,
          _ptr(sigma_avg, "sigma_avg") if update_state else None, _ptr(chol, "chol") if update_state else None,
          _ptr(out64, "out64", f64), _ptr(T_s, "T_s", f64), _ptr(T_pp, "T_pp", f64), _ptr(T_kp, "T_kp", f64),
          _ptr(T_pk, "T_pk", f64), _ptr(T_kk, "T_kk", f64), _ptr(status, "status", torch.int32))


@_on_tensor_device
def ts_rotate2(X: torch.Tensor, T1: torch.Tensor, Y: torch.Tensor, T2: torch.Tensor, k: Optional[int] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (n, k) = X (n, m) @ T1[:, :k] + Y (n, m) @ T2[:, :k] with T1, T2 float64, everything accumulated in float64
    and rounded once to float32 (nsvd_ts_rotate2). out must not alias X or Y."""
    xp, ldx = _rows_ptr(X, "X")
    yp, ldy = _rows_ptr(Y, "Y")
    n, m = X.shape
    if tuple(Y.shape) != (n, m):
        raise NsvdError("ts_rotate2: X and Y must have one shape")
    for T in (T1, T2):
        if T.dim() != 2 or T.shape[0] != m or T.stride(1) != 1 or T.dtype != torch.float64 or not T.is_cuda:
            raise NsvdError("ts_rotate2: T1, T2 must be (m, >= k) float64 GPU tensors with unit column stride")
    k = min(T1.shape[1], T2.shape[1]) if k is None else int(k)
    if out is None:
        out = torch.empty((n, max(k, 0)), dtype=torch.float32, device=X.device)
    elif tuple(out.shape) != (n, k):
        raise NsvdError("ts_rotate2: out must be (n, k)")
    op, ldo = _rows_ptr(out, "out")
    if op in (xp, yp):
        raise NsvdError("ts_rotate2: out must not alias X or Y")
    _call("ts_rotate2", xp, ldx, yp, ldy, n, m, T1.data_ptr(), T1.stride(0), T2.data_ptr(), T2.stride(0), k, op, ldo)
    return out


def spin_state_floats(shape: ModelShape) -> int:
    """floats of ONE parameter set of SpIN's compact Jacobian state ([W_0 | .. | b_0 | ..], no padding); J is (L, this)"""
    n = int(_lib.load().nsvd_spin_state_floats(_desc(shape)))
    if n == 0:
        raise NsvdError("nsvd_spin_state_floats: unsupported model (no exponential / box mask, D <= 64, L <= 64)")
    return n


def spin_jac_workspace(shape: ModelShape, B1: int, device) -> torch.Tensor:
    n = int(_lib.load().nsvd_spin_jac_workspace_bytes(_desc(shape), int(B1)))
    if n == 0:
        raise NsvdError("nsvd_spin_jac_workspace_bytes: unsupported model or batch (no exponential / box mask, D <= 64, "
                        "L <= 64, B1 >= 2)")
    return torch.empty(n, dtype=torch.uint8, device=device)


@_on_tensor_device
def spin_jac_step(shape: ModelShape, params: Params, x: torch.Tensor, phi: torch.Tensor, hard_mul_const: float,
                  gsigma: torch.Tensor, decay: float, J: torch.Tensor, grads: Params,
                  ws: Optional[torch.Tensor] = None) -> None:
    """SpIN's second gradient term (nsvd_spin_jac_step): J (L, spin_state_floats) <- (1 - decay) J + decay j_new IN
    PLACE, j_new[a, c] = (2 / B1) sum_b phi[b, a] d model_c(x_b) / d p, and grads += sum_a gsigma[a, c] J[a, c]."""
    B1 = x.shape[0]
    if tuple(x.shape) != (B1, shape.D) or tuple(phi.shape) != (B1, shape.L):
        raise NsvdError(f"spin_jac_step: x must be (B1, {shape.D}) and phi (B1, {shape.L})")
    if tuple(gsigma.shape) != (shape.L, shape.L):
        raise NsvdError(f"spin_jac_step: gsigma must be ({shape.L}, {shape.L})")
    if J.numel() != shape.L * spin_state_floats(shape):
        raise NsvdError("spin_jac_step: J must hold L * spin_state_floats(shape) floats")
    if ws is None:
        ws = spin_jac_workspace(shape, B1, x.device)
    _call("spin_jac_step", _desc(shape), C.byref(params), _ptr(x, "x"), B1, _ptr(phi, "phi"), float(hard_mul_const),
          _ptr(gsigma, "gsigma", torch.float64), float(decay), _ptr(J, "J"), C.byref(grads), *_ws(ws))


def cdk_workspace(B: int, L: int, set_first_mode_const: bool, device) -> torch.Tensor:
    n = _lib.load().nsvd_cdk_workspace_bytes(int(B), int(L), int(bool(set_first_mode_const)))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device)


@_on_tensor_device
def cdk_loss_forward(f: torch.Tensor, g: torch.Tensor, batch_weights: Optional[torch.Tensor], v: torch.Tensor,
                     M: torch.Tensor, set_first_mode_const: bool, loss: torch.Tensor,
                     rs_joint: Optional[torch.Tensor], rs_indep: Optional[torch.Tensor], ws: torch.Tensor) -> None:
    """NestedLoRALossFunctionForCDK.forward: loss (3), rs_joint (B), rs_indep (B(B-1)); state for the backward in ws."""
    B, L = f.shape
    Lp = L + int(bool(set_first_mode_const))
    if tuple(g.shape) != (B, L) or v.numel() != Lp or tuple(M.shape) != (Lp, Lp) or loss.numel() < 3:
        raise NsvdError(f"cdk_loss_forward: f, g (B, L); v ({Lp}); M ({Lp}, {Lp}); loss (3)")
    if batch_weights is not None and batch_weights.numel() != B:
        raise NsvdError("cdk_loss_forward: batch_weights must hold one weight per row")
    if (rs_joint is not None and rs_joint.numel() != B) or (rs_indep is not None and rs_indep.numel() != B * (B - 1)):
        raise NsvdError("cdk_loss_forward: rs_joint (B), rs_indep (B (B-1))")
    _call("cdk_loss_forward", _ptr(f, "f"), _ptr(g, "g"), _ptr(batch_weights, "batch_weights"), _ptr(v, "v"),
          _ptr(M, "M"), B, L, int(bool(set_first_mode_const)), _ptr(loss, "loss"), _ptr(rs_joint, "rs_joint"),
          _ptr(rs_indep, "rs_indep"), *_ws(ws))


@_on_tensor_device
def cdk_loss_backward(v: torch.Tensor, B: int, L: int, set_first_mode_const: bool, grad_out: Optional[torch.Tensor],
                      grad_f: Optional[torch.Tensor], grad_g: Optional[torch.Tensor], ws: torch.Tensor) -> None:
    for t, n in ((grad_f, "grad_f"), (grad_g, "grad_g")):
        if t is not None and tuple(t.shape) != (B, L):
            raise NsvdError(f"cdk_loss_backward: {n} must be (B, L)")
    _call("cdk_loss_backward", _ptr(v, "v"), int(B), int(L), int(bool(set_first_mode_const)),
          _ptr(grad_out, "grad_out"), _ptr(grad_f, "grad_f"), _ptr(grad_g, "grad_g"), *_ws(ws))


@_on_tensor_device
def rmsprop_ema_step(p: torch.Tensor, grad: torch.Tensor, sq: torch.Tensor, ema: Optional[torch.Tensor], lr: float,
                     alpha: float, eps: float, ema_decay: float, grad_scale: float = 1.0) -> None:
    n = _opt_sizes("rmsprop_ema_step", p, grad, sq, None, ema)
    tb = torch_binding()
    if tb is not None:
        tb.rmsprop_ema_step(p, grad, sq, ema, float(lr), float(alpha), float(eps), float(ema_decay), float(grad_scale))
        return
    _call("rmsprop_ema_step", _ptr(p, "p"), _ptr(grad, "grad"), _ptr(sq, "sq"), _ptr(ema, "ema"), n, float(lr),
          float(alpha), float(eps), float(ema_decay), float(grad_scale))


@_on_tensor_device
def rmsprop_ema_step_dev(p: torch.Tensor, grad: torch.Tensor, sq: torch.Tensor, ema: Optional[torch.Tensor],
                         state: "StepState", grad_scale: float = 1.0, advance: bool = True) -> None:
    """rmsprop_ema_step with lr / EMA decay read from the device-resident schedule; advance: last optimiser launch of
    the step (state.step += 1 on the device)."""
    n = _opt_sizes("rmsprop_ema_step_dev", p, grad, sq, None, ema)
    _call("rmsprop_ema_step_dev", _ptr(p, "p"), _ptr(grad, "grad"), _ptr(sq, "sq"), _ptr(ema, "ema"), n, state.ptr,
          float(grad_scale), int(bool(advance)))


OPTIMIZER_KINDS = {"rmsprop": _lib.OPT_RMSPROP, "sgd": _lib.OPT_SGD, "adam": _lib.OPT_ADAM}


def opt_config(optimizer: str, lr: float, alpha: float = 0.99, eps: float = 1e-10, momentum: float = 0.0,
               betas: Tuple[float, float] = (0.9, 0.999), ema_decay: float = 0.0) -> _lib.OptConfig:
    """nsvd_opt_config of one of the reference's optimisers (examples/utils.py:48-72): "rmsprop" | "adam" | "sgd";
    eps is RMSprop's (1e-10 in the reference) or Adam's (--adam_eps)."""
    if optimizer not in OPTIMIZER_KINDS:
        raise NsvdError(f"unknown optimizer {optimizer!r}: one of {sorted(OPTIMIZER_KINDS)}")
    c = _lib.OptConfig()
    c.kind = OPTIMIZER_KINDS[optimizer]
    c.lr, c.alpha, c.eps, c.momentum = float(lr), float(alpha), float(eps), float(momentum)
    c.beta1, c.beta2 = float(betas[0]), float(betas[1])
    c.ema_decay = float(ema_decay)
    return c


def opt_uses(cfg: _lib.OptConfig) -> Tuple[bool, bool]:
    """(uses the sq slot, uses the mom slot) of cfg's rule"""
    if cfg.kind == _lib.OPT_ADAM:
        return True, True
    if cfg.kind == _lib.OPT_RMSPROP:
        return True, cfg.momentum != 0.0
    return False, cfg.momentum != 0.0


def _opt_sizes(what, p, grad, sq, mom, ema):
    n = p.numel()
    for t in (grad, sq, mom, ema):
        if t is not None and t.numel() != n:
            raise NsvdError(f"{what}: size mismatch")
    return n


@_on_tensor_device
def opt_step(cfg: _lib.OptConfig, p: torch.Tensor, grad: torch.Tensor, sq: Optional[torch.Tensor],
             mom: Optional[torch.Tensor], ema: Optional[torch.Tensor], steps_taken: int, lr: Optional[float] = None,
             ema_decay: Optional[float] = None, grad_scale: float = 1.0) -> None:
    """one step of cfg's rule + the EMA update over a flat tensor (nsvd_opt_step); lr / ema_decay: the step's scheduled
    values when they differ from cfg's; steps_taken: optimiser steps before this one"""
    n = _opt_sizes("opt_step", p, grad, sq, mom, ema)
    c = cfg
    if lr is not None or ema_decay is not None:
        c = _lib.OptConfig.from_buffer_copy(cfg)
        c.lr = cfg.lr if lr is None else float(lr)
        c.ema_decay = cfg.ema_decay if ema_decay is None else float(ema_decay)
    tb = torch_binding()
    if tb is not None:
        tb.opt_step(int(c.kind), p, grad, sq, mom, ema, c.lr, c.alpha, c.eps, c.momentum, c.beta1, c.beta2, c.ema_decay,
                    int(steps_taken), float(grad_scale))
        return
    _call("opt_step", _ptr(p, "p"), _ptr(grad, "grad"), _ptr(sq, "sq"), _ptr(mom, "mom"), _ptr(ema, "ema"), n,
          C.byref(c), int(steps_taken), float(grad_scale))


class OptState(_DeviceSchedule):
    """The device-resident schedule of any optimiser rule (include/nsvd.h: nsvd_opt_state): what StepState is for
    RMSprop without momentum, plus Adam's bias corrections and SGD's first-step flag."""
    _mirror, _entry = _lib.OptState, "opt_state"

    def __init__(self, device, cfg: _lib.OptConfig, T_max: int, eta_min: float = 0.0, step: int = 0):
        self.cfg, self.T_max, self.eta_min = cfg, int(T_max), float(eta_min)
        super().__init__(device, step)

    def _init_args(self, step: int) -> tuple:
        return C.byref(self.cfg), self.eta_min, self.T_max, step


@_on_tensor_device
def opt_step_dev(p: torch.Tensor, grad: torch.Tensor, sq: Optional[torch.Tensor], mom: Optional[torch.Tensor],
                 ema: Optional[torch.Tensor], state: OptState, grad_scale: float = 1.0, advance: bool = True) -> None:
    """opt_step with the step's scalars read from the device-resident schedule; advance: last optimiser launch of the
    step (state.step += 1 on the device)."""
    n = _opt_sizes("opt_step_dev", p, grad, sq, mom, ema)
    _call("opt_step_dev", _ptr(p, "p"), _ptr(grad, "grad"), _ptr(sq, "sq"), _ptr(mom, "mom"), _ptr(ema, "ema"), n,
          C.byref(state.cfg), state.ptr, float(grad_scale), int(bool(advance)))


@_on_tensor_device
def spectrum_accumulate(f: torch.Tensor, Tf: torch.Tensor, x: torch.Tensor, sigma: float, use_importance: bool,
                        lim: float, cov: torch.Tensor, quad: torch.Tensor, first_mode_const: bool = False) -> None:
    """cov += phi^T phi, quad += phi^T Tphi. float32 accumulators: the reference's (methods/spectrum.py:60-75);
    float64 accumulators (cov.dtype == torch.float64): products and sums in float64 (nsvd_spectrum_accumulate_f64).
    first_mode_const (float64 accumulators of shape (L + 1, L + 1)): a constant-one column in front of phi and Tphi
    (methods/spectrum.py:68-70)."""
    B, L = f.shape
    D = x.shape[1]
    if cov.dtype != quad.dtype or cov.dtype not in (torch.float32, torch.float64):
        raise NsvdError("spectrum_accumulate: cov / quad must both be float32 or both float64")
    Lp = L + int(bool(first_mode_const))
    if tuple(cov.shape) != (Lp, Lp) or tuple(quad.shape) != (Lp, Lp) or Tf.shape != f.shape:
        raise NsvdError(f"spectrum_accumulate: cov / quad must be ({Lp}, {Lp}), Tf like f")
    if first_mode_const and cov.dtype != torch.float64:
        raise NsvdError("spectrum_accumulate(first_mode_const=True) takes float64 accumulators")
    if cov.dtype == torch.float64:
        _call("spectrum_accumulate_const_f64" if first_mode_const else "spectrum_accumulate_f64", _ptr(f, "f"),
              _ptr(Tf, "Tf"), _ptr(x, "x"), B, L, D, float(sigma), int(bool(use_importance)), float(lim),
              _ptr(cov, "cov", torch.float64), _ptr(quad, "quad", torch.float64))
        return
    tb = torch_binding()
    if tb is not None:
        tb.spectrum_accumulate(f, Tf, x, float(sigma), bool(use_importance), float(lim), cov, quad)
        return
    _call("spectrum_accumulate", _ptr(f, "f"), _ptr(Tf, "Tf"), _ptr(x, "x"), B, L, D, float(sigma),
          int(bool(use_importance)), float(lim), _ptr(cov, "cov"), _ptr(quad, "quad"))


def _qnums_arg(qnums, width: int = 2):
    """(Lg, width) quantum numbers as the HOST int array the eigfunc entry points read during the call"""
    q = [tuple(int(v) for v in row) for row in qnums]
    if any(len(row) != width for row in q):
        raise NsvdError(f"quantum numbers: {width} per function")
    return (C.c_int * (width * len(q)))(*[v for row in q for v in row]), len(q)


def _eigfunc_eval(D, kind, param, qnums, x, out):
    name = "eigfunc_eval" if D == 2 else "eigfunc3_eval"
    arr, Lg = _qnums_arg(qnums, D)
    if x.dim() != 2 or x.shape[1] != D:
        raise NsvdError(f"{name}: x must be (B, {D})")
    if out is not None and tuple(out.shape) != (x.shape[0], Lg):
        raise NsvdError(f"{name}: out must be ({x.shape[0]}, {Lg})")
    psi = torch.empty((x.shape[0], Lg), dtype=torch.float64, device=x.device) if out is None else out
    _call(name, int(kind), float(param), arr, Lg, _ptr(x, "x"), x.shape[0], _ptr(psi, "psi", torch.float64))
    return psi


def _eigfunc_accumulate(D, kind, param, qnums, f, x, sigma, use_importance, lim, gram, cross, cov):
    name = "eigfunc_accumulate" if D == 2 else "eigfunc3_accumulate"
    arr, Lg = _qnums_arg(qnums, D)
    B, L = f.shape
    if x.dim() != 2 or tuple(x.shape) != (B, D):
        raise NsvdError(f"{name}: x must be (B, {D}) with f's B")
    if tuple(gram.shape) != (Lg, Lg) or tuple(cross.shape) != (Lg, L) or (cov is not None and tuple(cov.shape) != (L, L)):
        raise NsvdError(f"{name}: gram ({Lg}, {Lg}), cross ({Lg}, {L}), cov ({L}, {L}) or None")
    _call(name + "_f64", int(kind), float(param), arr, Lg, _ptr(f, "f"), L, _ptr(x, "x"), B, float(sigma),
          int(bool(use_importance)), float(lim), _ptr(gram, "gram", torch.float64), _ptr(cross, "cross", torch.float64),
          _ptr(cov, "cov", torch.float64))


@_on_tensor_device
def eigfunc_eval(kind: int, param: float, qnums, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """psi (B, Lg) float64: the analytic eigenfunctions `qnums` of ground truth `kind` (GT_*) at x (B, 2) float32
    (nsvd_eigfunc_eval)."""
    return _eigfunc_eval(2, kind, param, qnums, x, out)


@_on_tensor_device
def eigfunc_accumulate(kind: int, param: float, qnums, f: torch.Tensor, x: torch.Tensor, sigma: float,
                       use_importance: bool, lim: float, gram: torch.Tensor, cross: torch.Tensor,
                       cov: Optional[torch.Tensor] = None) -> None:
    """gram (Lg, Lg) += psi_w^T psi_w, cross (Lg, L) += psi_w^T phi, cov (L, L) += phi^T phi (or None), float64, with phi
    weighted as spectrum_accumulate weights it (nsvd_eigfunc_accumulate_f64)."""
    _eigfunc_accumulate(2, kind, param, qnums, f, x, sigma, use_importance, lim, gram, cross, cov)


@_on_tensor_device
def eigfunc3_eval(kind: int, param: float, qnums, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """psi (B, Lg) float64: the states `qnums` = (n, l, m) of GT_HYDROGEN3D with charge `param` at x (B, 3) float32
    (nsvd_eigfunc3_eval)."""
    return _eigfunc_eval(3, kind, param, qnums, x, out)


@_on_tensor_device
def eigfunc3_accumulate(kind: int, param: float, qnums, f: torch.Tensor, x: torch.Tensor, sigma: float,
                        use_importance: bool, lim: float, gram: torch.Tensor, cross: torch.Tensor,
                        cov: Optional[torch.Tensor] = None) -> None:
    """eigfunc_accumulate for x (B, 3): p_val = (2 lim)^-3, the Gaussian weight over three coordinates
    (nsvd_eigfunc3_accumulate_f64)."""
    _eigfunc_accumulate(3, kind, param, qnums, f, x, sigma, use_importance, lim, gram, cross, cov)


def profile_next_forward(ev_start: "torch.cuda.Event", ev_stop: "torch.cuda.Event") -> None:
    """Bracket the dominant kernel of the next operator_forward with two timing events (bench.py)."""
    for e in (ev_start, ev_stop):
        if e.cuda_event == 0:  # torch creates the hipEvent lazily, at the first record
            e.record()
    check(_lib.load().nsvd_profile_next_forward(ev_start.cuda_event, ev_stop.cuda_event), "nsvd_profile_next_forward")


def dominant_kernel_name(shape: ModelShape, B: int, path: int = PATH_AUTO) -> str:
    if path_name(shape, B, path).startswith("fused"):
        return "pmlp_fused_fwd_kernel"
    # generic path: the bracket spans the whole forward (features, every layer's contraction + activation pass, epilogue)
    return "generic forward [fourier_evenodd_kernel, gemm_generic3_kernel + softplus_inplace_kernel per layer, fd_epilogue_kernel]"


# ------------------------------------------------------------------------------ row normalisation (CDK towers)
@_on_tensor_device
def row_normalize(z: torch.Tensor, r_up: float, mode: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """normalize(z, r_up, 'l2_ball' | 'l2_sphere') of examples/models/siam.py:170-183 on (B, L) float32 rows."""
    if z.dim() != 2 or z.dtype != torch.float32 or not z.is_contiguous():
        raise NsvdError("row_normalize: z must be a contiguous (B, L) float32 tensor")
    if out is None:
        out = torch.empty_like(z)
    _call("row_normalize_forward", _ptr(z, "z"), z.shape[0], z.shape[1], float(r_up), int(mode), _ptr(out, "out"))
    return out


@_on_tensor_device
def row_normalize_backward(z: torch.Tensor, dout: torch.Tensor, r_up: float, mode: int) -> torch.Tensor:
    dz = torch.empty_like(z)
    _call("row_normalize_backward", _ptr(z, "z"), _ptr(dout, "dout"), z.shape[0], z.shape[1], float(r_up), int(mode),
          _ptr(dz, "dz"))
    return dz


# ------------------------------------------------------------------------------ CDK towers (Linear-BN-lrelu-Linear-BN)
TOWER_KEYS = ("W1", "b1", "g1", "be1", "rm1", "rv1", "W2", "b2", "g2", "be2", "rm2", "rv2")


def tower_supported(B: int, d0: int, d1: int, d2: int) -> bool:
    return int(_lib.load().nsvd_tower_workspace_bytes(int(B), int(d0), int(d1), int(d2))) > 0


def tower_mixed_supported(B: int, d0: int, d1: int, d2: int) -> bool:
    """does the mixed-precision mode (gemm_bf16) take this shape? (B, d1, d2 multiples of 256, d0 of 128, B <= 1024)"""
    return bool(_lib.load().nsvd_tower_mixed_supported(int(B), int(d0), int(d1), int(d2)))


def tower_mixed_fused(B: int, d0: int, d1: int, d2: int, slope: float) -> bool:
    """does the mixed-precision tower of this shape run the wide layer with BatchNorm inside the contraction
    (csrc/tower_col.h; include/nsvd.h: nsvd_tower_mixed_fused)? The oracle mode that restates its roundings:
    tower_forward_backward(gemm_bf16="fused") - otherwise gemm_bf16=True."""
    return bool(_lib.load().nsvd_tower_mixed_fused(int(B), int(d0), int(d1), int(d2), float(slope)))


def tower_workspace(B: int, d0: int, d1: int, d2: int, device) -> torch.Tensor:
    n = int(_lib.load().nsvd_tower_workspace_bytes(int(B), int(d0), int(d1), int(d2)))
    if n == 0:
        raise NsvdError(f"tower: unsupported shape B={B}, sizes {(d0, d1, d2)} (multiples of 128, B <= 1024)")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _tower_struct(t: dict, need_running: bool) -> "_lib.TowerParams":
    p = _lib.TowerParams()
    for k in TOWER_KEYS:
        v = t.get(k)
        if v is None:
            if k.startswith("r") and not need_running:
                continue
            raise NsvdError(f"tower: tensor {k} missing")
        setattr(p, k, _ptr(v, k))
    p._keepalive = dict(t)
    return p


def tower_y2(ws: torch.Tensor, B: int, d0: int, d1: int, d2: int) -> torch.Tensor:
    """the (B, d2) float32 view of a tower workspace where phase 1 leaves this rank's partial A1 W2^T (hidden width
    sharded over processes): all-reduce it in place between tower_forward(phase=1) and tower_forward(phase=2)"""
    off = int(_lib.load().nsvd_tower_y2_offset(int(B), int(d0), int(d1), int(d2)))
    return ws[off:off + 4 * B * d2].view(torch.float32).view(B, d2)


@_on_tensor_device
def tower_forward(x: torch.Tensor, params: dict, slope: float, eps: float, momentum: float, update_running: bool,
                  ws: torch.Tensor, gemm_bf16: bool = False, phase: int = 0) -> Optional[torch.Tensor]:
    """z = BN2(Linear2(lrelu(BN1(Linear1(x))))) in training mode; params: dict over TOWER_KEYS (torch layouts).
    gemm_bf16: mixed precision - bfloat16 operands and wide activations, float32 accumulation and statistics (nsvd.h;
    shapes: tower_mixed_supported). The value 3 (bit 1) says the bfloat16 weight copies inside ws are current.
    phase (hidden width sharded over processes, params = this rank's slices): 1 = up to the partial product in
    tower_y2(ws, ...) (returns None), 2 = bias + second BatchNorm from the all-reduced tower_y2; 0 = the whole tower."""
    B, d0 = x.shape
    d1, d2 = params["W1"].shape[0], params["W2"].shape[0]
    if tuple(params["W1"].shape) != (d1, d0) or tuple(params["W2"].shape) != (d2, d1):
        raise NsvdError("tower_forward: W1 must be (d1, d0), W2 (d2, d1)")
    for k, n in (("b1", d1), ("g1", d1), ("be1", d1), ("b2", d2), ("g2", d2), ("be2", d2)):
        if params[k].numel() != n:
            raise NsvdError(f"tower_forward: {k} must have {n} elements")
    z = torch.empty((B, d2), dtype=torch.float32, device=x.device) if phase != 1 else None
    p = _tower_struct(params, bool(update_running))
    _call("tower_forward_phase", _ptr(x, "x"), C.byref(p), B, d0, d1, d2, float(slope), float(eps), float(momentum),
          int(bool(update_running)), int(gemm_bf16), int(phase), _ptr(z, "z"), *_ws(ws))
    return z


@_on_tensor_device
def tower_backward(x: torch.Tensor, params: dict, dz: torch.Tensor, slope: float, ws: torch.Tensor,
                   gemm_bf16: bool = False) -> dict:
    """gradients of sum(dz * z) w.r.t. W1, b1, g1, be1, W2, b2, g2, be2 (same workspace as the forward call)."""
    B, d0 = x.shape
    d1, d2 = params["W1"].shape[0], params["W2"].shape[0]
    if tuple(dz.shape) != (B, d2):
        raise NsvdError("tower_backward: dz must be (B, d2)")
    grads = {k: torch.empty_like(params[k]) for k in TOWER_KEYS if not k.startswith("r")}
    p, g = _tower_struct(params, False), _tower_struct(grads, False)
    _call("tower_backward", _ptr(x, "x"), C.byref(p), _ptr(dz, "dz"), B, d0, d1, d2, float(slope), int(gemm_bf16),
          C.byref(g), *_ws(ws))
    return grads


@_on_tensor_device
def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """bfloat16(x), round to nearest even (nsvd_to_bf16) - the cast the mixed-precision towers' operands go through"""
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() % 8:
        raise NsvdError("to_bf16: contiguous float32 tensor with a multiple of 8 elements")
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _call("to_bf16", _ptr(x, "x"), out.data_ptr(), x.numel())
    return out


@_on_tensor_device
def gemm_bf16(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor] = None, a_kstrided: bool = False,
              b_kstrided: bool = False, out_bf16: bool = False, slices: int = 1, want_sumsq: bool = False):
    """C = A B^T on the bf16 MFMA with float32 accumulation (nsvd_gemm_bf16). A, B: bfloat16, 2-D, contiguous.
    a_kstrided: A is (K, M) - the contraction index first (A^T as stored), else (M, K); likewise B with N.
    slices > 1: C has a leading slice dimension (split-K partial products). Returns C, or (C, sumsq per tile)."""
    for t, n in ((A, "A"), (B, "B")):
        if t.dtype != torch.bfloat16 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda:
            raise NsvdError(f"gemm_bf16: {n} must be a contiguous 2-D bfloat16 GPU tensor")
    K, M = (A.shape if a_kstrided else A.shape[::-1])
    Kb, N = (B.shape if b_kstrided else B.shape[::-1])
    if K != Kb:
        raise NsvdError("gemm_bf16: contraction lengths differ")
    shape = (M, N) if slices == 1 else (slices, M, N)
    Cm = torch.empty(shape, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=A.device)
    ss = torch.zeros((M // 256) * (N // 128) * slices, dtype=torch.float32, device=A.device) if want_sumsq else None
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N or not bias.is_cuda):
        raise NsvdError("gemm_bf16: bias must be N float32 values on the GPU")
    _call("gemm_bf16", A.data_ptr(), B.data_ptr(), Cm.data_ptr(), bias.data_ptr() if bias is not None else None, M, N, K,
          A.shape[1], B.shape[1], N, int(bool(a_kstrided)), int(bool(b_kstrided)), int(bool(out_bf16)), int(slices),
          M * N, ss.data_ptr() if ss is not None else None)
    return (Cm, ss) if want_sumsq else Cm


TOWER16_F16 = 16  # gemm_bf16 bit 4: the half type of the mixed-precision towers is IEEE float16 (include/nsvd.h)


class GradScaler:
    """torch.cuda.amp.GradScaler's state on the DEVICE (include/nsvd.h: nsvd_grad_scaler; the reference's AMP branch,
    examples/cdk/sketchy/main_sketchy.py:161,194-208): nsvd_cdk_step scales the loss gradient, skips the optimiser step
    on inf / NaN gradients and grows / backs off the scale without any host round trip. ``state()`` copies it back."""

    def __init__(self, device, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        self.buf = torch.zeros(C.sizeof(_lib.GradScalerState) // 4, dtype=torch.int32, device=device)
        with torch.cuda.device(self.buf.device):
            _call("grad_scaler_init", self.buf.data_ptr(), float(init_scale), float(growth_factor),
                  float(backoff_factor), int(growth_interval))

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr()

    def state(self) -> dict:
        """(synchronises) scale, growth_tracker, steps_ok (optimiser steps taken), steps_skipped, ..."""
        raw = self.buf.cpu().numpy().tobytes()
        st = _lib.GradScalerState.from_buffer_copy(raw)
        return {n: getattr(st, n) for n, _ in _lib.GradScalerState._fields_}


def cdk_step_desc(B: int, d0: int, d1: int, d2: int, slope: float, bn_eps: float, bn_momentum: float, mu: float,
                  normalize_mode: int, set_first_mode_const: bool, lr: float, momentum: float, max_grad_norm: float,
                  first_step: bool, gemm_bf16: int = 0, grad_scaler: Optional["GradScaler"] = None) -> "_lib.CdkStepDesc":
    d = _lib.CdkStepDesc()
    d.B, d.d0, d.d1, d.d2 = int(B), int(d0), int(d1), int(d2)
    d.slope, d.bn_eps, d.bn_momentum, d.mu = float(slope), float(bn_eps), float(bn_momentum), float(mu)
    d.normalize_mode, d.set_first_mode_const = int(normalize_mode), int(bool(set_first_mode_const))
    d.lr, d.momentum, d.max_grad_norm = float(lr), float(momentum), float(max_grad_norm or 0.0)
    d.first_step = int(bool(first_step))
    d.gemm_bf16 = int(gemm_bf16)
    d.grad_scaler = grad_scaler.ptr if grad_scaler is not None else None
    return d


def cdk_step_workspace(desc: "_lib.CdkStepDesc", device) -> torch.Tensor:
    n = int(_lib.load().nsvd_cdk_step_workspace_bytes(C.byref(desc)))
    if n == 0:
        raise NsvdError("cdk_step: unsupported description (tower shapes must be multiples of 128, batch <= 1024; "
                        "l2_ball / l2_sphere normalisation; mu > 0)")
    return torch.empty(n, dtype=torch.uint8, device=device)


@_on_tensor_device
def cdk_step(desc: "_lib.CdkStepDesc", x: torch.Tensor, y: torch.Tensor, towers: Sequence[dict],
             momentum_bufs: Sequence[dict], v: torch.Tensor, M: torch.Tensor, loss: torch.Tensor, ws: torch.Tensor,
             rs_joint: Optional[torch.Tensor] = None, rs_indep: Optional[torch.Tensor] = None) -> None:
    """one CDK training step (nsvd_cdk_step): towers / momentum_bufs are two dicts each over TOWER_KEYS (the momentum
    dicts without the running statistics), updated in place; loss: (4) = loss, operator term, metric term, grad norm"""
    if tuple(x.shape) != (desc.B, desc.d0) or tuple(y.shape) != (desc.B, desc.d0) or loss.numel() < 4:
        raise NsvdError("cdk_step: x, y must be (B, d0) and loss hold 4 floats")
    Lp = desc.d2 + desc.set_first_mode_const
    if v.numel() != Lp or tuple(M.shape) != (Lp, Lp):
        raise NsvdError(f"cdk_step: v ({Lp}), M ({Lp}, {Lp})")
    tw = (_lib.TowerParams * 2)(_tower_struct(towers[0], True), _tower_struct(towers[1], True))
    mb = (_lib.TowerParams * 2)(_tower_struct(momentum_bufs[0], False), _tower_struct(momentum_bufs[1], False))
    _call("cdk_step", C.byref(desc), _ptr(x, "x"), _ptr(y, "y"), tw, mb, _ptr(v, "v"), _ptr(M, "M"), _ptr(loss, "loss"),
          _ptr(rs_joint, "rs_joint"), _ptr(rs_indep, "rs_indep"), *_ws(ws))


# ------------------------------------------------------------------------------------- NeuralEF (include/nsvd.h)
@_on_tensor_device
def nef_operator_forward(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, ws: torch.Tensor,
                         norm_biased: torch.Tensor, norm_unbiased: torch.Tensor, initialized: torch.Tensor,
                         momentum: float, path: int = PATH_AUTO):
    """Training-mode Tphi, phi = operator(BatchL2NormalizedFunctions(model), x, importance); updates the running norms
    (1 + 2D times) and sets `initialized`. Returns (phi, Tphi, saved) - saved = (h, r, stats) for nef_operator_backward."""
    B = x.shape[0]
    if x.dim() != 2 or x.shape[1] != shape.D:
        raise NsvdError(f"x must be (B, {shape.D})")
    if norm_biased.numel() != shape.L or norm_unbiased.numel() != shape.L:
        raise NsvdError(f"running norms must hold {shape.L} values")
    dev = x.device
    phi = torch.empty((B, shape.L), dtype=torch.float32, device=dev)
    Tphi, h, r = torch.empty_like(phi), torch.empty_like(phi), torch.empty_like(phi)
    stats = torch.empty((1 + 2 * shape.D, shape.L), dtype=torch.float32, device=dev)
    _call("nef_operator_forward", _desc(shape), C.byref(params), C.byref(prob), _ptr(x, "x"), B, _ptr(phi), _ptr(Tphi),
          _ptr(h), _ptr(r), _ptr(stats), _ptr(norm_biased, "norm_biased"), _ptr(norm_unbiased, "norm_unbiased"),
          _ptr(initialized, "initialized", torch.int32), float(momentum), *_ws(ws), int(path))
    return phi, Tphi, (h, r, stats)


@_on_tensor_device
def nef_operator_backward(shape: ModelShape, params: Params, prob: Problem, x: torch.Tensor, dphi: torch.Tensor,
                          saved, grads: Params, ws: torch.Tensor, path: int = PATH_AUTO) -> None:
    h, r, stats = saved
    B = x.shape[0]
    if tuple(dphi.shape) != (B, shape.L):
        raise NsvdError(f"dphi must be {(B, shape.L)}")
    du0 = torch.empty_like(h)
    _call("nef_operator_backward", _desc(shape), C.byref(params), C.byref(prob), _ptr(x, "x"), B, _ptr(dphi, "dphi"),
          _ptr(h), _ptr(r), _ptr(stats), _ptr(du0), C.byref(grads), *_ws(ws), int(path))


@_on_tensor_device
def nef_loss(phi: torch.Tensor, Tphi: torch.Tensor, phi1: torch.Tensor, Tphi1: torch.Tensor, phi2: torch.Tensor,
             Tphi2: torch.Tensor, unbiased: bool, diagonal: int, out=None, scratch: Optional[torch.Tensor] = None):
    """NeuralEigenfunctionsLossFunction on the HIP kernels. Returns (loss (1,), dphi, dphi1, dphi2): with phi1 / phi2
    the two chunks of phi, dphi holds the whole d loss / d phi and dphi1 = dphi2 = None. out: that tuple as buffers to
    write (a step that allocates nothing), scratch: nef_loss_scratch of the shape."""
    B, L = phi.shape
    B1, B2 = phi1.shape[0], phi2.shape[0]
    for n, t, rows in (("Tphi", Tphi, B), ("phi1", phi1, B1), ("Tphi1", Tphi1, B1), ("phi2", phi2, B2),
                       ("Tphi2", Tphi2, B2)):
        if t.dim() != 2 or tuple(t.shape) != (rows, L):
            raise NsvdError(f"{n} must be {(rows, L)} (got {tuple(t.shape)})")
    dev = phi.device
    chunked = (phi1.data_ptr() == phi.data_ptr() and Tphi1.data_ptr() == Tphi.data_ptr() and B1 + B2 == B and
               phi2.data_ptr() == phi.data_ptr() + 4 * B1 * L and Tphi2.data_ptr() == Tphi.data_ptr() + 4 * B1 * L)
    nbytes = _lib.load().nsvd_nef_loss_workspace_bytes(B, B1, B2, L)
    if nbytes == 0:
        raise NsvdError(f"nsvd_nef_loss: unsupported shape B={B}, B1={B1}, B2={B2}, L={L} (L <= 64)")
    if scratch is None:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif scratch.numel() < nbytes:
        raise NsvdError("nsvd_nef_loss: scratch is too small for this shape")
    if out is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dphi = torch.empty_like(phi)
        d1 = None if chunked else torch.empty_like(phi1)
        d2 = None if chunked else torch.empty_like(phi2)
    else:
        loss, dphi, d1, d2 = out
        if tuple(dphi.shape) != (B, L) or (not chunked and (d1 is None or d2 is None or
                                                          tuple(d1.shape) != (B1, L) or tuple(d2.shape) != (B2, L))):
            raise NsvdError("nsvd_nef_loss: out must be (loss (1,), dphi (B, L), dphi1 (B1, L), dphi2 (B2, L))")
        if chunked:
            d1 = d2 = None
    _call("nef_loss", _ptr(phi, "phi"), _ptr(Tphi, "Tphi"), B, _ptr(phi1, "phi1"), _ptr(Tphi1, "Tphi1"), B1,
          _ptr(phi2, "phi2"), _ptr(Tphi2, "Tphi2"), B2, L, int(bool(unbiased)), int(diagonal), _ptr(loss), _ptr(dphi),
          _ptr(d1), _ptr(d2), _ws(scratch, "scratch")[0], nbytes)
    return loss, dphi, d1, d2


def nef_loss_scratch(B: int, B1: int, B2: int, L: int, device) -> torch.Tensor:
    nbytes = _lib.load().nsvd_nef_loss_workspace_bytes(int(B), int(B1), int(B2), int(L))
    if nbytes == 0:
        raise NsvdError(f"nsvd_nef_loss: unsupported shape B={B}, B1={B1}, B2={B2}, L={L} (L <= 64)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


NEF_MAX_L = 64  # heads nsvd_nef_loss and nsvd_nef_rows_* take


def nef_rows_workspace(B: int, L: int, device) -> torch.Tensor:
    """the workspace of nef_rows_forward / nef_rows_backward on a (B, L) block (either segmentation)"""
    nbytes = _lib.load().nsvd_nef_rows_workspace_bytes(int(B), int(L))
    if nbytes == 0:
        raise NsvdError(f"nsvd_nef_rows: unsupported shape B={B}, L={L} (1 <= L <= {NEF_MAX_L}, B <= 65536)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _nef_rows_shape(u: torch.Tensor, B1: Optional[int], name: str):
    if u.dim() != 2:
        raise NsvdError(f"{name} must be (B, L)")
    B, L = u.shape
    B1 = B if B1 is None else int(B1)
    if not 1 <= B1 <= B:
        raise NsvdError(f"nsvd_nef_rows: the first segment must hold 1..{B} rows (got {B1})")
    return B, B1, L


@_on_tensor_device
def nef_rows_forward(u: torch.Tensor, B1: Optional[int], norm_biased: Optional[torch.Tensor],
                     norm_unbiased: Optional[torch.Tensor], initialized: Optional[torch.Tensor], momentum: float,
                     order=(0,), ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     stats: Optional[torch.Tensor] = None):
    """BatchL2NormalizedFunctions.forward in training mode on the raw head outputs u (B, L) (nsvd_nef_rows_forward):
    the rows are one segment (B1 None or B) or the two segments [0, B1), [B1, B). Returns (phi = u / n_h by segment,
    stats (2, L) = the batch norms n_1 | n_2); the running norms (L values each) take one update per entry of `order`
    (segment indices, at most four; none: the three state tensors may be None) and `initialized` (int32, 1 value) is
    set. out may be u."""
    B, B1, L = _nef_rows_shape(u, B1, "u")
    order = tuple(int(o) for o in order)
    if len(order) > 4 or any(o not in ((0, 1) if B1 < B else (0,)) for o in order):
        raise NsvdError("nsvd_nef_rows_forward: order holds at most four indices of existing segments")
    if order and (norm_biased is None or norm_unbiased is None or initialized is None):
        raise NsvdError("nsvd_nef_rows_forward: running-norm updates need norm_biased, norm_unbiased and initialized")
    for n, t in (("norm_biased", norm_biased), ("norm_unbiased", norm_unbiased)):
        if t is not None and t.numel() != L:
            raise NsvdError(f"{n} must hold {L} values")
    if out is None:
        out = torch.empty_like(u)
    elif tuple(out.shape) != (B, L):
        raise NsvdError("nsvd_nef_rows_forward: out must be (B, L)")
    if stats is None:
        stats = torch.empty((2, L), dtype=torch.float32, device=u.device)
    elif stats.numel() != 2 * L:
        raise NsvdError("nsvd_nef_rows_forward: stats must hold 2 L values")
    if ws is None:
        ws = nef_rows_workspace(B, L, u.device)
    _call("nef_rows_forward", _ptr(u, "u"), B, B1, L, _ptr(out, "out"), _ptr(stats, "stats"),
          _ptr(norm_biased, "norm_biased"), _ptr(norm_unbiased, "norm_unbiased"),
          _ptr(initialized, "initialized", torch.int32), float(momentum),
          (C.c_int * 4)(*(order + (0,) * (4 - len(order)))), len(order), *_ws(ws))
    return out, stats


@_on_tensor_device
def nef_rows_backward(phi: Optional[torch.Tensor], stats: Optional[torch.Tensor], B1: Optional[int],
                      dphi: torch.Tensor, dphi1: Optional[torch.Tensor] = None, dphi2: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the cotangent of u (nsvd_nef_rows_backward): g = dphi (+ dphi1 + dphi2, each (B, L)), du = (g - phi s_h) / n_h
    with s_h the segment's column means of g phi; stats None (batchnorm_mode 'none'): du = g. out may be dphi."""
    B, B1, L = _nef_rows_shape(dphi, B1, "dphi")
    if (dphi1 is None) != (dphi2 is None):
        raise NsvdError("nsvd_nef_rows_backward: dphi1 and dphi2 come together")
    for n, t in (("phi", phi), ("dphi1", dphi1), ("dphi2", dphi2), ("out", out)):
        if t is not None and tuple(t.shape) != (B, L):
            raise NsvdError(f"nsvd_nef_rows_backward: {n} must be {(B, L)}")
    if stats is not None and (phi is None or stats.numel() != 2 * L):
        raise NsvdError("nsvd_nef_rows_backward: stats (2 L values) comes with phi")
    if out is None:
        out = torch.empty_like(dphi)
    if ws is None:
        ws = nef_rows_workspace(B, L, dphi.device)
    _call("nef_rows_backward", _ptr(phi, "phi"), _ptr(stats, "stats"), B, B1, L, _ptr(dphi, "dphi"),
          _ptr(dphi1, "dphi1"), _ptr(dphi2, "dphi2"), _ptr(out, "out"), *_ws(ws))
    return out


@_on_tensor_device
def nef_scale_heads(f: torch.Tensor, Tf: torch.Tensor, norm: torch.Tensor) -> None:
    """f /= norm, Tf /= norm per head, in place (BatchL2NormalizedFunctions in evaluation mode)."""
    B, L = f.shape
    _call("nef_scale_heads", _ptr(f, "f"), _ptr(Tf, "Tf"), _ptr(norm.reshape(-1), "norm"), B, L)


# ------------------------------------------------------------------------ retrieval metrics (include/nsvd.h)
RETR_INNER_PRODUCT, RETR_EUCLIDEAN = 0, 1


def retrieval_max_gallery() -> int:
    """the largest gallery nsvd_retrieval_eval ranks (host-side query, no GPU needed)"""
    return int(_lib.load().nsvd_retrieval_max_gallery())


def retrieval_max_k() -> int:
    """the largest K nsvd_retrieval_eval returns top-K lists for (host-side query)"""
    return int(_lib.load().nsvd_retrieval_max_k())


def retrieval_max_d() -> int:
    """the widest embedding nsvd_retrieval_eval takes (host-side query)"""
    return int(_lib.load().nsvd_retrieval_max_d())


def retrieval_workspace_bytes(Nq: int, Ng: int, d: int, K: int) -> int:
    """bytes of workspace for one nsvd_retrieval_eval call (host-side query); raises for an invalid description"""
    n = _lib.load().nsvd_retrieval_workspace_bytes(int(Nq), int(Ng), int(d), int(K))
    if n == 0:
        raise NsvdError(f"retrieval: invalid or unsupported description Nq={Nq}, Ng={Ng}, d={d}, K={K} (d <= "
                        f"{retrieval_max_d()}, 1 <= K <= min(Ng, {retrieval_max_k()}), Ng <= {retrieval_max_gallery()})")
    return int(n)


def _retr_matrix(z: torch.Tensor, name: str):
    if not isinstance(z, torch.Tensor) or not z.is_cuda:
        raise NsvdError(f"{name} must live on the GPU (got {getattr(z, 'device', type(z))}); neural_svd_amd has no CPU path")
    if z.dtype != torch.float32:
        raise NsvdError(f"{name} must be float32 (got {z.dtype})")
    if z.dim() != 2 or z.shape[1] < 1:
        raise NsvdError(f"{name} must be a (rows, d) matrix with d >= 1")
    if z.stride(1) != 1 or (z.shape[0] > 1 and z.stride(0) < z.shape[1]):
        raise NsvdError(f"{name}: unit column stride and a row stride >= d (a column window of a contiguous matrix)")
    return z.data_ptr(), (int(z.stride(0)) if z.shape[0] > 1 else int(z.shape[1]))


@_on_tensor_device
def retrieval_eval(zq: torch.Tensor, zg: torch.Tensor, q_cls: torch.Tensor, g_cls: torch.Tensor,
                   n_relevant_items: Optional[torch.Tensor] = None, metric: int = RETR_INNER_PRODUCT, K: int = 100,
                   want_topk: bool = True, want_ap: bool = True, ws: Optional[torch.Tensor] = None):
    """nsvd_retrieval_eval: every query's whole-gallery ranking (descending key, ties by ascending gallery index).
    zq (Nq, d), zg (Ng, d): float32 with unit column stride (column windows of a wider matrix are taken as they are);
    q_cls (Nq), g_cls (Ng), n_relevant_items (Nq): int32. Returns a dict: prec_at_k (Nq), hits_at_k (Nq) int32 (the count behind it), n_relevant_found (Nq) and,
    when asked for, topk_idx (Nq, K) int32, topk_rel (Nq, K) bool, avg_prec (3, Nq) float64 = ap_ver 1, 2, 3."""
    pq, ldq = _retr_matrix(zq, "zq")
    pg, ldg = _retr_matrix(zg, "zg")
    Nq, d = zq.shape
    Ng = zg.shape[0]
    if zg.shape[1] != d:
        raise NsvdError(f"zq and zg must share the embedding width (got {d} and {zg.shape[1]})")
    if metric not in (RETR_INNER_PRODUCT, RETR_EUCLIDEAN):
        raise NsvdError(f"retrieval_eval: unknown metric {metric}")
    if q_cls.numel() != Nq or g_cls.numel() != Ng:
        raise NsvdError("retrieval_eval: q_cls / g_cls must hold one class id per row")
    if want_ap and (n_relevant_items is None or n_relevant_items.numel() != Nq):
        raise NsvdError("retrieval_eval: the average precisions need n_relevant_items (Nq)")
    lib = _lib.load()
    K = int(K)
    nbytes = lib.nsvd_retrieval_workspace_bytes(Nq, Ng, d, K)
    if nbytes == 0:
        if 1 <= K <= min(Ng, retrieval_max_k()) and 1 <= d <= retrieval_max_d() and Ng > lib.nsvd_retrieval_max_gallery():
            check(_lib.EUNSUPPORTED, f"nsvd_retrieval_eval (Ng = {Ng} > {lib.nsvd_retrieval_max_gallery()})")
        check(_lib.EINVAL, f"nsvd_retrieval_eval (Nq={Nq}, Ng={Ng}, d={d}, K={K})")
    dev = zq.device
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif ws.numel() * ws.element_size() < nbytes:
        raise NsvdError(f"retrieval_eval: workspace of {ws.numel() * ws.element_size()} bytes, {nbytes} needed")
    out = {"prec_at_k": torch.empty(Nq, dtype=torch.float32, device=dev),
           "hits_at_k": torch.empty(Nq, dtype=torch.int32, device=dev),
           "n_relevant_found": torch.empty(Nq, dtype=torch.int32, device=dev)}
    if want_topk:
        out["topk_idx"] = torch.empty((Nq, K), dtype=torch.int32, device=dev)
        out["topk_rel"] = torch.empty((Nq, K), dtype=torch.uint8, device=dev)
    if want_ap:
        out["avg_prec"] = torch.empty((3, Nq), dtype=torch.float64, device=dev)
    _call("retrieval_eval", pq, ldq, pg, ldg, Nq, Ng, d, _ptr(q_cls, "q_cls", torch.int32),
          _ptr(g_cls, "g_cls", torch.int32),
          _ptr(n_relevant_items if want_ap else None, "n_relevant_items", torch.int32), int(metric), K,
          _ptr(out.get("topk_idx"), "topk_idx", torch.int32), _ptr(out.get("topk_rel"), "topk_rel", torch.uint8),
          _ptr(out["prec_at_k"]), _ptr(out["hits_at_k"], "hits_at_k", torch.int32),
          _ptr(out.get("avg_prec"), "avg_prec", torch.float64), _ptr(out["n_relevant_found"], "n", torch.int32), *_ws(ws))
    if want_topk:
        out["topk_rel"] = out["topk_rel"].view(torch.bool)
    return out
