"""CPU checks of the dense two-sided product (nsvd_kernel_apply_pair, hip_ops.kernel_apply_pair,
kernel_ops.DenseCrossOperator, kernel_svd.DenseSvdTrainer): the symbols and exports, the workspace and partition queries,
the refusals that come before any launch, and the float64 restatement (tests/_dense_pair_oracle.py) against a triple loop.
Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _dense_pair_oracle as DP
from tests import _pair_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nsvd_kernel_apply_pair_workspace_bytes", "nsvd_kernel_apply_pair_partition", "nsvd_kernel_apply_pair")


def _declared_arg_counts():
    """name -> number of parameters of its declaration in include/nsvd_dense.h"""
    src = open(os.path.join(ROOT, "include", "nsvd_dense.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: len(params.split(",")) for name, params in re.findall(r"\b(nsvd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}


def test_new_symbols_in_header_signatures_and_exports():
    """the dense pair's entry points live in a library of their own (libnsvd_dense.so, include/nsvd_dense.h,
    _lib.DENSE_SIGNATURES), held to what tests/test_abi.py holds libnsvd_hip.so to: header == ctypes table == exported
    symbols, argument counts included; libnsvd_hip.so and its table stay the entry points of ABI 6"""
    import subprocess
    import neural_svd_amd
    from neural_svd_amd import _lib, kernel_ops, kernel_svd
    from neural_svd_amd import hip_ops as H
    if not os.path.exists(_lib.DENSE_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    counts = _declared_arg_counts()
    assert sorted(counts) == sorted(NEW) == sorted(_lib.DENSE_SIGNATURES)
    assert {n: len(a) for n, (_, a) in _lib.DENSE_SIGNATURES.items()} == counts
    objdump = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
    out = subprocess.check_output([objdump, "-T", _lib.DENSE_LIB_PATH], text=True)
    exported = sorted({ln.split()[-1] for ln in out.splitlines()
                       if ln.split() and ln.split()[-1].startswith("nsvd_") and "*UND*" not in ln})
    assert exported == sorted(NEW)
    lib = _lib.load_dense()
    for name in NEW:
        assert hasattr(lib, name) and name not in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 6 and _lib.load().nsvd_abi_version() == 6  # new symbols only
    assert len(_lib.DENSE_SIGNATURES["nsvd_kernel_apply_pair"][1]) == 18
    for name in ("kernel_apply_pair", "kernel_apply_pair_workspace", "kernel_apply_pair_partition"):
        assert callable(getattr(H, name)), name
    assert hasattr(H.kernel_apply_pair, "__wrapped__")  # the device guard
    assert neural_svd_amd.DenseCrossOperator is kernel_ops.DenseCrossOperator
    assert neural_svd_amd.DenseSvdTrainer is kernel_svd.DenseSvdTrainer
    assert {"DenseCrossOperator", "DenseSvdTrainer"} <= set(neural_svd_amd.__all__)
    assert not issubclass(kernel_svd.DenseSvdTrainer, kernel_svd.KernelSvdTrainer)  # a sibling, not a subclass


def _bytes(N2, B1, L):
    """the layout of csrc/kernel_apply_pair.hip: Sg^T, f^T, the CG copies of A g, the RG copies of A[rows, :]^T f"""
    def up(n, m):
        return (n + m - 1) // m * m
    B1p, N2p, Lp = up(B1, 64), up(N2, 64), up(L, 64)
    rg, cg = P.pair_split(B1, N2, L)  # (the same rule, with the padded columns of A in the place of the y rows)
    return sum(up(4 * n, 256) for n in (Lp * N2p, Lp * B1p, cg * B1p * Lp, rg * N2p * Lp)), rg, cg


def test_workspace_and_partition_queries():
    from neural_svd_amd import _lib
    lib = _lib.load_dense()
    q, part = lib.nsvd_kernel_apply_pair_workspace_bytes, lib.nsvd_kernel_apply_pair_partition
    rg, cg = ctypes.c_int(-5), ctypes.c_int(-5)
    for k in range(5):
        for v in (0, -3):
            bad = [16, 16, 8, 8, 2]
            bad[k] = v
            assert q(*bad) == 0, bad
            assert part(*bad, ctypes.byref(rg), ctypes.byref(cg)) == _lib.EINVAL and (rg.value, cg.value) == (-5, -5)
    assert part(16, 16, 8, 8, 2, None, ctypes.byref(cg)) == _lib.EINVAL
    assert part(16, 16, 8, 8, 2, ctypes.byref(rg), None) == _lib.EINVAL
    for N1, N2, B1, B2, L in ((1, 1, 1, 1, 1), (130, 67, 5, 400, 1), (300, 1000, 193, 70, 33),
                              (2048, 2304, 512, 512, 64), (300, 130, 1024, 1024, 70), (10000, 10000, 8192, 8192, 64),
                              (20000, 5000, 8192, 8192, 64)):
        want, wr, wc = _bytes(N2, B1, L)
        assert q(N1, N2, B1, B2, L) == want and want > 0 and want % 256 == 0, (N1, N2, B1, B2, L)
        assert part(N1, N2, B1, B2, L, ctypes.byref(rg), ctypes.byref(cg)) == 0
        assert (rg.value, cg.value) == (wr, wc) and 1 <= wr <= 32 and 1 <= wc <= 32
    assert min(_bytes(2304, 512, 64)[1:]) > 1  # the GPU suite's several-groups case


def test_workspace_is_monotone_in_each_argument():
    from neural_svd_amd import _lib
    q = _lib.load_dense().nsvd_kernel_apply_pair_workspace_bytes
    sizes = (1, 63, 64, 65, 130, 257, 1030, 4096, 8192, 8193, 16384, 40000)
    base = dict(N1=1000, N2=1000, B1=256, B2=256, L=16)
    for fixed in (dict(), dict(N2=8192, B1=8192, L=64), dict(N2=1, B1=1, L=1)):
        for name in ("N1", "N2", "B1", "B2"):
            vals = []
            for s in sizes:
                a = dict(base, **fixed)
                a[name] = s
                vals.append(q(a["N1"], a["N2"], a["B1"], a["B2"], a["L"]))
            assert all(v > 0 for v in vals) and vals == sorted(vals), (name, fixed, vals)
        vals = [q(1000, 1000, 256, 256, L) for L in (1, 5, 63, 64, 65, 128, 130, 200)]
        assert all(v > 0 for v in vals) and vals == sorted(vals)


def test_c_refusals_need_no_device():
    """null pointers, non-positive sizes, a bad lda or alignment and a bad workspace are NSVD_EINVAL before any HIP call:
    the addresses are made up and nothing is launched"""
    from neural_svd_amd import _lib
    lib = _lib.load_dense()
    fn = lib.nsvd_kernel_apply_pair
    N1, N2, B1, B2, L = 100, 70, 32, 48, 3
    need = lib.nsvd_kernel_apply_pair_workspace_bytes(N1, N2, B1, B2, L)
    good = dict(A=0x10000, lda=128, N1=N1, N2=N2, rows=0x20000, B1=B1, cols=0x30000, B2=B2, g=0x40000, f=0x50000, L=L,
                sg=1.0, sf=1.0, ox=0x60000, oy=0x70000, ws=0x80000, wsb=need, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return fn(*[a[k] for k in good])
    for name in ("A", "rows", "cols", "g", "f", "ox", "oy", "ws"):
        assert call(**{name: None}) == _lib.EINVAL, name
    for name in ("N1", "N2", "B1", "B2", "L"):
        assert call(**{name: 0}) == _lib.EINVAL and call(**{name: -1}) == _lib.EINVAL, name
    assert call(lda=70) == _lib.EINVAL      # below N2 rounded up to 64 (and not a multiple of 4)
    assert call(lda=124) == _lib.EINVAL     # a multiple of 4 below 128
    assert call(lda=130) == _lib.EINVAL     # covers the padded width, not a multiple of 4
    assert call(A=0x10004) == _lib.EINVAL   # A not 16-byte aligned
    assert call(ws=0x80080) == _lib.EINVAL  # workspace not 256-byte aligned
    assert call(wsb=need - 1) == _lib.EINVAL


def test_python_refusals_without_a_gpu():
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    from neural_svd_amd.kernel_ops import DenseCrossOperator
    A = torch.zeros(10, 64)
    rows, cols = torch.zeros(8, dtype=torch.int64), torch.zeros(9, dtype=torch.int64)
    g, f = torch.zeros(9, 3), torch.zeros(8, 3)
    with pytest.raises(NsvdError, match="GPU"):
        H.kernel_apply_pair(A, 10, 7, rows, cols, g, f, 1.0, 1.0)
    with pytest.raises(NsvdError, match="invalid|positive"):
        H.kernel_apply_pair_workspace(10, 7, 0, 9, 3, "cpu")
    with pytest.raises(NsvdError):
        H.kernel_apply_pair_partition(10, 0, 8, 9, 3)
    assert H.kernel_apply_pair_partition(2048, 2304, 512, 512, 64) == _bytes(2304, 512, 64)[1:]

    class SaysItIsOnTheGpu(torch.Tensor):  # the shape checks come before any address is taken
        is_cuda = True

    def gpu(t):
        return t.as_subclass(SaysItIsOnTheGpu)
    for bad in (dict(g=gpu(torch.zeros(8, 3))), dict(f=gpu(torch.zeros(8, 2))), dict(f=gpu(torch.zeros(9, 3))),
                dict(rows=gpu(rows.int())), dict(cols=gpu(cols[:, None])), dict(A=gpu(A.double())), dict(N2=65),
                dict(N1=11), dict(out_x=gpu(torch.zeros(9, 3))), dict(out_y=gpu(torch.zeros(8, 3)))):
        a = dict(A=gpu(A), N1=10, N2=7, rows=gpu(rows), cols=gpu(cols), g=gpu(g), f=gpu(f), scale_g=1.0, scale_f=1.0)
        a.update(bad)
        with pytest.raises(NsvdError):
            H.kernel_apply_pair.__wrapped__(**a)
    with pytest.raises(NsvdError, match="GPU"):
        DenseCrossOperator(torch.zeros(10, 7), torch.zeros(10, 2), torch.zeros(7, 3))
    for px, py in ((torch.zeros(9, 2), torch.zeros(7, 3)), (torch.zeros(10, 2), torch.zeros(8, 3)),
                   (torch.zeros(10), torch.zeros(7, 3))):
        with pytest.raises(ValueError):
            DenseCrossOperator(gpu(torch.zeros(10, 7)), px, py)
    with pytest.raises(ValueError):
        DenseCrossOperator(gpu(torch.zeros(10)), torch.zeros(10, 2), torch.zeros(7, 3))


def test_oracle_against_a_triple_loop():
    rng = np.random.default_rng(0)
    N1, N2, L = 7, 5, 3
    A = rng.standard_normal((N1 + 2, 64))  # two rows beyond N1 and the column padding: never read
    A[:, N2:] = 7.0
    A[N1:] = 7.0
    rows = np.array([3, 3, 0, -1, 6, 7, 2, 3, 12])       # duplicates; -1, 7, 12 are out of range
    cols = np.array([4, 0, 4, 5, -2, 1, 4])              # duplicates; 5, -2 are out of range
    g, f = rng.standard_normal((len(cols), L)), rng.standard_normal((len(rows), L))
    want_x, want_y = np.zeros((len(rows), L)), np.zeros((len(cols), L))
    for i, r in enumerate(rows):
        for k, c in enumerate(cols):
            if 0 <= r < N1 and 0 <= c < N2:
                for l in range(L):
                    want_x[i, l] += 0.5 * A[r, c] * g[k, l]
                    want_y[k, l] += 0.25 * A[r, c] * f[i, l]
    got_x, got_y = DP.dense_apply_pair(A, N1, N2, rows, cols, g, f, 0.5, 0.25)
    assert np.abs(got_x - want_x).max() < 1e-14 and np.abs(got_y - want_y).max() < 1e-14
    assert not got_x[[3, 5, 8]].any() and not got_y[[3, 4]].any() and got_x[0].any() and got_y[0].any()
    assert np.array_equal(got_x[0], got_x[1]) and np.array_equal(got_x[0], got_x[7])  # duplicates: equal rows
