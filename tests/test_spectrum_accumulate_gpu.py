"""spectrum.hip (nsvd_spectrum_accumulate, _f64, _const_f64) against the float64 restatement tests/_spectrum_oracle.py
(itself held to the reference's compute_spectrum_evd by tests/test_spectrum_oracle.py) at every shape where the kernel
takes another path. Which case reaches what - from the dispatch code (one workgroup per SR = 128 rows, LDS
2 * 128 * (L + pad) floats, SMAXL = 64), not from a run:

  (B, L, D, pad, Gaussian)
  (1, 1, 1, no, no)       one row, one output, use_importance = 0, D = 1
  (127, 3, 2, yes, yes)   one workgroup of fewer than 128 rows; the padded constant column; Gaussian weight
  (128, 16, 3, no, yes)   exactly one full workgroup; D = 3
  (129, 63, 5, yes, no)   a second workgroup of ONE row; L + pad = 64; use_importance = 0 with the pad; D = 5
  (300, 64, 12, no, yes)  L = SMAXL, 65,536 bytes of LDS (exactly 64 KiB); D = 12; three workgroups, the last of 44 rows
  (300, 64, 2, yes, yes)  L = SMAXL with the pad: 2 * 128 * 65 * 4 = 66,560 bytes of dynamic LDS, (65, 65) accumulators
  (257, 5, 12, yes, yes)  D = 12 with the pad, L*L < 256 (idle threads in the product loop), a last workgroup of one row

Every case with B >= 127 carries the four rows that decide the x ~ 0 rule (_spectrum_oracle.planted_rows). The
accumulators start non-zero and every case makes two calls: += and not overwrite.

Input condition, checked for every row: -0.5 |x / sigma|^2 + log_norm > -80. Below that the float32 exp of the weight
underflows - in the reference's float32 run too; sqrt(exp(a)) is the reference's formula and not in question here.

Measure: each entry's error over its Cauchy-Schwarz scale, sqrt(cov_ii cov_jj) for cov and sqrt(cov_ii tt_jj),
tt = Tphi^T Tphi, for quad; the maximum over entries. Bars: float64 accumulators 1e-6 (the bar of
test_spectrum_accumulators_float64), float32 accumulators 1e-5 on cov and 1e-4 on quad (the same test's). The 1e-6 rests
on a float32 weight: at D = 12 its exponent is about -50, which float32 carries to 2^-24 * 50 = 3e-6 absolute, 1.5e-6
relative on sqrt(exp(.)) for a single row. The yardstick y is therefore evaluated beside every float64 figure: the
same quantity with the weight formula alone in numpy float32 (everything else float64); the assertion is
got <= max(1e-6, 4 y), the 4 for expf's last bits against numpy's.

Measured on MI355X (got / y, float64 accumulators; worst pair first):
  (300, 64, 12, no pad)   cov 1.67e-6 / 1.68e-6   quad 7.31e-7 / 6.98e-7   - above 1e-6, and all of it the float32 weight
  (257, 5, 12, pad)       cov 1.32e-6 / 1.30e-6   quad 2.82e-7 / 2.92e-7
  (128, 16, 3, no pad)    cov 4.72e-7 / 4.21e-7   quad 1.32e-7 / 1.40e-7
  the other four cases: at most 2.80e-7 / 2.88e-7 on cov and 5.66e-8 / 5.47e-8 on quad; got follows y everywhere
  except (1, 1, 1) (cov 1.07e-7 / 2.98e-8: one product, its own float32 roundings)
  float32 accumulators: cov 1.91e-6 at worst (bar 1e-5), quad 7.27e-7 (bar 1e-4); non-finite inputs: 0 (exact)
The 66,560-byte launch of (300, 64, 2, pad) is granted as it is (no hipFuncSetAttribute call) and the case passes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _spectrum_oracle as SO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA, LIM = 16.0, 50.0
H = None

CASES = [(1, 1, 1, 0, 0), (127, 3, 2, 1, 1), (128, 16, 3, 0, 1), (129, 63, 5, 1, 0), (300, 64, 12, 0, 1),
         (300, 64, 2, 1, 1), (257, 5, 12, 1, 1)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    global H
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from neural_svd_amd import hip_ops
    H = hip_ops
    yield


def make_inputs(B, L, D, seed):
    g = np.random.default_rng(seed)
    x = (SIGMA * g.standard_normal((B, D))).astype(np.float32)
    if B >= 127:
        x[40:44] = SO.planted_rows(D)
    fa, fb = (g.standard_normal((B, L)).astype(np.float32) for _ in range(2))
    Ta, Tb = ((30.0 * g.standard_normal((B, L))).astype(np.float32) for _ in range(2))
    return x, (fa, Ta), (fb, Tb)


def reference(x, calls, gaussian, pad, weight32=False):
    cov = quad = tt = 0.0
    for f, Tf in calls:
        c, q, t = SO.accumulate(f, Tf, x, SIGMA, LIM, gaussian, pad, weight32)
        cov, quad, tt = cov + c, quad + q, tt + t
    return cov, quad, tt


def run_kernel(x, calls, gaussian, pad, dtype, c0, q0, lim=LIM, sigma=SIGMA):
    cov = torch.tensor(c0, dtype=dtype, device=DEV)
    quad = torch.tensor(q0, dtype=dtype, device=DEV)
    xd = torch.tensor(x, device=DEV)
    for f, Tf in calls:
        H.spectrum_accumulate(torch.tensor(f, device=DEV), torch.tensor(Tf, device=DEV), xd, sigma, bool(gaussian), lim,
                              cov, quad, first_mode_const=bool(pad))
    torch.cuda.synchronize()
    return cov.double().cpu().numpy(), quad.double().cpu().numpy()


@pytest.mark.parametrize("B,L,D,pad,gaussian", CASES)
def test_accumulators_against_float64(B, L, D, pad, gaussian):
    x, ca, cb = make_inputs(B, L, D, seed=1000 * B + 10 * L + D)
    if gaussian:
        assert float(SO.gauss_exponent(x, SIGMA).min()) > -80.0
    cov, quad, tt = reference(x, (ca, cb), gaussian, pad)
    cov32, quad32, _ = reference(x, (ca, cb), gaussian, pad, weight32=True)
    dc, dt = np.diag(cov), np.diag(tt)
    y_c, y_q = SO.entry_error(cov32, cov, dc, dc), SO.entry_error(quad32, quad, dc, dt)
    # non-zero starting values, a quarter of each entry's scale
    g = np.random.default_rng(B + L)
    Lp = L + pad
    c0 = 0.25 * np.sqrt(np.outer(dc, dc)) * g.uniform(-1, 1, (Lp, Lp))
    q0 = 0.25 * np.sqrt(np.outer(dc, dt)) * g.uniform(-1, 1, (Lp, Lp))
    got_c, got_q = run_kernel(x, (ca, cb), gaussian, pad, torch.float64, c0, q0)
    e_c, e_q = SO.entry_error(got_c, c0 + cov, dc, dc), SO.entry_error(got_q, q0 + quad, dc, dt)
    print(f"spectrum f64 (B={B}, L={L}, D={D}, pad={pad}, gauss={gaussian}): cov got {e_c:.2e} y {y_c:.2e}; "
          f"quad got {e_q:.2e} y {y_q:.2e}")
    assert e_c <= max(1e-6, 4 * y_c), (e_c, y_c)
    assert e_q <= max(1e-6, 4 * y_q), (e_q, y_q)
    if pad:
        return
    c0f, q0f = c0.astype(np.float32), q0.astype(np.float32)
    got_c, got_q = run_kernel(x, (ca, cb), gaussian, pad, torch.float32, c0f, q0f)
    e_c = SO.entry_error(got_c, c0f.astype(np.float64) + cov, dc, dc)
    e_q = SO.entry_error(got_q, q0f.astype(np.float64) + quad, dc, dt)
    print(f"spectrum f32 (B={B}, L={L}, D={D}): cov got {e_c:.2e}; quad got {e_q:.2e}")
    assert e_c <= 1e-5, e_c
    assert e_q <= 1e-4, e_q


@pytest.mark.parametrize("pad", [0, 1])
def test_non_finite_inputs(pad):
    """nan_to_num with float32 semantics (NaN -> 0, +-inf -> +-FLT_MAX) on both operands, then the x ~ 0 zeroing -
    also of a row whose Tf is inf. (129, 4, 2), no importance and lim = 0.5: the weight is exactly 1, and every product
    is finite in float64 (FLT_MAX^2 = 1.2e77). inf only in columns 0 and 2: the entries between the other columns keep
    their ordinary scale."""
    B, L, D = 129, 4, 2
    g = np.random.default_rng(7)
    x = g.standard_normal((B, D)).astype(np.float32)
    x[40:44] = SO.planted_rows(D)
    f = g.standard_normal((B, L)).astype(np.float32)
    Tf = (30.0 * g.standard_normal((B, L))).astype(np.float32)
    f[3, 1] = f[128, 3] = Tf[3, 3] = Tf[77, 1] = Tf[41, 1] = np.nan
    f[9, 0] = f[100, 2] = Tf[9, 0] = Tf[60, 2] = np.inf
    f[10, 0] = f[128, 2] = Tf[100, 0] = Tf[10, 2] = -np.inf
    Tf[40, 0] = np.inf   # the origin row: zeroed after nan_to_num
    Tf[42, 2] = -np.inf  # (0, 1): kept
    assert float(SO.sqrt_weight(x, 1.0, 0.5, False)[0]) == 1.0
    cov, quad, tt = SO.accumulate(f, Tf, x, 1.0, 0.5, False, pad)
    assert np.isfinite(cov).all() and np.isfinite(quad).all()
    dc, dt = np.diag(cov), np.diag(tt)
    Lp = L + pad
    z = np.zeros((Lp, Lp))
    got_c, got_q = run_kernel(x, ((f, Tf),), False, pad, torch.float64, z, z, lim=0.5, sigma=1.0)
    e_c, e_q = SO.entry_error(got_c, cov, dc, dc), SO.entry_error(got_q, quad, dc, dt)
    print(f"spectrum non-finite (pad={pad}): cov got {e_c:.2e}; quad got {e_q:.2e}")
    assert np.isfinite(got_c).all() and np.isfinite(got_q).all()
    assert e_c <= 1e-6 and e_q <= 1e-6, (e_c, e_q)


def _buffers(B=8, L=4, D=2, Lacc=4, dtype=torch.float64):
    g = torch.Generator().manual_seed(0)
    f, Tf, x = (torch.randn(B, n, generator=g).to(DEV) for n in (L, L, D))
    return f, Tf, x, torch.ones(Lacc, Lacc, dtype=dtype, device=DEV), torch.ones(Lacc, Lacc, dtype=dtype, device=DEV)


def test_refusals():
    # L = 65: past SMAXL, from all three entry points
    for dtype, pad in ((torch.float32, False), (torch.float64, False), (torch.float64, True)):
        f, Tf, x, cov, quad = _buffers(L=65, Lacc=65 + int(pad), dtype=dtype)
        with pytest.raises(H.NsvdError, match="NSVD_EUNSUPPORTED"):
            H.spectrum_accumulate(f, Tf, x, SIGMA, True, LIM, cov, quad, first_mode_const=pad)
        assert float(cov.sum()) == (65 + int(pad)) ** 2   # untouched
    f, Tf, x, cov, quad = _buffers()
    with pytest.raises(H.NsvdError):   # dtype mix
        H.spectrum_accumulate(f, Tf, x, SIGMA, True, LIM, cov, quad.float())
    with pytest.raises(H.NsvdError):   # the pad takes float64 accumulators
        H.spectrum_accumulate(f, Tf, x, SIGMA, True, LIM, torch.ones(5, 5, device=DEV), torch.ones(5, 5, device=DEV),
                              first_mode_const=True)
    with pytest.raises(H.NsvdError):   # (L, L) accumulators with the pad
        H.spectrum_accumulate(f, Tf, x, SIGMA, True, LIM, cov, quad, first_mode_const=True)
    f5, Tf5, x5, cov5, quad5 = _buffers(Lacc=5)
    with pytest.raises(H.NsvdError):   # (L + 1, L + 1) accumulators without it
        H.spectrum_accumulate(f5, Tf5, x5, SIGMA, True, LIM, cov5, quad5)
    with pytest.raises(H.NsvdError):   # float64 inputs
        H.spectrum_accumulate(f.double(), Tf, x, SIGMA, True, LIM, cov, quad)
    with pytest.raises(H.NsvdError):   # Tf of another shape
        H.spectrum_accumulate(f, Tf[:, :3].contiguous(), x, SIGMA, True, LIM, cov, quad)
    torch.cuda.synchronize()
    assert float(cov.sum()) == 16.0 and float(quad.sum()) == 16.0


def test_use_importance_at_the_c_abi():
    """use_importance is NSVD_IMP_*, not a truth value: NSVD_IMP_UNIFORM (2) is NSVD_EUNSUPPORTED - the kernel has the
    Gaussian density only, and used to evaluate it for 2 - and anything outside NSVD_IMP_* is NSVD_EINVAL; valid
    buffers, nothing launched, the accumulators untouched. 0 and 1 still run."""
    from neural_svd_amd import _lib
    lib = _lib.load()
    assert (_lib.IMP_NONE, _lib.IMP_GAUSSIAN, _lib.IMP_UNIFORM) == (0, 1, 2)
    stream = torch.cuda.current_stream().cuda_stream
    for name, dtype, Lacc in (("nsvd_spectrum_accumulate", torch.float32, 4),
                              ("nsvd_spectrum_accumulate_f64", torch.float64, 4),
                              ("nsvd_spectrum_accumulate_const_f64", torch.float64, 5)):
        f, Tf, x, cov, quad = _buffers(Lacc=Lacc, dtype=dtype)
        fn = getattr(lib, name)

        def call(imp):
            rc = fn(f.data_ptr(), Tf.data_ptr(), x.data_ptr(), 8, 4, 2, C.c_float(SIGMA), int(imp), C.c_float(LIM),
                    cov.data_ptr(), quad.data_ptr(), stream)
            torch.cuda.synchronize()
            return rc

        assert call(_lib.IMP_UNIFORM) == _lib.EUNSUPPORTED
        for bad in (3, -1, 256):
            assert call(bad) == _lib.EINVAL
        assert float(cov.sum()) == Lacc * Lacc and float(quad.sum()) == Lacc * Lacc
        assert call(_lib.IMP_NONE) == 0
        c_none = cov.clone()
        assert call(_lib.IMP_GAUSSIAN) == 0
        # the two densities differ: 1 against the Gaussian pdf (so 1 was not taken for 0, nor 0 for 1)
        d_none, d_gauss = c_none - 1.0, cov - c_none
        assert float(d_none.abs().sum()) > 0 and float(d_gauss.abs().sum()) > 0
        assert not torch.allclose(d_none, d_gauss, rtol=1e-3)
