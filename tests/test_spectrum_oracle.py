"""The float64 restatement of the spectrum accumulation (tests/_spectrum_oracle.py) against the reference's own float64
run of compute_spectrum_evd on recorded (Tphi, phi) (tests/golden/spectrum_acc.npz, made by
tests/golden/make_golden_spectrum.py): both set_first_mode_const values, with and without a Gaussian importance_train,
D = 1, 2, 3, rows at and around the origin, NaN entries. CPU only."""
import numpy as np
import pytest

from tests import _golden as G
from tests import _spectrum_oracle as SO


@pytest.fixture(scope="module")
def z():
    return G.load("spectrum_acc")


def test_fixture_holds_the_planted_rows(z):
    f, Tf = z["f"], z["Tf"]
    assert f.dtype == np.float32 and Tf.dtype == np.float32
    assert np.isnan(f).sum() >= 3 and np.isnan(Tf).sum() >= 3 and not np.isinf(f).any() and not np.isinf(Tf).any()
    for D in z["dims"]:
        x = z[f"x_D{D}"]
        assert x.dtype == np.float32 and np.array_equal(x[5:9], SO.planted_rows(int(D)))
        zeroed = np.all(np.abs(x.astype(np.float64)) <= 1e-8, axis=1)
        # ((0, 1, ...): some coordinates 0 only - at D = 1 the row is 1; 2e-8 is above isclose's 1e-8)
        assert zeroed[5] and zeroed[6] and not zeroed[7] and not zeroed[8] and int(zeroed.sum()) == 2


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("gaussian", [0, 1])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_restatement_matches_the_reference(z, D, gaussian, pad):
    sigma, lim = (float(t) for t in z["cfg"])
    cov, quad, tt = SO.accumulate(z["f"], z["Tf"], z[f"x_D{D}"], sigma, lim, bool(gaussian), pad)
    want_c, want_q = z[f"cov_D{D}_g{gaussian}_p{pad}"], z[f"quad_D{D}_g{gaussian}_p{pad}"]
    assert cov.shape == want_c.shape == (4 + pad, 4 + pad)
    dc = np.diag(want_c)
    assert SO.entry_error(cov, want_c, dc, dc) < 1e-12
    assert SO.entry_error(quad, want_q, dc, np.diag(tt)) < 1e-12
    assert np.linalg.norm(cov - want_c) < 1e-12 * np.linalg.norm(want_c)
    assert np.linalg.norm(quad - want_q) < 1e-12 * np.linalg.norm(want_q)


def test_the_zero_rule_and_the_pad_are_visible_in_the_fixture(z):
    """the fixture would not notice a restatement that ignored a rule if the rule changed nothing: dropping the x ~ 0
    zeroing, zeroing the (0, 1) row, or keeping the padded column on the zeroed rows each move quad by far more than
    the 1e-12 the restatement is held to"""
    sigma, lim = (float(t) for t in z["cfg"])
    f, Tf, x = z["f"], z["Tf"], z["x_D2"]
    want = z["quad_D2_g1_p1"]
    phi, tphi = SO.weighted(f, Tf, x, sigma, lim, True, 1)
    w = SO.sqrt_weight(x, sigma, lim, True)[:, None]
    raw = SO.nan_to_num32(np.concatenate([np.ones((len(x), 1)), w * Tf.astype(np.float64)], 1))
    for rows, cols in (([5], slice(None)), ([6], slice(None)), ([5, 6], slice(0, 1))):
        t = tphi.copy()
        t[rows, cols] = raw[rows, cols]
        assert np.linalg.norm(phi.T @ t - want) > 1e-6 * np.linalg.norm(want)
    t = tphi.copy()
    t[7] = 0.0
    assert np.linalg.norm(phi.T @ t - want) > 1e-6 * np.linalg.norm(want)


def test_float32_weight_yardstick_is_close_to_the_float64_weight():
    g = np.random.default_rng(0)
    for D in (1, 2, 5, 12):
        x = (16.0 * g.standard_normal((64, D))).astype(np.float32)
        w64, w32 = SO.sqrt_weight(x, 16.0, 50.0, True), SO.sqrt_weight(x, 16.0, 50.0, True, weight32=True)
        # float32 rounds the exponent -0.5 |x / sigma|^2 + log_norm (up to ~60 in size at D = 12) to 2^-24 relative:
        # up to 60 * 6e-8 / 2 = 2e-6 on sqrt(exp(.)); far below a formula that differs
        assert np.max(np.abs(w32 / w64 - 1)) < 5e-6
        u64, u32 = SO.sqrt_weight(x, 16.0, 50.0, False), SO.sqrt_weight(x, 16.0, 50.0, False, weight32=True)
        assert np.max(np.abs(u32 / u64 - 1)) < 3e-7
