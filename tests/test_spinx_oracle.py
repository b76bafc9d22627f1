"""CPU checks of SpINx (neural_svd_amd/spinx.py, csrc/spinx.hip): the float64 oracle (tests/_spinx_oracle.py) against
the fixture recorded from the reference's own SpINx (tests/golden/spinx.npz, make_golden_spinx.py), its hand-derived
cotangents against torch float64 autograd of the direct formula, the moment form of the residual losses against the
direct form, the NTK weights, the new symbols of the C ABI, and the refusals. No GPU.

Bounds: the oracle and the reference's float64 run are the same float64 arithmetic in another order on matrices with
cond <= 1e3 (asserted in the generator): 1e-9, as test_spin_oracle.py holds SpIN's oracle to. The weights: 2e-6, because
the reference's _update_weights accumulates the NTK norms in a float32 vector even in its float64 run (eps32 = 6e-8 per
accumulation, a square root halves it; 2e-6 leaves a factor of ten)."""
import os

import numpy as np
import pytest
import torch

from tests import _spinx_oracle as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "spinx.npz"))


def _oracle_of(z, name):
    fB, ws, bs, xs = X.load_case(z, name)
    return X.SpinxOracle(fB, ws, bs, X.CASES[name]["decay"], X.gaussian_kernel(X.ELL), X.case_c(name)), xs


def test_fixture_holds_arrays_only(golden):
    path = os.path.join(ROOT, "tests", "golden", "spinx.npz")
    assert os.path.getsize(path) < 1 << 20
    z = np.load(path, allow_pickle=False)
    for k in z.files:
        assert z[k].dtype.kind in "fi", k


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", sorted(X.CASES))
def test_oracle_matches_reference_float64(golden, name, split):
    """every recorded quantity of every step, and the weights after the last one, both split modes"""
    orc, xs = _oracle_of(golden, name)
    for kind, it, res in X.run_case(orc, xs, split):
        if kind == "weights":
            want, _ = X.unpack_weights(golden, name, split)
            e = X.rel_err(res, want)
            print(f"{name} split={split} weights: rel {e:.1e}")
            assert e <= 2e-6, (name, split)
            continue
        want, cond = X.unpack_step(golden, name, split, it)
        assert cond <= X.COND_MAX
        assert abs(float(res["cond"]) - cond) <= 1e-6 * cond
        for k, v in X.flat(res).items():
            assert X.rel_err(X.sample(v), want[k][0]) <= 1e-9, (name, split, it, k)


def _random_tall(L, seed, split):
    """P, K, Phi with cond(S + 1e-3 I) <= 1e3 (asserted): near-orthogonal columns, a non-symmetric mix for K"""
    g = torch.Generator().manual_seed(seed)
    B = 3 * L + 5
    B1 = (B + 1) // 2 if split else B
    Phi = torch.randn(B, L, generator=g, dtype=torch.float64) * (0.5 + torch.rand(L, generator=g, dtype=torch.float64))
    P = Phi[:B1]
    K = P @ torch.randn(L, L, generator=g, dtype=torch.float64) / L ** 0.5 + \
        0.3 * torch.randn(B1, L, generator=g, dtype=torch.float64)
    S = Phi.T @ Phi / B
    cond = float(torch.linalg.cond(S + 1e-3 * torch.eye(L, dtype=torch.float64)))
    assert cond <= 1e3, cond
    return P, K, Phi


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("L", [2, 5, 16, 64])
def test_moment_form_is_the_direct_form(L, split):
    P, K, Phi = _random_tall(L, 10 + L, split)
    tw = 0.5 + torch.rand(L, dtype=torch.float64, generator=torch.Generator().manual_seed(L))
    direct = X.losses_direct(P, K, Phi, tw)
    moment = X.losses_moment(*X.moments(P, K, Phi), tw)[0]
    e = float((moment - direct).abs().max() / direct.abs().max())
    print(f"L={L} split={split}: moment vs direct {e:.1e}")
    assert e <= 1e-12


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("L", [2, 5, 16, 64])
def test_cotangents_against_autograd(L, split):
    """the hand-derived dP, dK, dPhi against torch float64 autograd through cholesky, inverse and residuals"""
    P0, K0, Phi0 = _random_tall(L, 20 + L, split)
    B, B1 = Phi0.shape[0], P0.shape[0]
    g = torch.Generator().manual_seed(L)
    w = 0.5 + torch.rand(L + 1, dtype=torch.float64, generator=g)
    tw = 0.5 + torch.rand(L, dtype=torch.float64, generator=g)
    Phi = Phi0.clone().requires_grad_(True)
    K = K0.clone().requires_grad_(True)
    loss = (X.losses_direct(Phi[:B1], K, Phi, tw) * w).sum() / L
    gPhi, gK = torch.autograd.grad(loss, (Phi, K))
    sol = X.solve(*X.moments(P0, K0, Phi0), w, tw)
    T = X.rotations(sol, B, B1)
    dK = P0 @ T["T_pk"] + K0 @ T["T_kk"]
    dPhi = Phi0 @ T["T_s"]
    dPhi[:B1] = P0 @ T["T_pp"] + K0 @ T["T_kp"]
    assert abs(float(sol["loss"] - loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    eK, eP = X.rel_err(dK, gK), X.rel_err(dPhi, gPhi)
    print(f"L={L} split={split}: dK {eK:.1e} dPhi {eP:.1e}")
    assert eK <= 1e-10 and eP <= 1e-10
    if split:
        assert float(gPhi[B1:].norm()) > 0


def test_weights_pick_single_losses(golden):
    """w = L e_k makes the loss losses_k: the recipe of update_weights_kernel"""
    orc, xs = _oracle_of(golden, "a")
    res = orc.step(xs[0], False)
    L = orc.L
    ps = [p.clone().requires_grad_(True) for p in orc.params()]
    Phi, P, K = orc._tall(xs[0], False, ps)
    for k in (0, 1, L):
        e = torch.zeros(L + 1, dtype=torch.float64)
        e[k] = L
        sol, _ = orc._grads(Phi, P, K, ps, e)
        assert abs(float(sol["loss"] - sol["losses"][k])) <= 1e-14 * abs(float(sol["losses"][k]))
    assert res["losses"].numel() == L + 1


# ---- the package side ------------------------------------------------------------------------------------------------
def _build_spinx(name, fB, ws, bs):
    from neural_svd_amd.models import GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    from neural_svd_amd.spinx import SpINx
    cs = X.CASES[name]
    fm = GaussianFourierFeatureTransform(input_dim=cs["D"], mapping_size=cs["m"], scale=X.FOURIER_SCALE)
    base = ParallelMLP(input_dim=cs["D"], mlp_hidden_dims=list(cs["hidden"]), output_dim=1, num_copies=cs["L"],
                       nonlinearity="softplus", bias=True, feature_map=fm)
    model = WaveFunctions(base, boundary_mask=lambda x: 1.0, hard_mul_const=X.case_c(name))
    with torch.no_grad():
        fm._B.copy_(fB)
        for dst, src in zip(list(base.ws) + list(base.bs), list(ws) + list(bs)):
            dst.copy_(src)
    return SpINx(model, cs["L"], cs["decay"])


def test_state_dict_keys_and_name(golden):
    fB, ws, bs, _ = X.load_case(golden, "t3")
    m = _build_spinx("t3", fB, ws, bs)
    L = X.CASES["t3"]["L"]
    assert m.name == "spinx"
    sd = m.state_dict()
    assert tuple(sd["sigma_avg"].shape) == (L, L) and tuple(sd["chol"].shape) == (L, L)
    assert tuple(sd["spinx_loss_ftn.trace_weights"].shape) == (L,)
    assert not any(p.requires_grad for p in (m.sigma_avg, m.chol, m.spinx_loss_ftn.trace_weights))
    assert "weights" not in sd and not isinstance(m.weights, torch.nn.Parameter)
    assert torch.equal(m.weights, torch.ones(L + 1))


def test_new_symbols_are_declared_bound_and_exported():
    from neural_svd_amd import _lib
    from tests.test_abi import _declared, _exported
    new = {"nsvd_spinx_solve", "nsvd_ts_rotate2"}
    assert new <= set(_declared()) and new <= set(_lib.SIGNATURES)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert new <= set(_exported(_lib.LIB_PATH))
    assert _lib.load().nsvd_abi_version() == 6  # new symbols only


def test_host_side_refusals_of_the_entry_points():
    """argument checks that return before any launch: no GPU needed"""
    import ctypes
    from neural_svd_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    q = p + 4096
    E, U = _lib.EINVAL, _lib.EUNSUPPORTED

    def solve(L, decay=0.01, update=1, state=p, S=p):
        return lib.nsvd_spinx_solve(S, 1.0, p, p, p, 1.0, L, p, None, decay, update, state, state, p, p, p, p, p, p, p,
                                    None)
    assert solve(1) == E and solve(65) == U
    assert solve(4, decay=-0.1) == E and solve(4, decay=1.5) == E and solve(4, decay=float("nan")) == E
    assert solve(4, state=None) == E and solve(4, S=None) == E

    def rot(n=8, m=4, k=4, out=q, X_=p, Y_=p, ld=4):
        return lib.nsvd_ts_rotate2(X_, ld, Y_, ld, n, m, p, m, p, m, k, out, ld, None)
    assert rot(m=81, k=81, ld=81) == U
    assert rot(k=5) == E and rot(k=0) == E and rot(n=0) == E and rot(ld=3) == E
    assert rot(out=p) == E                       # out aliases X (and Y)
    assert rot(X_=q, out=p) == E                 # out aliases Y
    assert rot(X_=None) == E


def test_refusals(golden):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.models import ExponentialMask, GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    from neural_svd_amd.spinx import SpINx, SpinxKernelTrainer
    fB, ws, bs, xs = X.load_case(golden, "t3")
    m = _build_spinx("t3", fB, ws, bs)
    L = X.CASES["t3"]["L"]
    x = xs[0]
    foreign = lambda x_ref: (lambda model, x, importance=None: (model(x), model(x)))  # noqa: E731
    op = RadialKernelOperator(H.RBF_GAUSSIAN, X.ELL, X.CASES["t3"]["D"])
    for fn in (m.compute_loss_kernel, m.update_weights_kernel):
        with pytest.raises(NotImplementedError, match="MatrixFreeKernelOperator"):
            fn(foreign, x, None, False)
        with pytest.raises(NotImplementedError, match="importance"):
            fn(op.get_approx_kernel_op, x, lambda z: torch.ones(len(z)), False)
    for fn in (m.compute_loss_operator, m.compute_losses_operator):
        with pytest.raises(NotImplementedError, match="stencil"):
            fn(None, x, None)
    with pytest.raises(NotImplementedError, match="stencil"):
        m.update_weights_operator(None, x, None, False)
    with pytest.raises(ValueError):
        SpINx(m.model, 1, 0.01)
    with pytest.raises(ValueError):
        SpINx(m.model, L + 1, 0.01)  # not the model's head count
    for decay in (-0.1, 1.5):
        with pytest.raises(ValueError):
            SpINx(m.model, L, decay)
    with pytest.raises(NotImplementedError, match="WaveFunctions"):
        SpINx(torch.nn.Linear(2, L), L, 0.01)
    fm = GaussianFourierFeatureTransform(input_dim=2, mapping_size=4, scale=1.0)
    base = ParallelMLP(input_dim=2, mlp_hidden_dims=[6], output_dim=1, num_copies=L, nonlinearity="softplus", bias=True,
                       feature_map=fm)
    masked = WaveFunctions(base, boundary_mask=ExponentialMask(L, init_scale=10.0), hard_mul_const=1.0)
    with pytest.raises(NotImplementedError, match="mask"):
        SpINx(masked, L, 0.01)
    with pytest.raises(NotImplementedError):
        SpinxKernelTrainer(object(), L, 4)


def test_factory_keeps_raising_and_names_the_class():
    from neural_svd_amd.nested_lowrank import get_evd_method
    with pytest.raises(NotImplementedError, match=r"neural_svd_amd\.spinx\.SpINx\.compute_loss_kernel"):
        get_evd_method(None, "spinx", None)


def test_exports():
    import neural_svd_amd
    from neural_svd_amd.spinx import SpINx, SpinxKernelTrainer
    assert neural_svd_amd.SpINx is SpINx and neural_svd_amd.SpinxKernelTrainer is SpinxKernelTrainer
