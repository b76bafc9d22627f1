"""CPU checks of SpIN (neural_svd_amd/spin.py, csrc/spin.hip): the float64 oracle (tests/_spin_oracle.py) against the
fixture recorded from the reference's own SpIN (tests/golden/spin.npz, make_golden_spin.py), the compact <-> dense
conversion of the Jacobian state, the new symbols of the C ABI, and the refusals. No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import _spin_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "spin.npz"))


def _oracle_of(z, name):
    fB, ws, bs, xs = S.load_case(z, name)
    # the per-sample loop for the narrow cases; the wide ones take the batched form of the same contraction, which
    # test_batched_contraction_is_the_per_sample_loop pins to the loop
    wide = S.CASES[name]["L"] * sum(t.numel() for t in ws) > 50000
    return S.SpinOracle(fB, ws, bs, S.CASES[name]["decay"], S.gaussian_kernel(S.ELL), S.case_c(name),
                        S.jacobian_contraction_einsum if wide else None), xs


def _flat(res):
    q = dict(loss=res["loss"], eigvals=res["eigvals"], sigma_avg=res["sigma_avg"], chol=res["chol"], phi=res["phi"],
             Kphi=res["Kphi"])
    for i, (t2, g) in enumerate(zip(res["term2"], res["grad"])):
        q[f"term2_{i}"], q[f"grad_{i}"] = t2, g
    return q


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_oracle_matches_reference_float64(golden, name, split):
    """every recorded quantity of every step to 1e-9 of the reference's float64 run, both split modes"""
    orc, xs = _oracle_of(golden, name)
    for it in range(S.NSTEPS):
        res = orc.step(xs[it], split)
        want, cond = S.unpack_step(golden, name, split, it)
        assert cond <= S.COND_MAX
        assert abs(float(res["cond"]) - cond) <= 1e-6 * cond
        for k, v in _flat(res).items():
            assert S.rel_err(S.sample(v), want[k][0]) <= 1e-9, (name, split, it, k)
        orc.sgd(res["grad"], S.LR)


def test_batched_contraction_is_the_per_sample_loop(golden):
    fB, ws, bs, xs = S.load_case(golden, "a")
    fB, ws, bs, x = fB.double(), [w.double() for w in ws], [b.double() for b in bs], xs[0].double()
    phi = S.model_forward(x, fB, ws, bs, 0.7)
    for a, b in zip(S.jacobian_contraction(x, phi, fB, ws, bs, 0.7),
                    S.jacobian_contraction_einsum(x, phi, fB, ws, bs, 0.7)):
        assert S.rel_err(b, a) <= 1e-12


def test_abs_contraction_bounds_the_contraction(golden):
    """jacobian_contraction_abs, the scale of the GPU tests' per-slice error metric: |j_new| <= A element by element
    (equal where no term changes sign: the last layer's bias, whose delta is the constant hard_mul_const, times |phi|)"""
    fB, ws, bs, xs = S.load_case(golden, "a")
    fB, ws, bs, x = fB.double(), [w.double() for w in ws], [b.double() for b in bs], xs[0].double()
    phi = S.model_forward(x, fB, ws, bs, 0.7)
    J = S.jacobian_contraction_einsum(x, phi, fB, ws, bs, 0.7)
    A = S.jacobian_contraction_abs(x, phi, fB, ws, bs, 0.7)
    assert len(J) == len(A) == 2 * len(ws)
    for j, a in zip(J, A):
        assert tuple(j.shape) == tuple(a.shape)
        assert bool((a > 0).all()) and bool((j.abs() <= a * (1 + 1e-12)).all())
    # the signed sum does cancel somewhere: the bound is not the contraction itself
    assert any(bool((j.abs() < 0.5 * a).any()) for j, a in zip(J, A))
    want = 2.0 * 0.7 * phi.abs().mean(0)  # A of the last bias: (2 / B1) sum_b |phi[b, a]| c for every head
    L = phi.shape[1]
    assert S.rel_err(A[-1].reshape(L, L), want[:, None].expand(L, L)) <= 1e-12


def _build_spin(name, fB, ws, bs):
    from neural_svd_amd.models import GaussianFourierFeatureTransform, ParallelMLP, WaveFunctions
    from neural_svd_amd.spin import SpIN
    cs = S.CASES[name]
    fm = GaussianFourierFeatureTransform(input_dim=cs["D"], mapping_size=cs["m"], scale=S.FOURIER_SCALE)
    base = ParallelMLP(input_dim=cs["D"], mlp_hidden_dims=list(cs["hidden"]), output_dim=1, num_copies=cs["L"],
                       nonlinearity="softplus", bias=True, feature_map=fm)
    model = WaveFunctions(base, boundary_mask=lambda x: 1.0, hard_mul_const=S.case_c(name))
    with torch.no_grad():
        fm._B.copy_(fB)
        for dst, src in zip(list(base.ws) + list(base.bs), list(ws) + list(bs)):
            dst.copy_(src)
    return SpIN(model, cs["L"], cs["decay"])


@pytest.mark.parametrize("split", [False, True])
def test_expand_and_load_j_avg_round_trip(golden, split):
    """the compact state expands to the reference's dense j_avg.<name> tensors (recorded after three steps of the
    smallest case) and loads back from them"""
    name = "t3"
    orc, xs = _oracle_of(golden, name)
    for it in range(S.NSTEPS):
        res = orc.step(xs[it], split)
        orc.sgd(res["grad"], S.LR)
    fB, ws, bs, _ = S.load_case(golden, name)
    spin = _build_spin(name, fB, ws, bs)
    L = S.CASES[name]["L"]
    n = len(ws)
    keys = [f"model_base_ws_{i}" for i in range(n)] + [f"model_base_bs_{i}" for i in range(n)]
    keys = [k[len("model_"):] for k in keys]
    dense = {k: torch.from_numpy(golden[f"{name}_s{int(split)}_javg_{i}"]) for i, k in enumerate(keys)}
    # the oracle's compact state is the reference's dense one on the head-diagonal slices, and nothing else is non-zero
    for j, full, k in zip(orc.J, orc.expand(), keys):
        assert S.rel_err(full, dense[k]) <= 1e-9
    with torch.no_grad():
        spin.j_avg.copy_(torch.cat([j.reshape(L, -1) for j in orc.J], dim=1).float())
    got = spin.expand_j_avg()
    assert set(got) == set(keys) | {"base_feature_map__B"}
    assert not bool(got["base_feature_map__B"].count_nonzero())
    for k in keys:
        assert tuple(got[k].shape) == tuple(dense[k].shape)
        assert S.rel_err(got[k], dense[k]) <= 1e-6  # (the state is float32)
    compact = spin.j_avg.data.clone()
    spin.j_avg.data.zero_()
    spin.load_j_avg({"j_avg." + k: v for k, v in dense.items()})
    assert S.rel_err(spin.j_avg.data, compact) <= 1e-6
    bad = {k: v.clone() for k, v in dense.items()}
    bad[keys[0]][0, 1, 0] += 1.0  # head 1's output does not depend on head 0's weights
    from neural_svd_amd._lib import NsvdError
    with pytest.raises(NsvdError):
        spin.load_j_avg(bad)


def test_state_dict_keys_and_name(golden):
    fB, ws, bs, _ = S.load_case(golden, "t3")
    spin = _build_spin("t3", fB, ws, bs)
    assert spin.name == "spin"
    sd = spin.state_dict()
    L = S.CASES["t3"]["L"]
    assert tuple(sd["sigma_avg"].shape) == (L, L) and tuple(sd["chol"].shape) == (L, L)
    assert tuple(sd["j_avg"].shape) == (L, sum(t.numel() for t in list(ws) + list(bs)))
    assert not any(p.requires_grad for p in (spin.sigma_avg, spin.chol, spin.j_avg))


def test_new_symbols_are_declared_bound_and_exported():
    from neural_svd_amd import _lib
    from tests.test_abi import _declared, _exported
    new = {"nsvd_spin_solve", "nsvd_spin_state_floats", "nsvd_spin_jac_workspace_bytes", "nsvd_spin_jac_step"}
    assert new <= set(_declared()) and new <= set(_lib.SIGNATURES)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert new <= set(_exported(_lib.LIB_PATH))
    assert _lib.load().nsvd_abi_version() == 6  # new symbols only


def test_host_side_queries(golden):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd._lib import NsvdError
    for name, cs in S.CASES.items():
        shape = H.ModelShape(L=cs["L"], D=cs["D"], m=cs["m"], hidden=cs["hidden"])
        assert H.spin_state_floats(shape) == sum(int(np.prod(s)) for s in shape.param_shapes())
    with pytest.raises(NsvdError):  # the kernel-operator models have no mask
        H.spin_state_floats(H.ModelShape(L=4, D=2, m=8, hidden=(16,), has_exp_mask=True))
    with pytest.raises(NsvdError):
        H.spin_state_floats(H.ModelShape(L=4, D=2, m=8, hidden=(16,), box_mask=H.BOX_SQRT, box_lim=1.0))


def test_refusals(golden):
    from neural_svd_amd import hip_ops as H
    from neural_svd_amd.kernel_ops import RadialKernelOperator
    from neural_svd_amd.spin import SpIN
    fB, ws, bs, xs = S.load_case(golden, "t3")
    spin = _build_spin("t3", fB, ws, bs)
    x = xs[0]
    with pytest.raises(NotImplementedError, match="MatrixFreeKernelOperator"):
        spin.compute_loss_kernel(lambda x_ref: (lambda model, x, importance=None: (model(x), model(x))), x, None, False)
    op = RadialKernelOperator(H.RBF_GAUSSIAN, S.ELL, S.CASES["t3"]["D"])
    with pytest.raises(NotImplementedError, match="importance"):
        spin.compute_loss_kernel(op.get_approx_kernel_op, x, lambda z: torch.ones(len(z)), False)
    with pytest.raises(NotImplementedError, match="stencil"):
        spin.compute_loss_operator(None, x, None)
    with pytest.raises(ValueError):  # the reference's own class fails there: spin_step receives a 0-D pi
        SpIN(spin.model, 1, 0.01)
    # use_vmap is accepted and ignored
    assert SpIN(spin.model, S.CASES["t3"]["L"], 0.01, use_vmap=False).use_vmap is False
