"""Checkpoint interchange with the reference (examples/operator/__init__.py:139-145 saves
dict(args, method=method.state_dict(), ema=ema.state_dict(), optimizer=optimizer.state_dict())): a `.pth` written from
this package's modules holds exactly what the REFERENCE's own NestedLoRA / WaveFunctions load with strict=True, and a
reference state_dict loads into ours the other way round, through torch.save / torch.load; the EMA entry has
torch_ema's keys. The reference side is tests/golden/checkpoint.npz (tests/golden/make_golden.py:golden_checkpoint):
its state_dict keys in order with shapes and dtypes, its trainable tensor count, its optimiser's param_groups, and one
of its state_dicts. CPU only."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _args(**over):
    # tests/golden/make_golden.py:make_args - the reference's argument namespace, as its scripts fill it
    a = argparse.Namespace(
        seed=0, ndim=2, n_particles=1, neigs=4, mlp_hidden_dims="32,32", nonlinearity="softplus", parallel=1,
        weight_normalization=0, use_fourier_feature=True, fourier_mapping_size=16, fourier_scale=0.1,
        fourier_deterministic=False, fourier_append_raw=False, apply_boundary=0, boundary_mode="dir_box_sqrt", lim=5.0,
        apply_exp_mask=0, exp_mask_init_scale=10.0, hard_mul_const=1.0, problem="sch", potential_type="hydrogen",
        charge=1.0, laplacian_eps=0.01, operator_scale=100.0, operator_shift=0.0, sampling_mode="gaussian",
        sampling_scale=16.0, batch_size=24, val_eps=0.5, optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999,
        momentum=0.0, num_iters=100, sort=0)
    seq = over.pop("sequential", 1)
    step = over.pop("step", 1)
    for k, v in over.items():
        setattr(a, k, v)
    a.loss = argparse.Namespace(name="neuralsvd", neuralsvd=argparse.Namespace(step=step, sequential=seq))
    return a


def _reference_case(i):
    z = np.load(os.path.join(HERE, "golden", "checkpoint.npz"))
    meta = json.loads(str(z[f"case{i}_meta"]))
    sd = {k: torch.from_numpy(z[f"case{i}_sd.{k}"].copy()) for k in meta["keys"]}
    return meta, sd


def _matches_reference_layout(sd, meta):
    """what the reference's load_state_dict(strict=True) demands of a state_dict: exactly its keys, each of its shape
    (and, for a bitwise round trip, its dtype)"""
    assert list(sd.keys()) == meta["keys"]
    for (k, t), shape, dtype in zip(sd.items(), meta["shapes"], meta["dtypes"]):
        assert list(t.shape) == shape and str(t.dtype) == dtype, k


@pytest.mark.parametrize("case, over", [(0, dict(neigs=4, mlp_hidden_dims="32,32", fourier_mapping_size=16)),
                                        (1, dict(neigs=3, mlp_hidden_dims="128,128,128", fourier_mapping_size=64,
                                                 potential_type="harmonic_oscillator", apply_exp_mask=1,
                                                 exp_mask_init_scale=10.0, sequential=0))],
                         ids=["over0", "over1"])
def test_state_dicts_load_both_ways_through_a_pth_file(tmp_path, case, over):
    from neural_svd_amd.drop_in import ExponentialMovingAverage, get_optimizer
    from neural_svd_amd.models import get_wavefunctions
    from neural_svd_amd.nested_lowrank import get_evd_method
    meta, ref_sd = _reference_case(case)
    args = _args(**dict(over))
    torch.manual_seed(3)
    ours = get_evd_method(args, "neuralsvd", get_wavefunctions(args))
    _matches_reference_layout(ours.state_dict(), meta)
    # ours -> file -> reference
    ema = ExponentialMovingAverage(ours.parameters(), decay=0.995)
    opt = get_optimizer(argparse.Namespace(optimizer="rmsprop", lr=1e-4, rmsprop_decay=0.999, momentum=0.0), ours)
    path = os.path.join(str(tmp_path), "100.pth")
    torch.save(dict(method=ours.state_dict(), ema=ema.state_dict(), optimizer=opt.state_dict()), path)
    ck = torch.load(path, weights_only=False)
    _matches_reference_layout(ck["method"], meta)
    for (k, a), b in zip(ours.state_dict().items(), ck["method"].values()):
        assert torch.equal(a, b), k
    assert set(ck["ema"].keys()) == {"decay", "num_updates", "shadow_params", "collected_params"}
    assert len(ck["ema"]["shadow_params"]) == meta["n_trainable"]
    # the reference's optimiser loads this state: same class, same parameter groups with the same parameter order and
    # hyper-parameters
    assert type(opt).__name__ == meta["optimizer"]
    groups = ck["optimizer"]["param_groups"]
    assert len(groups) == len(meta["param_groups"])
    for g, want in zip(groups, meta["param_groups"]):
        for k in ("params", "lr", "alpha", "eps", "momentum", "centered", "weight_decay"):
            assert g[k] == want[k], (k, g[k], want[k])
    # reference -> file -> ours, and the EMA state back into a fresh EMA object
    torch.save(dict(method=ref_sd), path)
    ours.load_state_dict(torch.load(path, weights_only=False)["method"], strict=True)
    for (k, a), b in zip(ours.state_dict().items(), ref_sd.values()):
        assert torch.equal(a, b), k
    ema2 = ExponentialMovingAverage(ours.parameters(), decay=0.9)
    ema2.load_state_dict(ck["ema"])
    assert ema2.decay == 0.995 and ema2.num_updates == 0 and ema2.collected_params is None
