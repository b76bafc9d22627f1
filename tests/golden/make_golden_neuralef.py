#!/usr/bin/env python3
"""Generate tests/golden/neuralef.npz by IMPORTING the reference's NeuralEF (methods/neuralef.py, methods/utils.py).

Runs only in the build container (needs /root/reference, imported the way make_golden.py does); the GPU box and the
test-suite never run it, they only read the committed npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_neuralef.py

Per case (hydrogen with Gaussian importance: both `unbiased` values, both batchnorm modes and 'none'; the oscillator
with its ExponentialMask; one odd batch), float64 (truth; float32: values only, no gradients): two training steps of the reference's own loop
body (compute_loss_operator, backward, RMSprop) recording x, phi, Tphi, the loss, every parameter gradient, both running
norms and the parameters after the step; then compute_spectrum_evd(normalize=False) on a small grid, and the
state_dict's keys / shapes / dtypes. No reference source text is stored: fixtures are arrays only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the stubs and puts the reference on sys.path)

from methods.general import get_evd_method  # noqa: E402
from methods.spectrum import compute_spectrum_evd  # noqa: E402
from examples.operator.pde.problems import get_problem  # noqa: E402
from examples.operator.pde import get_wavefunctions  # noqa: E402
from examples.operator.pde.main_pde import get_dataloader  # noqa: E402
from examples.utils import get_optimizer  # noqa: E402
from tools.generic import Namespace  # noqa: E402

OSC = dict(potential_type="harmonic_oscillator", operator_scale=1.0, operator_shift=16.0, sampling_scale=4.0,
           apply_exp_mask=1, exp_mask_init_scale=10.0, fourier_scale=1.0)
CASES = dict(
    hyd_ub=dict(neigs=4, unbiased=1, batchnorm_mode="unbiased"),
    hyd_bb=dict(neigs=5, unbiased=0, batchnorm_mode="biased"),
    hyd_ubb=dict(neigs=4, unbiased=1, batchnorm_mode="biased"),
    hyd_none=dict(neigs=4, unbiased=0, batchnorm_mode="none"),
    osc_mask=dict(neigs=6, unbiased=1, batchnorm_mode="unbiased", **OSC),
    hyd_odd=dict(neigs=4, unbiased=0, batchnorm_mode="unbiased", batch_size=25),
)


def make_args(case):
    c = dict(case)
    ub, mode = c.pop("unbiased"), c.pop("batchnorm_mode")
    a = G.make_args(**dict(dict(mlp_hidden_dims="16,16", fourier_mapping_size=8, batch_size=24), **c))
    a.loss = Namespace(dict(name="neuralef", neuralef=dict(unbiased=ub, batchnorm_mode=mode, include_diag=0),
                            neuralsvd=dict(step=1, sequential=1)))
    return a


def run_case(out, name, case, nsteps=2):
    args0 = make_args(case)
    torch.manual_seed(args0.seed + 1000)
    xs = [args0.sampling_scale * torch.randn((args0.batch_size, 1, args0.ndim)) for _ in range(nsteps)]
    out[f"{name}_x"] = np.stack([x.reshape(x.shape[0], -1).numpy() for x in xs])
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        args = make_args(case)
        torch.manual_seed(args.seed)
        operator, gt = get_problem(args, torch.device("cpu"))
        model = get_wavefunctions(args)
        _, val_data, batch_ftn_val, _, imp_val = get_dataloader(args, torch.device("cpu"))
        method = get_evd_method(args, "neuralef", model).to(dtype)
        imp_train = G.importance_for(args, dtype)
        store = (lambda t: G.np64(t)) if tag == "f64" else (lambda t: t.detach().cpu().float().numpy().copy())
        p = f"{name}_{tag}_"
        if tag == "f64":
            sd = method.state_dict()
            out[f"{name}_sd_keys"] = np.array(list(sd.keys()))
            out[f"{name}_sd_shapes"] = np.array([repr(tuple(v.shape)) for v in sd.values()])
            out[f"{name}_sd_dtypes"] = np.array([str(v.dtype) for v in method.float().state_dict().values()])
            method = method.to(dtype)
            out[f"{name}_param_names"] = np.array([n for n, t in method.named_parameters() if t.requires_grad])
            for n, t in method.named_parameters():
                if t.requires_grad:
                    out[f"{name}_param0_{n}"] = t.detach().float().numpy()
                elif n.endswith("feature_map._B"):
                    out[f"{name}_fourier_B"] = t.detach().float().numpy()
            out[f"{name}_cfg"] = np.array(repr({k: v for k, v in vars(args).items() if k != "loss"}))
            out[f"{name}_mode"] = np.array([case["unbiased"], {"none": 0, "biased": 1, "unbiased": 2}[case["batchnorm_mode"]]])
        optimizer = get_optimizer(args, method)
        bn = method.model if case["batchnorm_mode"] != "none" else None
        for it in range(nsteps):
            method.train()
            optimizer.zero_grad()
            x = xs[it].to(dtype).reshape(xs[it].shape[0], -1)
            loss, aux = method.compute_loss_operator(operator, x, importance=imp_train)
            loss.backward()
            out[p + f"step{it}_loss"] = G.np64(loss)
            out[p + f"step{it}_phi"] = store(aux["f"])
            out[p + f"step{it}_Tphi"] = store(aux["Tf"])
            if bn is not None:
                out[p + f"step{it}_norm_biased"] = G.np64(bn._norm_biased)
                out[p + f"step{it}_norm_unbiased"] = G.np64(bn._norm_unbiased)
            for n, t in method.named_parameters():
                if t.grad is not None and tag == "f64":
                    out[p + f"step{it}_grad_{n}"] = G.np64(t.grad)
            optimizer.step()
            if tag == "f64" and it == nsteps - 1:
                for n, t in method.named_parameters():
                    if t.requires_grad:
                        out[p + f"step{it}_param_{n}"] = G.np64(t)
        method.eval()
        with torch.no_grad():
            vd = val_data.to(dtype)
            bs = args.batch_size

            def loader():
                for i in range(int(np.ceil(len(vd) / float(bs)))):
                    yield vd[i * bs:min((i + 1) * bs, len(vd))], 0.

            res = compute_spectrum_evd(method, dataloader=loader(), operator=operator, importance_train=imp_train,
                                       importance_val=lambda z: imp_val(z).to(dtype), normalize=False,
                                       set_first_mode_const=False, device=torch.device("cpu"))
        out[p + "spec_eigvals"] = np.asarray(res["eigvals"], dtype=np.float64)
        out[p + "spec_norms"] = np.asarray(res["norms"], dtype=np.float64)
        if tag == "f64":
            out[f"{name}_val_data"] = val_data.numpy()


def main():
    out = {}
    for name, case in CASES.items():
        run_case(out, name, case)
    path = os.path.join(HERE, "neuralef.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
