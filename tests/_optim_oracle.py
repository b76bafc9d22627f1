"""float64 numpy restatement of the optimiser rules of the reference's PDE loop (examples/utils.py:48-72 as stepped at
examples/operator/__init__.py:69-73): torch.optim.SGD / RMSprop / Adam with weight_decay 0, dampening 0, no Nesterov,
no amsgrad, not centred; the torch_ema update with its warm-up; CosineAnnealingLR's closed form.
tests/test_optim_oracle.py holds it to the installed torch.optim objects; the kernels are held to it."""
import math

import numpy as np

KINDS = ("sgd", "rmsprop", "adam")


def cosine_lr(lr0, t, T, eta_min=0.0):
    """learning rate after t scheduler steps (T = 0: constant)"""
    if not T:
        return lr0
    return eta_min + (lr0 - eta_min) * (1.0 + math.cos(math.pi * t / T)) / 2.0


def ema_decay_at(decay, n):
    """torch_ema's decay at its n-th update (n from 1)"""
    return min(decay, (1.0 + n) / (10.0 + n))


def uses(kind, momentum):
    """(sq slot, mom slot)"""
    if kind == "adam":
        return True, True
    if kind == "rmsprop":
        return True, momentum != 0.0
    if kind == "sgd":
        return False, momentum != 0.0
    raise ValueError(kind)


class State:
    """p, optional sq / mom / ema (float64 arrays), steps taken"""

    def __init__(self, p, kind, momentum=0.0, ema=True):
        self.kind, self.momentum = kind, float(momentum)
        self.p = np.array(p, dtype=np.float64)
        has_sq, has_mom = uses(kind, self.momentum)
        self.sq = np.zeros_like(self.p) if has_sq else None
        self.mom = np.zeros_like(self.p) if has_mom else None
        self.ema = self.p.copy() if ema else None
        self.t = 0


def step(st, grad, lr, alpha=0.99, eps=1e-10, betas=(0.9, 0.999), ema_decay=0.0, grad_scale=1.0):
    """one step with the already scheduled lr and the already warmed-up EMA decay"""
    g = grad_scale * np.asarray(grad, dtype=np.float64)
    mu = st.momentum
    if st.kind == "sgd":
        if mu == 0.0:
            st.p -= lr * g
        else:
            st.mom = g.copy() if st.t == 0 else mu * st.mom + g
            st.p -= lr * st.mom
    elif st.kind == "rmsprop":
        st.sq = alpha * st.sq + (1.0 - alpha) * g * g
        avg = np.sqrt(st.sq) + eps
        if mu == 0.0:
            st.p -= lr * g / avg
        else:
            st.mom = mu * st.mom + g / avg
            st.p -= lr * st.mom
    elif st.kind == "adam":
        b1, b2 = betas
        t = st.t + 1
        st.mom = st.mom + (1.0 - b1) * (g - st.mom)
        st.sq = b2 * st.sq + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        st.p -= (lr / bc1) * st.mom / (np.sqrt(st.sq) / math.sqrt(bc2) + eps)
    else:
        raise ValueError(st.kind)
    if st.ema is not None:
        st.ema -= (1.0 - ema_decay) * (st.ema - st.p)
    st.t += 1


def run(kind, momentum, p0, grads, lr0, T_max, alpha=0.99, eps=1e-10, betas=(0.9, 0.999), ema_decay=None,
        grad_scale=1.0):
    """len(grads) scheduled steps (cosine learning rate over T_max, EMA warm-up); ema_decay None: no EMA"""
    st = State(p0, kind, momentum, ema=ema_decay is not None)
    for t, g in enumerate(grads):
        step(st, g, cosine_lr(lr0, t, T_max), alpha, eps, betas,
             ema_decay_at(ema_decay, t + 1) if ema_decay is not None else 0.0, grad_scale)
    return st
