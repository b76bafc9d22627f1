"""Float64 restatement of the deep ReLU kinds of the dot-product kernel operator (nsvd_dot_apply / nsvd_dot_apply_pair
with NSVD_DOT_RELU_NNGP and NSVD_DOT_RELU_NTK, kernel_ops.DotKernelOperator): the NNGP kernel S_depth and the neural
tangent kernel T_depth of a ReLU network `depth` layers deep with weight variance gamma and bias variance coef0.

    A1(c) = (sin t + (pi - t) cos t) / pi,  A0(c) = (pi - t) / pi,  cos t = c clamped to [-1, 1]
    S_0 = T_0 = x.y,  q_0(x) = |x|^2,  and for l = 1 .. depth
        p = sqrt(q_{l-1}(x) q_{l-1}(y)),  c = S_{l-1} / p,  S_l = gamma p A1(c) + coef0,
        T_l = S_l + gamma T_{l-1} A0(c),  q_l(x) = gamma q_{l-1}(x) + coef0

Where p = 0 both A terms are taken as 0: S_l = T_l = coef0. The bracket of A1 is clamped at 0 from below, and sin t and
pi - t come from the same clamped c (sqrt((1 - c)(1 + c)) and acos(-c)), the rules of tests/_dot_oracle.py's ARCCOS1.
`relu_gram_form` is the same kernels computed the other way - each level's diagonal read off the level's own Gram
matrix - for the test that the closed-form diagonals q_l state nothing new."""
import math

import torch

RELU_NNGP, RELU_NTK = 3, 4


def _check(kind, gamma, coef0, depth):
    if kind not in (RELU_NNGP, RELU_NTK):
        raise ValueError(kind)
    if int(depth) != depth or not 1 <= depth <= 8:
        raise ValueError(depth)
    if not (gamma > 0 and math.isfinite(gamma)) or not (coef0 >= 0 and math.isfinite(coef0)):
        raise ValueError((gamma, coef0))


def a1_a0(c):
    """(A1, A0) of a float64 tensor of cosines, clamped here"""
    c = c.clamp(-1.0, 1.0)
    ac = torch.acos(-c)
    bracket = (torch.sqrt((1.0 - c) * (1.0 + c)) + ac * c).clamp(min=0.0)
    return bracket / math.pi, ac / math.pi


def _level(S, T, p, gamma, coef0):
    ok = p > 0
    c = torch.where(ok, S / torch.where(ok, p, torch.ones_like(p)), torch.zeros_like(p))
    A1, A0 = a1_a0(c)
    flat = torch.full_like(p, float(coef0))
    S1 = torch.where(ok, gamma * p * A1 + coef0, flat)
    T1 = torch.where(ok, S1 + gamma * T * A0, flat)
    return S1, T1


def relu_kernel_matrix(x, y, kind, gamma=1.0, coef0=0.0, depth=1):
    _check(kind, gamma, coef0, depth)
    x, y = torch.as_tensor(x).double(), torch.as_tensor(y).double()
    gamma, coef0 = float(gamma), float(coef0)
    S = x @ y.T
    T = S.clone()
    qx, qy = (x * x).sum(1), (y * y).sum(1)
    for _ in range(int(depth)):
        p = torch.sqrt(qx[:, None] * qy[None, :])
        S, T = _level(S, T, p, gamma, coef0)
        qx, qy = gamma * qx + coef0, gamma * qy + coef0
    return S if kind == RELU_NNGP else T


def relu_gram_form(x, kind, gamma=1.0, coef0=0.0, depth=1):
    """the symmetric Gram of x with itself, each level's q read off the diagonal of the level's own S"""
    _check(kind, gamma, coef0, depth)
    x = torch.as_tensor(x).double()
    gamma, coef0 = float(gamma), float(coef0)
    S = x @ x.T
    T = S.clone()
    for _ in range(int(depth)):
        q = S.diagonal().clone()
        p = torch.sqrt(q[:, None] * q[None, :])
        S, T = _level(S, T, p, gamma, coef0)
    return S if kind == RELU_NNGP else T


def relu_kernel_apply(x, y, f, kind, gamma, coef0, depth, scale):
    return scale * (relu_kernel_matrix(x, y, kind, gamma, coef0, depth) @ torch.as_tensor(f).double())


def relu_kernel_apply_pair(x, y, g, f, kind, gamma, coef0, depth, scale_g, scale_f):
    K = relu_kernel_matrix(x, y, kind, gamma, coef0, depth)
    return scale_g * (K @ torch.as_tensor(g).double()), scale_f * (K.T @ torch.as_tensor(f).double())


def relu_kernel_matrix32(x, y, kind, gamma, coef0, depth):
    """The yardstick of the GPU tests: the same recursion composed in float32 from library calls on x's device (x @ y.T,
    elementwise torch ops), as tests/test_dot_apply_gpu.py composes ARCCOS1 - through t = acos(c) and sin(t)."""
    S = x @ y.T
    T = S.clone()
    qx, qy = (x * x).sum(1), (y * y).sum(1)
    for _ in range(int(depth)):
        p = torch.sqrt(qx[:, None] * qy[None, :])
        c = (S / p).clamp(-1.0, 1.0)
        t = torch.acos(c)
        A1 = (torch.sin(t) + (torch.pi - t) * c).clamp(min=0.0) / torch.pi
        A0 = (torch.pi - t) / torch.pi
        flat = torch.full_like(p, float(coef0))
        S1 = torch.where(p > 0, gamma * p * A1 + coef0, flat)
        T = torch.where(p > 0, S1 + gamma * T * A0, flat)
        S = S1
        qx, qy = gamma * qx + coef0, gamma * qy + coef0
    return S if kind == RELU_NNGP else T
