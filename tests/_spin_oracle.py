"""Float64 restatement of SpIN's training step on a kernel operator (reference methods/spin.py:33-38, 41-73, 76-100,
130-193, 209-215) with the COMPACT Jacobian state of neural_svd_amd/spin.py: plain torch, an explicit loop over the
samples for the Jacobians, no torch.func.

Model: the plain WaveFunctions(ParallelMLP(Fourier features)) - phi_c(x) = hard_mul_const * MLP_c([sin(x B), cos(x B)]),
softplus hidden layers, last width 1. Parameters: fB (D, m), ws[i] (L, h_i, h_{i-1}), bs[i] (L, h_i, 1).

State: sigma_avg (L, L), and per trainable tensor (ws.., bs..) one (L_a, *p.shape) array J with
J[a, c, ...] = reference j_avg[a, c, c, ...] - everything else of the reference's (L, L, *p.shape) tensors stays zero,
because head c's output depends on head c's parameters only.
"""
import math

import torch

THRESHOLD = 20.0


def softplus(z):
    return torch.where(z > THRESHOLD, z, torch.log1p(torch.exp(torch.clamp(z, max=THRESHOLD))))


def softplus_grad(z):
    return torch.where(z > THRESHOLD, torch.ones_like(z), torch.sigmoid(z))


def features(x, fB):
    proj = x @ fB
    return torch.cat([torch.sin(proj), torch.cos(proj)], dim=1)  # (B, 2m)


def model_forward(x, fB, ws, bs, c=1.0, keep=False):
    """phi (B, L); keep: also the inputs a_{i-1} (layer 0: (B, F) shared, else (L, h_{i-1}, B)) and pre-activations z_i"""
    feat = features(x, fB)
    h = torch.einsum("lhd,bd->lhb", ws[0], feat) + bs[0]
    ins, zs = [feat], [h]
    for i in range(1, len(ws)):
        a = softplus(h)
        ins.append(a)
        h = torch.einsum("lhp,lpb->lhb", ws[i], a) + bs[i]
        zs.append(h)
    out = c * h[:, 0, :].T  # (B, L); output width 1
    return (out, ins, zs) if keep else out


def jacobian_contraction(x, phi, fB, ws, bs, c=1.0):
    """j_new[a, c, ...] = (2 / B1) sum_b phi[b, a] d phi_c(x_b) / d p, one sample at a time: for sample b the unit-seed
    chain delta_n = hard_mul_const, delta_{i-1} = (W_i^T delta_i) softplus'(z_{i-1}) per head, then
    d phi_c / d W_i = delta_i^c a_{i-1}^c^T and d phi_c / d b_i = delta_i^c. Returns [per ws.., per bs..], each
    (L_a, *p.shape)."""
    B1, L, n = x.shape[0], ws[0].shape[0], len(ws)
    _, ins, zs = model_forward(x, fB, ws, bs, c, keep=True)
    jw = [torch.zeros((L,) + tuple(w.shape), dtype=x.dtype) for w in ws]
    jb = [torch.zeros((L,) + tuple(b.shape), dtype=x.dtype) for b in bs]
    for b in range(B1):
        delta = torch.full((L, 1), float(c), dtype=x.dtype)  # (L, h_n = 1)
        for i in range(n - 1, -1, -1):
            a_prev = ins[0][b].expand(L, -1) if i == 0 else ins[i][:, :, b]  # (L, h_{i-1})
            dW = delta[:, :, None] * a_prev[:, None, :]  # (L_c, h_i, h_{i-1}): d phi_c(x_b) / d W_i[c]
            jw[i] += phi[b][:, None, None, None] * dW[None]
            jb[i] += phi[b][:, None, None, None] * delta[None, :, :, None]
            if i > 0:
                delta = torch.einsum("lhp,lh->lp", ws[i], delta) * softplus_grad(zs[i - 1][:, :, b])
    return [2.0 * j / B1 for j in jw] + [2.0 * j / B1 for j in jb]


def jacobian_contraction_einsum(x, phi, fB, ws, bs, c=1.0):
    """the same contraction with the samples batched: one einsum per (layer, tensor). For the larger GPU test shapes;
    tests/test_spin_oracle.py pins it to the per-sample loop above."""
    B1, L, n = x.shape[0], ws[0].shape[0], len(ws)
    _, ins, zs = model_forward(x, fB, ws, bs, c, keep=True)
    jw, jb = [None] * n, [None] * n
    delta = torch.full((L, 1, B1), float(c), dtype=x.dtype)
    for i in range(n - 1, -1, -1):
        if i == 0:
            jw[i] = torch.einsum("ba,chb,bk->achk", phi, delta, ins[0])
        else:
            jw[i] = torch.einsum("ba,chb,ckb->achk", phi, delta, ins[i])
        jb[i] = torch.einsum("ba,chb->ach", phi, delta)[..., None]
        if i > 0:
            delta = torch.einsum("chp,chb->cpb", ws[i], delta) * softplus_grad(zs[i - 1])
    return [2.0 * j / B1 for j in jw] + [2.0 * j / B1 for j in jb]


def jacobian_contraction_abs(x, phi, fB, ws, bs, c=1.0):
    """A[a, c, ...] = (2 / B1) sum_b |phi[b, a]| |delta_i^c(x_b)| |a_{i-1}^c(x_b)|: jacobian_contraction_einsum with every
    factor of the sum over the samples replaced by its absolute value (the deltas and activations themselves are the
    signed ones), so every element bounds the sum of the absolute terms of the same element of j_new - the scale a
    float32 rounding error of that element is relative to, however much the signed terms cancel."""
    B1, L, n = x.shape[0], ws[0].shape[0], len(ws)
    _, ins, zs = model_forward(x, fB, ws, bs, c, keep=True)
    aw, ab = [None] * n, [None] * n
    delta = torch.full((L, 1, B1), float(c), dtype=x.dtype)
    pa = phi.abs()
    for i in range(n - 1, -1, -1):
        if i == 0:
            aw[i] = torch.einsum("ba,chb,bk->achk", pa, delta.abs(), ins[0].abs())
        else:
            aw[i] = torch.einsum("ba,chb,ckb->achk", pa, delta.abs(), ins[i].abs())
        ab[i] = torch.einsum("ba,chb->ach", pa, delta.abs())[..., None]
        if i > 0:
            delta = torch.einsum("chp,chb->cpb", ws[i], delta) * softplus_grad(zs[i - 1])
    return [2.0 * j / B1 for j in aw] + [2.0 * j / B1 for j in ab]


def spin_solve(sigma_avg, pi):
    """steps 3-5: chol, Ci, Lambda, eigvals, loss, gsigma, gpi"""
    L = sigma_avg.shape[0]
    chol = torch.linalg.cholesky(sigma_avg + 1e-3 * torch.eye(L, dtype=sigma_avg.dtype))
    Ci = torch.linalg.inv(chol)
    Lam = Ci @ pi @ Ci.T
    dl = torch.diag(torch.diagonal(Ci))
    gsigma = Ci.T @ torch.triu(Lam @ dl)
    gpi = -Ci.T @ dl
    return dict(chol=chol, Ci=Ci, Lambda=Lam, eigvals=torch.diagonal(Lam).clone(), loss=torch.trace(Lam), gsigma=gsigma,
                gpi=gpi)


class SpinOracle:
    """kernel(a, b) -> (len(a), len(b)) float64 matrix of a symmetric kernel. ``step`` returns the quantities of one
    compute_loss_kernel + backward and updates the state (sigma_avg, J)."""

    def __init__(self, fB, ws, bs, decay, kernel, c=1.0, contraction=None):
        # contraction: jacobian_contraction (the per-sample loop, default) or jacobian_contraction_einsum (the same
        # numbers with the samples batched: for the wide cases, where the loop takes tens of seconds)
        self.contraction = contraction or jacobian_contraction
        self.fB = fB.double()
        self.ws = [w.double().clone() for w in ws]
        self.bs = [b.double().clone() for b in bs]
        self.decay, self.kernel, self.c = float(decay), kernel, float(c)
        L = self.ws[0].shape[0]
        self.sigma_avg = torch.zeros((L, L), dtype=torch.float64)
        self.J = [torch.zeros((L,) + tuple(p.shape), dtype=torch.float64) for p in self.ws + self.bs]

    def params(self):
        return self.ws + self.bs

    def step(self, x, split_batch):
        x = x.double()
        B = x.shape[0]
        B1 = (B + 1) // 2 if split_batch else B
        x1, x_ref = (x[:B1], x[B1:]) if split_batch else (x, x)
        B2 = x_ref.shape[0]
        ps = [p.clone().requires_grad_(True) for p in self.params()]
        n = len(self.ws)
        phi_all = model_forward(x, self.fB, ps[:n], ps[n:], self.c)
        phi1 = phi_all[:B1]
        phi_ref = phi_all[B1:] if split_batch else phi_all
        Kphi = self.kernel(x1, x_ref) @ phi_ref / B2
        with torch.no_grad():
            sigma = phi_all.T @ phi_all / B
            pi = phi1.T @ Kphi / B1
            self.sigma_avg = (1.0 - self.decay) * self.sigma_avg + self.decay * sigma
            s = spin_solve(self.sigma_avg, pi)
            cond = torch.linalg.cond(self.sigma_avg + 1e-3 * torch.eye(len(sigma), dtype=torch.float64))
            # term 2
            j_new = self.contraction(x1, phi1, self.fB, self.ws, self.bs, self.c)
            self.J = [(1.0 - self.decay) * jo + self.decay * jn for jo, jn in zip(self.J, j_new)]
            term2 = [torch.einsum("ac,ac...->c...", s["gsigma"], j) for j in self.J]
            # term 1: Covariance.backward's cotangents, then autograd through phi and Kphi
            dphi, dKphi = Kphi @ s["gpi"] / B1, phi1 @ s["gpi"] / B1
        term1 = torch.autograd.grad((dphi * phi1).sum() + (dKphi * Kphi).sum(), ps)
        return dict(loss=s["loss"], eigvals=s["eigvals"], sigma_avg=self.sigma_avg.clone(), chol=s["chol"],
                    gsigma=s["gsigma"], gpi=s["gpi"], phi=phi1.detach(), Kphi=Kphi.detach(), cond=cond,
                    term2=term2, grad=[a + b for a, b in zip(term2, term1)])

    def sgd(self, grads, lr):
        n = len(self.ws)
        self.ws = [w - lr * g for w, g in zip(self.ws, grads[:n])]
        self.bs = [b - lr * g for b, g in zip(self.bs, grads[n:])]

    def expand(self):
        """the reference's dense j_avg tensors (L, L, *p.shape) of the trainable tensors, ws.. then bs.."""
        out = []
        L = self.sigma_avg.shape[0]
        idx = torch.arange(L)
        for j in self.J:
            full = torch.zeros((L,) + tuple(j.shape), dtype=j.dtype)  # (a, c, c', ...)
            full[:, idx, idx] = j
            out.append(full)
        return out


def gaussian_kernel(ell):
    def k(a, b):
        return torch.exp(-torch.cdist(a, b) ** 2 / (2.0 * ell ** 2))
    return k


# ---- what the GPU test modules share ---------------------------------------------------------------------------------
def pack_tensors(H, shape, tensors, fB=None):
    """hip_ops.pack_params of [ws.. | bs..]; H = neural_svd_amd.hip_ops, passed in: this module needs no GPU"""
    n = len(shape.dims)
    return H.pack_params(shape, tensors[:n], tensors[n:], fB, None)


def solve_ref(state64, sigma, pi, decay):
    """the moving average of sigma in float64 and spin_solve on it"""
    s = (1.0 - decay) * state64 + decay * sigma
    return s, spin_solve(s, pi)


# ---- what the golden script and the tests share: sampling of large tensors and the error measure ------------------
SAMPLE_ABOVE = 96


def sample(t):
    """the whole tensor (flattened) up to SAMPLE_ABOVE elements, else about 64 evenly strided elements of it"""
    v = t.reshape(-1)
    if v.numel() <= SAMPLE_ABOVE:
        return v
    return v[::max(v.numel() // 64, 1) | 1]  # (odd stride: walks through every row and column residue)


def rel_err(got, want):
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return float((got - want).norm() / max(float(want.norm()), 1e-300))


def quantity_names(n_tensors):
    """the compared quantities of one step, in the order the fixture packs them (n_tensors = weights + biases)"""
    return (["loss", "eigvals", "sigma_avg", "chol", "phi", "Kphi"] + [f"term2_{i}" for i in range(n_tensors)] +
            [f"grad_{i}" for i in range(n_tensors)])


def unpack_step(z, name, split, it):
    """{quantity: (float64 sample, float32 reference's error on it)} and cond of one recorded step: the fixture keeps
    the samples of a step back to back in `vals` with their lengths in `sizes`"""
    p = f"{name}_s{int(split)}_k{it}_"
    vals, sizes, err = torch.from_numpy(z[p + "vals"]), z[p + "sizes"], z[p + "err32"]
    names = quantity_names(2 * (len(CASES[name]["hidden"]) + 1))
    assert len(names) == len(sizes) == len(err)
    out, off = {}, 0
    for k, n, e in zip(names, sizes, err):
        out[k] = (vals[off:off + int(n)], float(e))
        off += int(n)
    return out, float(z[p + "cond"])


def bound(err32):
    """the tolerance of a compared quantity: max(1e-4, 4 x the float32 reference's error on it)"""
    return max(1e-4, 4.0 * float(err32))


CASES = dict(
    # name: L, m, hidden, B, D, decay, c = hard_mul_const (the wide cases scale the outputs down to keep
    # cond(sigma_avg + 1e-3 I) under COND_MAX)
    t3=dict(L=3, m=4, hidden=(6, 5), B=10, D=2, decay=0.3),
    a=dict(L=4, m=8, hidden=(16, 16), B=24, D=2, decay=0.01),
    b=dict(L=5, m=64, hidden=(128, 128), B=64, D=3, decay=0.01),
    b1=dict(L=5, m=64, hidden=(128, 128), B=64, D=3, decay=1.0),
    c=dict(L=16, m=8, hidden=(16, 16), B=40, D=2, decay=0.01, c=0.5),
    d=dict(L=64, m=8, hidden=(16,), B=96, D=4, decay=0.01, c=0.25),
    o=dict(L=5, m=8, hidden=(16, 24), B=33, D=3, decay=1.0),
)
ELL, LR, NSTEPS, FOURIER_SCALE, X_SCALE = 1.5, 0.01, 3, 0.3, 1.5
COND_MAX = 5e3
STORE_PARAMS_UP_TO = 20000  # larger models are rebuilt from their seed (init_params)


def case_c(name):
    return float(CASES[name].get("c", 1.0))


def case_seed(name):
    return 300 + sorted(CASES).index(name)


def init_params(L, D, m, hidden, seed):
    """the reference's draw order under torch.manual_seed(seed): Fourier _B, then per layer W ~ sqrt(2 / fan_in) randn,
    b = 0 (examples/utils.py:116-119, examples/models/mlp.py:185-189)"""
    torch.manual_seed(seed)
    fB = 2 * torch.pi * FOURIER_SCALE * torch.randn((D, m)).float()
    ws, bs, prev = [], [], 2 * m
    for h in list(hidden) + [1]:
        ws.append(math.sqrt(2.0 / prev) * torch.randn(L, h, prev))
        bs.append(torch.zeros(L, h, 1))
        prev = h
    return fB, ws, bs


def load_case(z, name):
    """(fB, ws, bs, xs (NSTEPS, B, D)) float32 of a golden case"""
    cs = CASES[name]
    n = len(cs["hidden"]) + 1
    if f"{name}_fB" in z.files:
        fB = torch.from_numpy(z[f"{name}_fB"])
        ws = [torch.from_numpy(z[f"{name}_w{i}"]) for i in range(n)]
        bs = [torch.from_numpy(z[f"{name}_b{i}"]) for i in range(n)]
    else:
        fB, ws, bs = init_params(cs["L"], cs["D"], cs["m"], cs["hidden"], case_seed(name))
    return fB, ws, bs, torch.from_numpy(z[f"{name}_x"])
