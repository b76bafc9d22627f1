"""Float64 restatement of NeuralEF's training step on a kernel operator (reference methods/neuralef.py:13-62, 117-137 over
methods/utils.py:36-68) in the form neural_svd_amd/neuralef.py:NefKernelTrainer runs: plain torch, ONE model evaluation
on all rows, the batch normalisation per segment with its hand-derived reverse mode, no torch.func.

u = model(x) on all B rows; segments: one ([0, B)) or, with split_batch, the two chunks [0, B1) and [B1, B):
    n_h[l] = ||u_h[:, l]|| / sqrt(B_h),  phi = u / n_h by segment
    Kphi = k(x, x) phi / B, or split: Kphi[:B1] = k(x1, x2) phi2 / B2, Kphi[B1:] = k(x2, x1) phi1 / B1
    loss = NeuralEigenfunctionsLossFunction(phi, Kphi, phi1, Kphi1, phi2, Kphi2) with phi1 = phi2 = phi when not split
    g = d loss / d phi as that function's backward returns it (4 variance + 2 align_1 + 2 align_2 by rows; nothing
        reaches Kphi), du = (g - phi s_h) / n_h with s_h[l] = mean over the segment's rows of g phi
The running norms are updated in the order the operator callable evaluates the model: model(x) first, model(x_ref) only
when x_ref is another batch - segment 0 once, or with split_batch segments 0, 1, 1, 0 (``order``); the first update ever
is a copy, then biased m r + (1 - m) n, unbiased sqrt(m r^2 + (1 - m) n^2).
"""
import torch

from tests._spin_oracle import (FOURIER_SCALE, ELL, LR, X_SCALE, STORE_PARAMS_UP_TO, bound, gaussian_kernel,  # noqa: F401
                                init_params, model_forward, rel_err, sample)
from tests._spinx_oracle import CASES as SHAPES

NSTEPS = 3
MOMENTUM = 0.9           # BatchL2NormalizedFunctions' default, which NeuralEigenfunctions never overrides
NORM_RATIO_MIN = 0.05    # admission: min_l n / max_l n within every segment, at every recorded step
DIAG_RATIO_MIN = 1e-3    # admission (unbiased=False): min_i |Q_ii + 1e-5| / max_i |Q_ii| of both halves' Q

# the variants recorded per shape: (tag, unbiased, batchnorm_mode, include_diag); each in both split_batch modes
MAIN_VARIANTS = (("b0", False, "unbiased", False), ("b1", True, "unbiased", False))
EXTRA_VARIANTS = (("biased", False, "biased", False), ("none", False, "none", False), ("diag", False, "unbiased", True))
EXTRA_SHAPE = "a"


def variants(name):
    return MAIN_VARIANTS + (EXTRA_VARIANTS if name == EXTRA_SHAPE else ())


def case_c(name):
    return float(SHAPES[name]["c"])


def case_seed(name):
    # (shape d: its place in the row, 903, fails the diagonal admission at the second step of the split run - 8.1e-4)
    return 906 if name == "d" else 900 + sorted(SHAPES).index(name)


def chunk_rows(B, split):
    B1 = (B + 1) // 2 if split else B
    return B1, (B - B1 if split else B)


def update_order(split):
    """segment indices in the order the running norms see them in one step"""
    return (0, 1, 1, 0) if split else (0,)


# ---- the pieces ------------------------------------------------------------------------------------------------------
def segment_norms(u, B1):
    """(2, L): n_1 | n_2 (one segment: n_1 twice)"""
    B = u.shape[0]
    n1 = u[:B1].norm(dim=0) / B1 ** 0.5
    n2 = u[B1:].norm(dim=0) / (B - B1) ** 0.5 if B1 < B else n1
    return torch.stack([n1, n2])


def normalize(u, B1):
    """(phi, stats)"""
    stats = segment_norms(u, B1)
    return torch.cat([u[:B1] / stats[0], u[B1:] / stats[1]]), stats


def normalize_backward(phi, stats, B1, g):
    """du = (g - phi s_h) / n_h, the hand-written reverse mode of u -> u / n(u) per segment; stats None: du = g"""
    if stats is None:
        return g.clone()
    out = torch.empty_like(g)
    for h, rows in enumerate((slice(0, B1), slice(B1, None))):
        if phi[rows].shape[0]:
            s = (g[rows] * phi[rows]).mean(0)
            out[rows] = (g[rows] - phi[rows] * s) / stats[h]
    return out


def running_update(state, n, momentum=MOMENTUM):
    """one BatchL2NormalizedFunctions.update_norm on state = dict(biased, unbiased, initialized)"""
    if not state["initialized"]:
        state.update(biased=n.clone(), unbiased=n.clone(), initialized=True)
    else:
        state["biased"] = momentum * state["biased"] + (1 - momentum) * n
        state["unbiased"] = torch.sqrt(momentum * state["unbiased"] ** 2 + (1 - momentum) * n ** 2)


def gram(f, Tf):
    return f.T @ Tf / f.shape[0]


def coefficients(phi1, K1, phi2, K2, unbiased, diagonal):
    """(coeff_1, coeff_2) of methods/neuralef.py:38-49"""
    if unbiased:
        return gram(phi1, phi1).triu(diagonal), gram(phi2, phi2).triu(diagonal)
    Q1, Q2 = gram(phi1, K1), gram(phi2, K2)
    return (Q2.triu(diagonal) / (Q2.diag() + 1e-5).view(-1, 1), Q1.triu(diagonal) / (Q1.diag() + 1e-5).view(-1, 1))


def loss_and_grads(phi, Kphi, phi1, K1, phi2, K2, unbiased, diagonal):
    """(loss, dphi, dphi1, dphi2): the value and the three gradients NeuralEigenfunctionsLossFunction returns"""
    var = -Kphi / phi.shape[0]
    c1, c2 = coefficients(phi1, K1, phi2, K2, unbiased, diagonal)
    a1, a2 = K1 @ c1 / phi1.shape[0], K2 @ c2 / phi2.shape[0]
    loss = (phi * var).sum() + 0.5 * ((phi1 * a1).sum() + (phi2 * a2).sum())
    return loss, 4 * var, 2 * a1, 2 * a2


# ---- one full step ---------------------------------------------------------------------------------------------------
class NefOracle:
    """kernel(a, b) -> (len(a), len(b)) float64 matrix of a symmetric kernel. ``step`` returns the quantities of one
    compute_loss_kernel + backward and updates the running norms; ``updates`` logs the segment of every update."""

    def __init__(self, fB, ws, bs, kernel, c=1.0, unbiased=False, mode="unbiased", include_diag=False):
        self.fB = fB.double()
        self.ws = [w.double().clone() for w in ws]
        self.bs = [b.double().clone() for b in bs]
        self.kernel, self.c = kernel, float(c)
        self.unbiased, self.mode, self.diagonal = bool(unbiased), mode, 0 if include_diag else 1
        L = self.ws[0].shape[0]
        self.state = dict(biased=torch.ones(L, dtype=torch.float64), unbiased=torch.ones(L, dtype=torch.float64),
                          initialized=False)
        self.updates = []

    def params(self):
        return self.ws + self.bs

    def step(self, x, split_batch):
        x = x.double()
        B = x.shape[0]
        B1, B2 = chunk_rows(B, split_batch)
        ps = [p.clone().requires_grad_(True) for p in self.params()]
        n = len(self.ws)
        u = model_forward(x, self.fB, ps[:n], ps[n:], self.c)
        with torch.no_grad():
            ud = u.detach()
            if self.mode == "none":
                phi, stats = ud, None
            else:
                phi, stats = normalize(ud, B1)
                for h in update_order(split_batch):
                    running_update(self.state, stats[h])
                    self.updates.append(h)
            if split_batch:
                Kx = self.kernel(x[:B1], x[B1:])
                Kphi = torch.cat([Kx @ phi[B1:] / B2, Kx.T @ phi[:B1] / B1])
                loss, g, g1, g2 = loss_and_grads(phi, Kphi, phi[:B1], Kphi[:B1], phi[B1:], Kphi[B1:], self.unbiased,
                                                 self.diagonal)
                g = g + torch.cat([g1, g2])
            else:
                Kphi = self.kernel(x, x) @ phi / B
                loss, g, g1, g2 = loss_and_grads(phi, Kphi, phi, Kphi, phi, Kphi, self.unbiased, self.diagonal)
                g = g + g1 + g2
            du = normalize_backward(phi, stats, B1, g)
        grad = torch.autograd.grad((du * u).sum(), ps)
        return dict(loss=loss, phi=phi, Kphi=Kphi, grad=list(grad), norm_biased=self.state["biased"].clone(),
                    norm_unbiased=self.state["unbiased"].clone(), stats=stats, g=g, du=du)

    def sgd(self, grads, lr):
        n = len(self.ws)
        self.ws = [w - lr * g for w, g in zip(self.ws, grads[:n])]
        self.bs = [b - lr * g for b, g in zip(self.bs, grads[n:])]


def admission(phi, Kphi, stats, B1, split, unbiased):
    """(norm ratio, diagonal ratio) of one step: min_l n / max_l n over the segments (1.0 without batch norms), and for
    unbiased=False min_i |Q_ii + 1e-5| / max_i |Q_ii| over the two halves' Q (inf otherwise)"""
    nr = 1.0 if stats is None else min(float(s.min() / s.max()) for s in (stats if split else stats[:1]))
    dr = float("inf")
    if not unbiased:
        halves = ((phi[:B1], Kphi[:B1]), (phi[B1:], Kphi[B1:])) if split else ((phi, Kphi),)
        for p, k in halves:
            q = gram(p, k).diag()
            dr = min(dr, float((q + 1e-5).abs().min() / q.abs().max()))
    return nr, dr


# ---- the fixture's layout ----------------------------------------------------------------------------------------------
def quantity_names(n_tensors):
    return ["loss", "phi", "Kphi", "norm_biased", "norm_unbiased"] + [f"grad_{i}" for i in range(n_tensors)]


def flat(res):
    q = {k: res[k] for k in ("loss", "phi", "Kphi", "norm_biased", "norm_unbiased")}
    for i, g in enumerate(res["grad"]):
        q[f"grad_{i}"] = g
    return q


def prefix(name, tag, split, it):
    return f"{name}_{tag}_s{int(split)}_k{it}_"


def unpack_step(z, name, tag, split, it):
    """{quantity: (float64 sample, float32 reference's error on it)} of one recorded step"""
    p = prefix(name, tag, split, it)
    vals, sizes, err = torch.from_numpy(z[p + "vals"]), z[p + "sizes"], z[p + "err32"]
    names = quantity_names(2 * (len(SHAPES[name]["hidden"]) + 1))
    assert len(names) == len(sizes) == len(err)
    out, off = {}, 0
    for k, n, e in zip(names, sizes, err):
        out[k] = (vals[off:off + int(n)], float(e))
        off += int(n)
    return out


def load_case(z, name):
    """(fB, ws, bs, xs (NSTEPS, B, D)) float32 of a golden shape"""
    cs = SHAPES[name]
    n = len(cs["hidden"]) + 1
    if f"{name}_fB" in z.files:
        fB = torch.from_numpy(z[f"{name}_fB"])
        ws = [torch.from_numpy(z[f"{name}_w{i}"]) for i in range(n)]
        bs = [torch.from_numpy(z[f"{name}_b{i}"]) for i in range(n)]
    else:
        fB, ws, bs = init_params(cs["L"], cs["D"], cs["m"], cs["hidden"], case_seed(name))
    return fB, ws, bs, torch.from_numpy(z[f"{name}_x"])
