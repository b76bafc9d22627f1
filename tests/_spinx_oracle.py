"""Float64 restatement of SpINx's training step on a kernel operator (reference methods/spinx.py:13-23, 92-99, 114-132,
148-169) in the MOMENT form neural_svd_amd/spinx.py runs: plain torch, hand-derived cotangents, no torch.func.

P = phi on the B1 rows that carry K = Kphi, Phi = phi on all B rows:
    S = Phi^T Phi / B, Gpp = P^T P / B1, Gpk = P^T K / B1 (= pi), Gkk = K^T K / B1
    A = cholesky(S + 1e-3 I)^-1 with rows a_l; lambda_l = a_l^T Gpk a_l, qk_l = a_l^T Gkk a_l, qp_l = a_l^T Gpp a_l
    losses = [sum_l tw_l lambda_l | r_l = qk_l - lambda_l^2 (2 - qp_l)],  loss = sum_k w_k losses_k / L
r_l is mean_b (K a_l - lambda_l P a_l)^2 expanded: its cross term a_l^T (K^T P / B1) a_l is lambda_l itself.
State: sigma_avg <- (1 - decay) sigma_avg + decay S from zeros (no bias correction), chol = cholesky(sigma_avg + 1e-3 I);
the loss factors the BATCH S, the state is only what forward() whitens with.
NTK weights over the TRAINABLE tensors (ws, bs): ntk_k = sum ||d losses_k / d p||^2, weights = sqrt(sum(ntk) / ntk).
"""
import torch

from tests._spin_oracle import (FOURIER_SCALE, ELL, LR, X_SCALE, STORE_PARAMS_UP_TO, bound, gaussian_kernel,  # noqa: F401
                                init_params, model_forward, rel_err, sample)

NSTEPS = 3          # steps with uniform weights; one more (index NSTEPS) runs with nonuniform_weights
COND_MAX = 1e3      # of the batch sigma + 1e-3 I at every recorded step

CASES = dict(
    # name: L, m, hidden, B, D, decay, c = hard_mul_const (scales the outputs: the batch sigma stays well conditioned)
    t3=dict(L=3, m=4, hidden=(6, 5), B=10, D=2, decay=0.3, c=1.0),
    a=dict(L=4, m=8, hidden=(16, 16), B=24, D=2, decay=0.01, c=1.0),
    b=dict(L=5, m=64, hidden=(128, 128), B=64, D=3, decay=1.0, c=1.0),
    o=dict(L=5, m=8, hidden=(16, 24), B=33, D=3, decay=0.01, c=1.0),
    c=dict(L=16, m=8, hidden=(16, 16), B=40, D=2, decay=0.01, c=0.1),
    d=dict(L=64, m=8, hidden=(16,), B=96, D=4, decay=0.01, c=0.05),
)


def case_c(name):
    return float(CASES[name]["c"])


def case_seed(name):
    return 700 + sorted(CASES).index(name)


def nonuniform_weights(L):
    """the weights of the fourth recorded step: L + 1 distinct-ish values in [0.5, 1.4]"""
    return 0.5 + ((torch.arange(L + 1, dtype=torch.float64) * 7) % 10) / 10.0


def chunk_rows(B, split):
    B1 = (B + 1) // 2 if split else B
    return B1, (B - B1 if split else B)


# ---- the loss: moment form and direct form ---------------------------------------------------------------------------
def moments(P, K, Phi):
    B, B1 = Phi.shape[0], P.shape[0]
    return Phi.T @ Phi / B, P.T @ P / B1, P.T @ K / B1, K.T @ K / B1


def whitener(S):
    L = S.shape[0]
    C = torch.linalg.cholesky(S + 1e-3 * torch.eye(L, dtype=S.dtype))
    return C, torch.linalg.solve_triangular(C, torch.eye(L, dtype=S.dtype), upper=False)


def losses_moment(S, Gpp, Gpk, Gkk, tw=None):
    """(losses (L + 1), lambda, qk, qp, A) from the four moments"""
    _, A = whitener(S)
    lam = torch.einsum("li,ij,lj->l", A, Gpk, A)
    qk = torch.einsum("li,ij,lj->l", A, Gkk, A)
    qp = torch.einsum("li,ij,lj->l", A, Gpp, A)
    tw = torch.ones_like(lam) if tw is None else tw
    return torch.cat([(tw * lam).sum()[None], qk - lam ** 2 * (2.0 - qp)]), lam, qk, qp, A


def losses_direct(P, K, Phi, tw=None):
    """the same losses from the tall matrices: whitened residuals K A^T - (P A^T) diag(lambda), squared, column means"""
    S = Phi.T @ Phi / Phi.shape[0]
    _, A = whitener(S)
    lam = torch.diagonal(A @ (P.T @ K / P.shape[0]) @ A.T)
    tw = torch.ones_like(lam) if tw is None else tw
    res = K @ A.T - (P @ A.T) * lam[None, :]
    return torch.cat([(tw * lam).sum()[None], (res ** 2).mean(0)])


def solve(S, Gpp, Gpk, Gkk, w, tw=None):
    """the loss and the hand-derived cotangents of the four moments (what nsvd_spinx_solve computes)"""
    L = S.shape[0]
    losses, lam, qk, qp, A = losses_moment(S, Gpp, Gpk, Gkk, tw)
    tw = torch.ones_like(lam) if tw is None else tw
    w0, wl = w[0], w[1:]
    u, v, c = wl / L, wl * lam ** 2 / L, (w0 * tw - 2.0 * wl * lam * (2.0 - qp)) / L
    Gkk_bar, Gpp_bar, Gpk_bar = A.T @ (u[:, None] * A), A.T @ (v[:, None] * A), A.T @ (c[:, None] * A)
    A_bar = torch.tril(u[:, None] * (A @ (Gkk + Gkk.T)) + v[:, None] * (A @ (Gpp + Gpp.T)) + c[:, None] * (A @ (Gpk + Gpk.T)))
    C, _ = whitener(S)
    C_bar = -torch.tril(A.T @ A_bar @ A.T)
    M = torch.tril(C.T @ C_bar)
    M = M - 0.5 * torch.diag(torch.diagonal(M))
    X = A.T @ M @ A
    S_bar = 0.5 * (X + X.T)
    return dict(loss=(losses * w).sum() / L, losses=losses, eigvals=lam, S_bar=S_bar, Gpp_bar=Gpp_bar, Gpk_bar=Gpk_bar,
                Gkk_bar=Gkk_bar, A=A, C=C)


def rotations(sol, B, B1):
    """the five matrices of the tall products: dP = P T_pp + K T_kp, dK = P T_pk + K T_kk, dPhi = Phi T_s"""
    T_s = (sol["S_bar"] + sol["S_bar"].T) / B
    return dict(T_s=T_s, T_pp=(sol["Gpp_bar"] + sol["Gpp_bar"].T) / B1 + T_s, T_kp=sol["Gpk_bar"].T / B1,
                T_pk=sol["Gpk_bar"] / B1, T_kk=(sol["Gkk_bar"] + sol["Gkk_bar"].T) / B1)


def solve_ref(S_raw, s_scale, Gpp_raw, Gpk_raw, Gkk_raw, g_scale, w, tw, state64, decay):
    """nsvd_spinx_solve in float64: (out64, T's dict, new sigma_avg, chol, cond of the batch matrix)"""
    S, Gpp, Gpk, Gkk = s_scale * S_raw, g_scale * Gpp_raw, g_scale * Gpk_raw, g_scale * Gkk_raw
    sol = solve(S, Gpp, Gpk, Gkk, w, tw)
    T = rotations(sol, 1.0 / s_scale, 1.0 / g_scale)
    new = (1.0 - decay) * state64 + decay * S
    L = S.shape[0]
    eye = 1e-3 * torch.eye(L, dtype=torch.float64)
    chol = torch.linalg.cholesky(new + eye)
    out64 = torch.cat([sol["loss"][None], sol["losses"], sol["eigvals"]])
    return out64, T, new, chol, float(torch.linalg.cond(S + eye))


# ---- one full step ---------------------------------------------------------------------------------------------------
class SpinxOracle:
    """kernel(a, b) -> (len(a), len(b)) float64 matrix of a symmetric kernel. ``step`` returns the quantities of one
    compute_loss_kernel + backward and updates the state; ``ntk_weights`` is update_weights_kernel."""

    def __init__(self, fB, ws, bs, decay, kernel, c=1.0):
        self.fB = fB.double()
        self.ws = [w.double().clone() for w in ws]
        self.bs = [b.double().clone() for b in bs]
        self.decay, self.kernel, self.c = float(decay), kernel, float(c)
        L = self.ws[0].shape[0]
        self.L = L
        self.sigma_avg = torch.zeros((L, L), dtype=torch.float64)
        self.chol = torch.zeros((L, L), dtype=torch.float64)
        self.weights = torch.ones(L + 1, dtype=torch.float64)

    def params(self):
        return self.ws + self.bs

    def _tall(self, x, split_batch, ps):
        x = x.double()
        B = x.shape[0]
        B1, B2 = chunk_rows(B, split_batch)
        x1, x_ref = (x[:B1], x[B1:]) if split_batch else (x, x)
        n = len(self.ws)
        Phi = model_forward(x, self.fB, ps[:n], ps[n:], self.c)
        P = Phi[:B1]
        K = self.kernel(x1, x_ref) @ (Phi[B1:] if split_batch else Phi) / B2
        return Phi, P, K

    def _grads(self, Phi, P, K, ps, w):
        """the hand-derived cotangents of the tall matrices, then autograd through the model and the kernel product"""
        B, B1 = Phi.shape[0], P.shape[0]
        with torch.no_grad():
            sol = solve(*moments(P, K, Phi), w)
            T = rotations(sol, B, B1)
            dK = P @ T["T_pk"] + K @ T["T_kk"]
            dPhi = Phi @ T["T_s"]
            dPhi[:B1] = P @ T["T_pp"] + K @ T["T_kp"]
        return sol, torch.autograd.grad((dPhi * Phi).sum() + (dK * K).sum(), ps, retain_graph=True)

    def step(self, x, split_batch):
        ps = [p.clone().requires_grad_(True) for p in self.params()]
        Phi, P, K = self._tall(x, split_batch, ps)
        sol, grad = self._grads(Phi, P, K, ps, self.weights)
        with torch.no_grad():
            S = Phi.T @ Phi / Phi.shape[0]
            eye = 1e-3 * torch.eye(self.L, dtype=torch.float64)
            cond = torch.linalg.cond(S + eye)
            self.sigma_avg = (1.0 - self.decay) * self.sigma_avg + self.decay * S
            self.chol = torch.linalg.cholesky(self.sigma_avg + eye)
        return dict(loss=sol["loss"], losses=sol["losses"], eigvals=sol["eigvals"], phi=P.detach(), Kphi=K.detach(),
                    sigma_avg=self.sigma_avg.clone(), chol=self.chol.clone(), grad=list(grad), cond=cond)

    def ntk_weights(self, x, split_batch):
        """weights = sqrt(sum(ntk) / ntk), ntk_k = squared norm of d losses_k / d (ws, bs); sets and returns them"""
        ps = [p.clone().requires_grad_(True) for p in self.params()]
        Phi, P, K = self._tall(x, split_batch, ps)
        L = self.L
        ntk = torch.zeros(L + 1, dtype=torch.float64)
        for k in range(L + 1):
            e = torch.zeros(L + 1, dtype=torch.float64)
            e[k] = float(L)  # loss = sum_k w_k losses_k / L: w = L e_k picks losses_k
            _, g = self._grads(Phi, P, K, ps, e)
            ntk[k] = sum(float((t ** 2).sum()) for t in g)
        self.weights = torch.sqrt(ntk.sum() / ntk)
        return self.weights.clone()

    def sgd(self, grads, lr):
        n = len(self.ws)
        self.ws = [w - lr * g for w, g in zip(self.ws, grads[:n])]
        self.bs = [b - lr * g for b, g in zip(self.bs, grads[n:])]


# ---- the fixture's layout ----------------------------------------------------------------------------------------------
def quantity_names(n_tensors):
    return ["loss", "phi", "Kphi", "sigma_avg", "chol"] + [f"grad_{i}" for i in range(n_tensors)]


def flat(res):
    q = {k: res[k] for k in ("loss", "phi", "Kphi", "sigma_avg", "chol")}
    for i, g in enumerate(res["grad"]):
        q[f"grad_{i}"] = g
    return q


def unpack_step(z, name, split, it):
    """{quantity: (float64 sample, float32 reference's error on it)} and cond of one recorded step"""
    p = f"{name}_s{int(split)}_k{it}_"
    vals, sizes, err = torch.from_numpy(z[p + "vals"]), z[p + "sizes"], z[p + "err32"]
    names = quantity_names(2 * (len(CASES[name]["hidden"]) + 1))
    assert len(names) == len(sizes) == len(err)
    out, off = {}, 0
    for k, n, e in zip(names, sizes, err):
        out[k] = (vals[off:off + int(n)], float(e))
        off += int(n)
    return out, float(z[p + "cond"])


def unpack_weights(z, name, split):
    """(weights (L + 1) float64, float32 reference's error) recorded after the last step"""
    p = f"{name}_s{int(split)}_weights"
    return torch.from_numpy(z[p]), float(z[p + "_err32"])


def load_case(z, name):
    """(fB, ws, bs, xs (NSTEPS + 1, B, D)) float32 of a golden case"""
    cs = CASES[name]
    n = len(cs["hidden"]) + 1
    if f"{name}_fB" in z.files:
        fB = torch.from_numpy(z[f"{name}_fB"])
        ws = [torch.from_numpy(z[f"{name}_w{i}"]) for i in range(n)]
        bs = [torch.from_numpy(z[f"{name}_b{i}"]) for i in range(n)]
    else:
        fB, ws, bs = init_params(cs["L"], cs["D"], cs["m"], cs["hidden"], case_seed(name))
    return fB, ws, bs, torch.from_numpy(z[f"{name}_x"])


def run_case(orc, xs, split):
    """the recorded sequence: NSTEPS steps with unit weights, one with nonuniform_weights, then the weight update on
    the last batch; yields ('step', it, result) and ('weights', None, weights)"""
    for it in range(NSTEPS + 1):
        if it == NSTEPS:
            orc.weights = nonuniform_weights(orc.L)
        res = orc.step(xs[it], split)
        yield "step", it, res
        orc.sgd(res["grad"], LR)
    yield "weights", None, orc.ntk_weights(xs[NSTEPS], split)
