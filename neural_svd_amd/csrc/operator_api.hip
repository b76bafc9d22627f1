// extern "C" entry points for the operator forward / backward: argument validation, workspace
// carving, and the choice between the fused MFMA kernels (pmlp_fwd.hip, pmlp_bwd.hip) and the generic
// layer-by-layer path implemented here on top of gemm_generic.hip / fd_epilogue.hip.
#include <stdlib.h>
#include <string.h>
#include "nsvd_kernels.h"
#include "evd_math.h"
#include "opt_math.h"

static thread_local hipEvent_t g_prof_start = nullptr;
static thread_local hipEvent_t g_prof_stop = nullptr;

void nsvd_prof_begin(hipStream_t s) {
    if (g_prof_start) (void)hipEventRecord(g_prof_start, s);
    g_prof_start = nullptr;
}
void nsvd_prof_end(hipStream_t s) {
    if (g_prof_stop) (void)hipEventRecord(g_prof_stop, s);
    g_prof_stop = nullptr;
}

extern "C" int nsvd_profile_next_forward(void* ev_start, void* ev_stop) {
    g_prof_start = (hipEvent_t)ev_start;
    g_prof_stop = (hipEvent_t)ev_stop;
    return 0;
}

namespace {

struct GenericWs {
    float* phiT;                      // (F, R)
    float* z[NSVD_MAX_LAYERS];        // z[i]: (L, h_i, R) ACTIVATIONS a_i for i < nl-1 ; z[nl-1] = the model output (L, R)
    float* jac;                       // (B, L)
    float* dsc;                       // (B, L)
    float* dz[2];                     // ping-pong (L, hmax, B)
    float* df;                        // (B, L) for nsvd_operator_backward_evd on the generic path
    int R;                            // rows per (head, unit): erows * B, erows = stencil blocks laid out
    size_t bytes;
};

// plain model evaluation (nsvd_model_forward / _backward) has no stencil: any input dimension up to 64
constexpr int MODEL_MAX_D = 64;
// the operator: NSVD_MAX_D input dimensions (above NSVD_SMALL_D in the finite-difference mode on the generic kernels only:
// nsvd_problem_status)
int validate(const nsvd_model_desc* d, int max_d = NSVD_MAX_D) {
    if (!d) return NSVD_EINVAL;
    if (d->L <= 0 || d->D <= 0 || d->m <= 0) return NSVD_EINVAL;
    if (d->nlayers < 1 || d->nlayers > NSVD_MAX_LAYERS) return NSVD_EINVAL;
    for (int i = 0; i < d->nlayers; ++i)
        if (d->dims[i] <= 0) return NSVD_EINVAL;
    if (d->dims[d->nlayers - 1] != 1) return NSVD_EINVAL;
    if (d->box_mask < NSVD_BOX_NONE || d->box_mask > NSVD_BOX_EXP) return NSVD_EINVAL;
    if (d->box_mask != NSVD_BOX_NONE && !(d->box_lim > 0.f)) return NSVD_EINVAL;
    if (d->D > max_d) return NSVD_EUNSUPPORTED;
    return 0;
}

// every operator path implements every potential and importance below; anything else is refused, never ignored
// (the Fokker-Planck kind only inside nsvd_problem_status' conditions: NSVD_EUNSUPPORTED outside them)
// path: NSVD_PATH_GENERIC_EXACT lifts the exact mode's limit of NSVD_SMALL_D input dimensions (nsvd_problem_status)
int validate_problem(const nsvd_model_desc* d, const nsvd_problem* p, int path = NSVD_PATH_AUTO) {
    if (!p) return NSVD_EINVAL;
    return nsvd_problem_status(*d, *p, path);
}

// NSVD_PATH_GENERIC_EXACT: the exact Laplacian on the generic kernels, D + 2 jet blocks per sample instead of the 1 + 2 D
// stencil blocks. Explicit request only; with eps > 0 it cannot be honoured (the Fokker-Planck kind has no exact mode at
// all: nsvd_problem_status refuses it with eps <= 0 on every path).
bool generic_exact(int path) { return path == NSVD_PATH_GENERIC_EXACT; }
int generic_exact_status(const nsvd_problem& p) {
    return (p.eps > 0.f || p.operator_kind != NSVD_OP_SCHROEDINGER) ? NSVD_EUNSUPPORTED : 0;
}
// stencil blocks of the generic layout for `path` (carve's erows; 0 = the 1 + 2 D of the stencil mode)
int generic_erows(const nsvd_model_desc& d, int path) { return generic_exact(path) ? d.D + 2 : 0; }

NsvdSampler make_sampler(const nsvd_problem& prob, unsigned long long seed, unsigned long long offset) {
    NsvdSampler smp;
    memset(&smp, 0, sizeof(smp));
    smp.seed = seed;
    smp.offset = offset;
    smp.sigma = prob.sigma;
    smp.on = 1;
    smp.kind = prob.use_importance;  // the batch is drawn from the density the problem names
    return smp;
}

// erows: stencil blocks the layout holds (1 + 2D for the operator, 1 for plain model evaluation)
GenericWs carve(const nsvd_model_desc& d, int B, void* base, int erows = 0) {
    GenericWs w;
    memset(&w, 0, sizeof(w));
    const size_t E = erows > 0 ? (size_t)erows : 1 + 2 * (size_t)d.D, R = E * B, F = 2 * (size_t)d.m;
    w.R = (int)R;
    NsvdArena a(base);
    w.phiT = a.take(F * R);
    int hmax = 1;
    for (int i = 0; i < d.nlayers; ++i) {
        w.z[i] = a.take((size_t)d.L * d.dims[i] * R);
        if (d.dims[i] > hmax) hmax = d.dims[i];
    }
    w.jac = a.take((size_t)B * d.L);
    w.dsc = a.take((size_t)B * d.L);
    w.dz[0] = a.take((size_t)d.L * hmax * B);
    w.dz[1] = a.take((size_t)d.L * hmax * B);
    w.df = a.take((size_t)B * d.L);
    w.bytes = a.off;
    return w;
}

// exact: the exact-Laplacian mode (prob->eps <= 0), whose D + 2 jet streams fit the MFMA path up to D = 3
bool want_fused(const nsvd_model_desc& d, int B, int path, bool exact = false) {
    // (NSVD_PATH_FUSED and NSVD_PATH_FUSED_BF16X3 both need the MFMA path)
    if (path == NSVD_PATH_GENERIC || path == NSVD_PATH_GENERIC_EXACT) return false;
    // above the small stencil: the split form on explicit request only - NSVD_PATH_AUTO stays on the generic kernels
    // until the two are measured against each other
    if (d.D > NSVD_SMALL_D) return path == NSVD_PATH_FUSED && !exact && nsvd_fused_split_nd_supported(d, B);
    return nsvd_fused_supported(d, B);
}

bool fused_requested(int path) { return path == NSVD_PATH_FUSED || path == NSVD_PATH_FUSED_BF16X3; }

// what every operator entry point ends its validation with: the workspace is big enough and 256-byte aligned, and an
// explicitly fused path on a shape the MFMA kernels do not take is refused, never rerouted. *fused: which kernels run
int resolve_path(const nsvd_model_desc& d, const nsvd_problem& prob, int B, const void* ws, size_t ws_bytes, int path,
                 bool* fused) {
    if (!nsvd_ws_ok(ws, ws_bytes, nsvd_workspace_bytes(&d, B))) return NSVD_EINVAL;
    *fused = want_fused(d, B, path, !(prob.eps > 0.f));
    return fused_requested(path) && !*fused ? NSVD_EUNSUPPORTED : 0;
}

int check_params(const nsvd_model_desc& d, const nsvd_params* p, bool need_fourier) {
    if (!p) return NSVD_EINVAL;
    if (need_fourier && !p->fourier_B) return NSVD_EINVAL;
    for (int i = 0; i < d.nlayers; ++i)
        if (!p->W[i] || !p->b[i]) return NSVD_EINVAL;
    if (d.has_exp_mask && !p->scales) return NSVD_EINVAL;
    return 0;
}

// Fourier map + every ParallelMLP layer for the first `nst` stencil blocks (nst = E: all rows, 1: centre only)
// jets: the nst = D + 2 blocks are the forward-mode jet of the exact mode (generic_jets.hip) instead of the stencil
int generic_mlp(const nsvd_model_desc& d, const nsvd_params& p, const float* x, int B, float eps, int nst,
                const GenericWs& w, hipStream_t s, bool features_ready = false, bool jets = false) {
    const int R = w.R, F = 2 * d.m;
    int rc = 0;
    // all stencil rows: the shifted row blocks in EVEN / ODD form - features, pre-activations and head
    // outputs of block 1 + 2 d / 2 + 2 d are the even / odd perturbations along d; centre rows only (nst = 1): plain
    const bool eo = nst > 1 && !jets;
    if (!features_ready)
        rc = jets ? nsvd_fourier_features_jets(x, p.fourier_B, w.phiT, B, d.D, d.m, R, s) :
             eo ? nsvd_fourier_features_evenodd(x, p.fourier_B, w.phiT, B, d.D, d.m, eps, R, s)
                : nsvd_fourier_features(x, p.fourier_B, w.phiT, B, d.D, d.m, eps, nst, R, s);
    if (rc) return rc;
    int kin = F;
    for (int i = 0; i < d.nlayers; ++i) {
        NsvdGemm g;
        g.batch = d.L;
        g.M = d.dims[i]; g.N = nst * B; g.K = kin;
        g.A = p.W[i]; g.sAm = kin; g.sAk = 1; g.bA = (long)d.dims[i] * kin;
        g.B = (i == 0) ? w.phiT : w.z[i - 1]; g.sBk = R; g.sBn = 1; g.bB = (i == 0) ? 0 : (long)kin * R;
        g.C = w.z[i]; g.sCm = R; g.bC = (long)d.dims[i] * R;
        g.bias = p.b[i]; g.bBias = d.dims[i];
        g.eo_cols = (eo || jets) ? B : 0;  // (jets too: a linear layer maps every stream by itself, the bias joins block 0)
        rc = nsvd_gemm_generic(g, s);
        if (rc) return rc;
        // hidden layers: pre-activations -> activations in place (what the next layer, the weight gradient and the data
        // gradient's sigmoid factor read); the last layer's output stays as it is
        if (i + 1 < d.nlayers) {
            rc = jets ? nsvd_softplus_jets_inplace(w.z[i], (long long)d.L * d.dims[i], B, d.D, s)
                      : nsvd_softplus_inplace(w.z[i], (long)d.L * d.dims[i], B, nst, s);
            if (rc) return rc;
        }
        kin = d.dims[i];
    }
    return 0;
}

int generic_forward(const nsvd_model_desc& d, const nsvd_params& p, const nsvd_problem& prob, const float* x, int B,
                    float* f, float* Tf, void* ws, hipStream_t s, bool features_ready, int path) {
    const bool exact = generic_exact(path);
    const GenericWs w = carve(d, B, ws, generic_erows(d, path));
    const int R = w.R, E = R / B;
    // (bench.py's event bracket: the WHOLE forward - features, every layer, the finite-difference epilogue - as the fused
    // forward kernel is one launch doing all of it; closed on the error path too, or the stop event would stay armed for
    // the next forward)
    nsvd_prof_begin(s);
    int rc = generic_mlp(d, p, x, B, prob.eps, E, w, s, features_ready, exact);
    if (!rc)
        rc = exact ? nsvd_fd_epilogue_exact(w.z[d.nlayers - 1], R, x, d.has_exp_mask ? p.scales : nullptr, prob, B, d.D,
                                            d.L, f, Tf, w.jac, w.dsc, s, nsvd_box_of(d))
                   : nsvd_fd_epilogue(w.z[d.nlayers - 1], R, x, d.has_exp_mask ? p.scales : nullptr, prob, B, d.D, d.L, f,
                                      Tf, w.jac, w.dsc, s, 1, nsvd_box_of(d));
    nsvd_prof_end(s);
    return rc;
}

int generic_backward(const nsvd_model_desc& d, const nsvd_params& p, const float* x, int B, const float* df,
                     const nsvd_params& g, void* ws, hipStream_t s, int erows = 0) {
    (void)x;
    const GenericWs w = carve(d, B, ws, erows);
    const int R = w.R, F = 2 * d.m;
    int cur = 0;
    int rc = nsvd_head_backward(df, w.jac, w.dsc, B, d.L, w.dz[cur], d.has_exp_mask ? g.scales : nullptr, s);
    if (rc) return rc;
    for (int i = d.nlayers - 1; i >= 0; --i) {
        const int hi = d.dims[i];
        const int kin = (i == 0) ? F : d.dims[i - 1];
        // weight gradient: dW_i[l][n][k] = sum_b dz_i[l][n][b] * a_{i-1}[l][k][b]   (w.z[i - 1] holds a_{i-1})
        NsvdGemm wg;
        wg.batch = d.L;
        wg.M = hi; wg.N = kin; wg.K = B;
        wg.A = w.dz[cur]; wg.sAm = B; wg.sAk = 1; wg.bA = (long)hi * B;
        wg.B = (i == 0) ? w.phiT : w.z[i - 1]; wg.sBk = 1; wg.sBn = R; wg.bB = (i == 0) ? 0 : (long)kin * R;
        wg.C = g.W[i]; wg.sCm = kin; wg.bC = (long)hi * kin;
        // bias gradient = row sums of dz_i: inside the weight-gradient launch where the kernel can, its own launch otherwise
        wg.rowsum = g.b[i]; wg.bRowsum = hi;
        bool rowsum_done = false;
        rc = nsvd_gemm_generic(wg, s, &rowsum_done);
        if (rc) return rc;
        if (!rowsum_done) {
            rc = nsvd_rowsum(w.dz[cur], g.b[i], d.L * hi, B, B, s);
            if (rc) return rc;
        }
        if (i > 0) {
            // data gradient: dz_{i-1}[l][k][b] = (sum_n W_i[l][n][k] dz_i[l][n][b]) * sigmoid(z_{i-1}[l][k][b]), the sigmoid
            // from the stored activation (1 - e^-a)
            NsvdGemm dg;
            dg.batch = d.L;
            dg.M = kin; dg.N = B; dg.K = hi;
            dg.A = p.W[i]; dg.sAm = 1; dg.sAk = kin; dg.bA = (long)hi * kin;
            dg.B = w.dz[cur]; dg.sBk = B; dg.sBn = 1; dg.bB = (long)hi * B;
            dg.C = w.dz[cur ^ 1]; dg.sCm = B; dg.bC = (long)kin * B;
            dg.Z = w.z[i - 1]; dg.sZm = R; dg.bZ = (long)kin * R;
            dg.sigmoid_mul = 1;
            rc = nsvd_gemm_generic(dg, s);
            if (rc) return rc;
            cur ^= 1;
        }
    }
    return 0;
}

// What one call of the forward family asks for - nsvd_operator_forward, _features, _sample_features(_dev), _backward -
// and which of the shared checks its entry point takes: the subsets differ, and the differences are part of the
// interface (a call one entry point refuses, another accepts). op_call fills what the entry points share, everything
// else off; op_prologue runs the checks in the one order all of them keep and says which kernels run.
struct OpCall {
    const nsvd_model_desc* desc;
    const nsvd_params* params;
    const nsvd_problem* prob;
    const float* x;
    int B;
    void* ws;
    size_t ws_bytes;
    int path;
    hipStream_t s;
    bool others_ok;           // the entry point's own device pointers (f, Tf; df) are there
    bool judge_problem;       // validate_problem
    bool exact_status_first;  // NSVD_PATH_GENERIC_EXACT is judged before the parameters and the workspace
    bool whole_params;        // check_params on the whole set (otherwise: fourier_B alone)
    const nsvd_params* grads;
    bool need_grads;          // check_params on grads
    bool fused;               // (out) the MFMA kernels run
};

OpCall op_call(const nsvd_model_desc* desc, const nsvd_params* params, const nsvd_problem* prob, const float* x, int B,
               void* ws, size_t ws_bytes, int path, void* stream) {
    OpCall c = OpCall();
    c.desc = desc; c.params = params; c.prob = prob;
    c.x = x; c.B = B;
    c.ws = ws; c.ws_bytes = ws_bytes; c.path = path; c.s = (hipStream_t)stream;
    c.others_ok = true;
    return c;
}

int op_prologue(OpCall& c) {
    int rc = validate(c.desc);
    if (rc) return rc;
    if (!c.prob || !c.x || !c.ws || !c.others_ok || c.B <= 0) return NSVD_EINVAL;
    if (!c.whole_params && (!c.params || !c.params->fourier_B)) return NSVD_EINVAL;
    if (c.judge_problem && (rc = validate_problem(c.desc, c.prob, c.path)) != 0) return rc;
    if (c.exact_status_first && generic_exact(c.path) && (rc = generic_exact_status(*c.prob)) != 0) return rc;
    if (c.whole_params && (rc = check_params(*c.desc, c.params, true)) != 0) return rc;
    if (c.need_grads && (rc = check_params(*c.desc, c.grads, false)) != 0) return rc;
    return resolve_path(*c.desc, *c.prob, c.B, c.ws, c.ws_bytes, c.path, &c.fused);
}

// the features of the generic layout for c.path: the jets generic_forward reads in the exact mode, the even / odd stencil
// rows otherwise (w.R = erows * B columns)
int generic_features(const OpCall& c) {
    const nsvd_model_desc& d = *c.desc;
    const GenericWs w = carve(d, c.B, c.ws, generic_erows(d, c.path));
    if (generic_exact(c.path)) return nsvd_fourier_features_jets(c.x, c.params->fourier_B, w.phiT, c.B, d.D, d.m, w.R, c.s);
    return nsvd_fourier_features_evenodd(c.x, c.params->fourier_B, w.phiT, c.B, d.D, d.m, c.prob->eps, w.R, c.s);
}

}  // namespace

extern "C" int nsvd_abi_version(void) { return NSVD_ABI_VERSION; }

extern "C" const char* nsvd_path_name(const nsvd_model_desc* desc, int B, int path) {
    if (validate(desc) != 0 || B <= 0) return "invalid";
    if (generic_exact(path)) return "generic_exact";
    return want_fused(*desc, B, path) ? "fused_mfma" : "generic";
}

extern "C" int nsvd_step_emits_planes(const nsvd_model_desc* desc, int B, int path) {
    if (validate(desc) != 0 || B <= 0 || path != NSVD_PATH_FUSED_BF16X3) return 0;
    // (the streaming backward never runs the kernel that writes the planes)
    return nsvd_fused_supported(*desc, B) && nsvd_fused_wgrad_slices(*desc, B) == 1 &&
                   nsvd_fused_stream_bwd_slices(*desc, B) == 0 ? 1 : 0;
}

extern "C" const char* nsvd_path_name_for(const nsvd_model_desc* desc, const nsvd_problem* prob, int B, int path) {
    // (more input dimensions than the stencil carries are nsvd_problem_status' to answer: "unsupported")
    if (validate(desc, MODEL_MAX_D) != 0 || B <= 0 || !prob) return "invalid";
    const int st = validate_problem(desc, prob, path);
    if (st) return st == NSVD_EUNSUPPORTED ? "unsupported" : "invalid";
    if (generic_exact(path)) return generic_exact_status(*prob) ? "unsupported" : "generic_exact";
    const bool exact = !(prob->eps > 0.f);
    if (want_fused(*desc, B, path, exact)) return "fused_mfma";
    // (above NSVD_SMALL_D an explicitly fused path has nothing to fall back to: the entry points return NSVD_EUNSUPPORTED)
    if (desc->D > NSVD_SMALL_D && fused_requested(path)) return "unsupported";
    return exact ? "unsupported" : "generic";
}

extern "C" size_t nsvd_model_workspace_bytes(const nsvd_model_desc* desc, int B) {
    if (validate(desc, MODEL_MAX_D) != 0 || B <= 0) return 0;
    const size_t gen = carve(*desc, B, nullptr, 1).bytes;
    const size_t fus = nsvd_fused_model_supported(*desc, B) ? nsvd_fused_workspace_bytes(*desc, B) : 0;
    return gen > fus ? gen : fus;
}

extern "C" size_t nsvd_workspace_bytes(const nsvd_model_desc* desc, int B) {
    if (validate(desc) != 0 || B <= 0) return 0;
    const size_t gen = carve(*desc, B, nullptr).bytes;
    const size_t fus = (nsvd_fused_supported(*desc, B) ||nsvd_fused_split_nd_supported(*desc, B))
                           ? nsvd_fused_workspace_bytes(*desc, B) : 0;
    return gen > fus ? gen : fus;
}

extern "C" int nsvd_operator_forward(const nsvd_model_desc* desc, const nsvd_params* params,
                                     const nsvd_problem* prob, const float* x, int B, float* f, float* Tf, void* ws,
                                     size_t ws_bytes, int save_for_backward, int path, void* stream) {
    OpCall c = op_call(desc, params, prob, x, B, ws, ws_bytes, path, stream);
    c.others_ok = f && Tf;
    c.judge_problem = c.exact_status_first = c.whole_params = true;
    if (const int rc = op_prologue(c)) return rc;
    // eps <= 0 selects the exact Laplacian (reference diff_ops.py:7): forward-mode jets, on the MFMA path or - on
    // explicit request only - on the generic kernels
    if (!(prob->eps > 0.f) && !c.fused && !generic_exact(path)) return NSVD_EUNSUPPORTED;
    const bool ready = (save_for_backward & NSVD_FEATURES_READY) != 0;
    const bool bf3 = path == NSVD_PATH_FUSED_BF16X3;
    const bool planes = (save_for_backward & NSVD_W_PLANES_READY) != 0 && bf3;
    if (c.fused)
        return nsvd_fused_forward(*desc, *params, *prob, x, B, f, Tf, ws,
                                  (save_for_backward & 1 ? NSVD_FWD_SAVE : 0) | (ready ? NSVD_FWD_FEATURES_READY : 0) |
                                      (planes ? NSVD_FWD_PLANES_READY : 0),
                                  c.s, bf3, 0);
    return generic_forward(*desc, *params, *prob, x, B, f, Tf, ws, c.s, ready, path);
}

// NeuralEF (neuralef.hip): the operator forward up to the raw head outputs - (L, ldr) rows e B + b in the even / odd
// stencil form of nsvd_fd_epilogue's `base` - and where the centre backward reads jac / dsc (the caller fills them)
int nsvd_operator_forward_raw(const nsvd_model_desc& d, const nsvd_params& p, const nsvd_problem& prob, const float* x,
                              int B, void* ws, int path, hipStream_t s, NsvdRawOut* out) {
    const bool fused = want_fused(d, B, path, !(prob.eps > 0.f));
    if (fused_requested(path) && !fused) return NSVD_EUNSUPPORTED;
    if (path == NSVD_PATH_FUSED_BF16X3 || !(prob.eps > 0.f)) return NSVD_EUNSUPPORTED;
    if (generic_exact(path)) return NSVD_EUNSUPPORTED;  // (no NeuralEF on the generic jets, and no stencil on that path)
    // the per-point batch norms know neither the box mask nor the uniform density
    if (d.box_mask != NSVD_BOX_NONE || prob.use_importance > NSVD_IMP_GAUSSIAN) return NSVD_EUNSUPPORTED;
    const int R = (1 + 2 * d.D) * B;
    if (fused) {
        const FusedWsView v = nsvd_fused_ws_view(d, B, ws);
        out->raw = v.base_raw;
        out->ldr = R;
        out->jac = v.jac;
        out->dsc = d.has_exp_mask ? v.dsc : nullptr;
        return nsvd_fused_forward(d, p, prob, x, B, nullptr, nullptr, ws, NSVD_FWD_SAVE, s, 0, 1);
    }
    const GenericWs w = carve(d, B, ws);
    out->raw = w.z[d.nlayers - 1];
    out->ldr = w.R;
    out->jac = w.jac;
    out->dsc = d.has_exp_mask ? w.dsc : nullptr;
    nsvd_prof_begin(s);
    const int rc = generic_mlp(d, p, x, B, prob.eps, 1 + 2 * d.D, w, s);
    nsvd_prof_end(s);
    return rc;
}

extern "C" int nsvd_operator_features(const nsvd_model_desc* desc, const nsvd_params* params,
                                      const nsvd_problem* prob, const float* x, int B, void* ws, size_t ws_bytes,
                                      int save_for_backward, int path, void* stream) {
    // (neither the problem nor the rest of the parameter set is judged here: the features read fourier_B and eps alone)
    OpCall c = op_call(desc, params, prob, x, B, ws, ws_bytes, path, stream);
    if (const int rc = op_prologue(c)) return rc;
    if (c.fused) return nsvd_fused_features(*desc, *params, *prob, x, B, ws, save_for_backward & 1, c.s, nullptr, nullptr);
    if (generic_exact(path)) {
        if (const int st = generic_exact_status(*prob)) return st;
    } else if (!(prob->eps > 0.f)) {
        return NSVD_EUNSUPPORTED;
    }
    return generic_features(c);
}

namespace {
int sample_features_impl(const nsvd_model_desc* desc, const nsvd_params* params, const nsvd_problem* prob,
                         unsigned long long seed, unsigned long long offset, const nsvd_step_state* state, float* x,
                         int B, void* ws, size_t ws_bytes, int save_for_backward, int path, void* stream) {
    OpCall c = op_call(desc, params, prob, x, B, ws, ws_bytes, path, stream);
    c.judge_problem = c.exact_status_first = true;
    if (const int rc = op_prologue(c)) return rc;
    NsvdSampler smp = make_sampler(*prob, seed, offset);
    smp.offset_add = state ? (const unsigned long long*)&state->step : nullptr;
    if (c.fused) return nsvd_fused_features(*desc, *params, *prob, x, B, ws, save_for_backward & 1, c.s, &smp, x);
    if (!(prob->eps > 0.f) && !generic_exact(path)) return NSVD_EUNSUPPORTED;
    if (const int rc = nsvd_sample_launch(smp, x, B, desc->D, c.s)) return rc;
    return generic_features(c);
}
}  // namespace

extern "C" int nsvd_operator_sample_features(const nsvd_model_desc* desc, const nsvd_params* params,
                                             const nsvd_problem* prob, unsigned long long seed,
                                             unsigned long long offset, float* x, int B, void* ws, size_t ws_bytes,
                                             int save_for_backward, int path, void* stream) {
    return sample_features_impl(desc, params, prob, seed, offset, nullptr, x, B, ws, ws_bytes, save_for_backward, path,
                                stream);
}

extern "C" int nsvd_operator_sample_features_dev(const nsvd_model_desc* desc, const nsvd_params* params,
                                                 const nsvd_problem* prob, unsigned long long seed,
                                                 unsigned long long offset_base, const nsvd_step_state* state,
                                                 float* x, int B, void* ws, size_t ws_bytes, int save_for_backward,
                                                 int path, void* stream) {
    if (!state || ((uintptr_t)state & 7) != 0) return NSVD_EINVAL;
    return sample_features_impl(desc, params, prob, seed, offset_base, state, x, B, ws, ws_bytes, save_for_backward,
                                path, stream);
}

extern "C" int nsvd_model_forward(const nsvd_model_desc* desc, const nsvd_params* params, const float* x, int B,
                                  float hard_mul_const, float* out, void* ws, size_t ws_bytes, int save_for_backward,
                                  void* stream) {
    // plain model evaluation always takes the generic kernels, on a workspace laid out for the centre rows only
    int rc = validate(desc, MODEL_MAX_D);
    if (rc) return rc;
    if (!x || !out || !ws || B <= 0) return NSVD_EINVAL;
    rc = check_params(*desc, params, true);
    if (rc) return rc;
    if (!nsvd_ws_ok(ws, ws_bytes, nsvd_model_workspace_bytes(desc, B))) return NSVD_EINVAL;
    if (nsvd_fused_model_supported(*desc, B))  // 128-wide hidden layers: the E = 1 instance of the MFMA forward
        return nsvd_fused_model_forward(*desc, *params, x, B, hard_mul_const, out, ws, save_for_backward,
                                        (hipStream_t)stream);
    const GenericWs w = carve(*desc, B, ws, 1);
    const int R = w.R;
    rc = generic_mlp(*desc, *params, x, B, 0.f, 1, w, (hipStream_t)stream);
    if (rc) return rc;
    return nsvd_model_out(w.z[desc->nlayers - 1], R, x, desc->has_exp_mask ? params->scales : nullptr,
                          hard_mul_const, B, desc->D, desc->L, out, save_for_backward ? w.jac : nullptr,
                          (save_for_backward && desc->has_exp_mask) ? w.dsc : nullptr, (hipStream_t)stream,
                          nsvd_box_of(*desc));
}

extern "C" int nsvd_model_backward(const nsvd_model_desc* desc, const nsvd_params* params, const float* x, int B,
                                   const float* dout, const nsvd_params* grads, void* ws, size_t ws_bytes,
                                   void* stream) {
    int rc = validate(desc, MODEL_MAX_D);
    if (rc) return rc;
    if (!x || !dout || !ws || B <= 0) return NSVD_EINVAL;
    rc = check_params(*desc, params, true);
    if (rc) return rc;
    rc = check_params(*desc, grads, false);
    if (rc) return rc;
    if (!nsvd_ws_ok(ws, ws_bytes, nsvd_model_workspace_bytes(desc, B))) return NSVD_EINVAL;
    if (nsvd_fused_model_supported(*desc, B))
        return nsvd_fused_backward(*desc, *params, B, dout, *grads, ws, (hipStream_t)stream);
    return generic_backward(*desc, *params, x, B, dout, *grads, ws, (hipStream_t)stream, 1);
}

extern "C" int nsvd_operator_backward(const nsvd_model_desc* desc, const nsvd_params* params,
                                      const nsvd_problem* prob, const float* x, int B, const float* df,
                                      const nsvd_params* grads, void* ws, size_t ws_bytes, int path, void* stream) {
    // (the problem is not judged here: the backward reads what the forward saved)
    OpCall c = op_call(desc, params, prob, x, B, ws, ws_bytes, path, stream);
    c.others_ok = df != nullptr;
    c.whole_params = true;
    c.grads = grads;
    c.need_grads = true;
    if (const int rc = op_prologue(c)) return rc;
    if (c.fused) return nsvd_fused_backward(*desc, *params, B, df, *grads, ws, c.s);
    if (generic_exact(path) && generic_exact_status(*prob)) return NSVD_EUNSUPPORTED;
    return generic_backward(*desc, *params, x, B, df, *grads, ws, c.s, generic_erows(*desc, path));
}

namespace {
// What one call of the EVD-backward family asks for. evd_call fills what the seven entry points share from their common
// arguments (everything else zero); each entry point then sets only the fields that make it different.
struct EvdCall {
    const nsvd_model_desc* desc;
    const nsvd_params* params;
    const nsvd_problem* prob;
    const float* x;
    int B;
    const float *f, *Tf;  // the loss inputs: f .. loss
    int mask_kind;
    const float *v, *M;
    float* moments;
    int moments_reduced;
    const void* evd_scratch;
    int L_total, l_offset;
    float grad_scale;
    float* loss;
    const nsvd_params* grads;
    void* ws;
    size_t ws_bytes;
    int path;
    void* stream;
    // model_mode: the forward was nsvd_model_forward (plain model evaluation, any input dimension up to 64, no
    // Hamiltonian): prob is null and Tf is whatever operator output the caller computed from f (the kernel-operator path)
    bool model_mode;
    int l_begin, l_count;  // the head window (l_count = 0: every head)
    NsvdNextBatch next;    // next.x set: the next batch rides in this call's chain launch (next_batch)
    int window_of_step, not_last;  // nsvd_fused_backward_evd
    void* ev_after_chain;
    // the optimiser step, where the entry point takes one: its descriptor (one of the two, or neither) and the step the
    // kernels take, which backward_evd converts it into
    const nsvd_rmsprop* rmsprop;
    const nsvd_optimizer* optimizer;
    bool take_step;
    NsvdOptStep opt;
};

EvdCall evd_call(const nsvd_model_desc* desc, const nsvd_params* params, const nsvd_problem* prob, const float* x, int B,
                 const float* f, const float* Tf, int mask_kind, const float* v, const float* M, float* moments,
                 int moments_reduced, const void* evd_scratch, int L_total, int l_offset, float grad_scale, float* loss,
                 const nsvd_params* grads, void* ws, size_t ws_bytes, int path, void* stream) {
    EvdCall c = EvdCall();
    c.desc = desc; c.params = params; c.prob = prob;
    c.x = x; c.B = B;
    c.f = f; c.Tf = Tf; c.mask_kind = mask_kind; c.v = v; c.M = M;
    c.moments = moments; c.moments_reduced = moments_reduced; c.evd_scratch = evd_scratch;
    c.L_total = L_total; c.l_offset = l_offset; c.grad_scale = grad_scale; c.loss = loss;
    c.grads = grads;
    c.ws = ws; c.ws_bytes = ws_bytes; c.path = path; c.stream = stream;
    return c;
}

// the next batch of a step (drawn by the sampler, written to x_next) and the OTHER workspace set its features go to
int next_batch(EvdCall& c, unsigned long long seed, unsigned long long offset, float* x_next, void* ws_next,
               size_t ws_next_bytes) {
    if (!x_next || !ws_next || ws_next == c.ws || !c.desc) return NSVD_EINVAL;
    if (!nsvd_ws_ok(ws_next, ws_next_bytes, nsvd_workspace_bytes(c.desc, c.B))) return NSVD_EINVAL;
    if (const int st = validate_problem(c.desc, c.prob)) return st;
    c.next.smp = make_sampler(*c.prob, seed, offset);
    c.next.x = x_next;
    c.next.ws = ws_next;
    c.next.eps = c.prob->eps;
    return 0;
}

// nsvd_rmsprop -> the step the kernels take: RMSprop without momentum, its device-resident schedule in `state`
int opt_step_from(const nsvd_model_desc& d, const nsvd_rmsprop& o, NsvdOptStep* st) {
    int rc = check_params(d, &o.sq, false);
    if (rc) return rc;
    if (o.has_ema) {
        rc = check_params(d, &o.ema, false);
        if (rc) return rc;
        st->ema = &o.ema;
    }
    st->sq = o.sq;
    st->h = nsvd_make_hyper(o.lr, o.alpha, o.eps, o.has_ema ? o.ema_decay : 0.0, 1.0);
    st->state = o.state;
    if (st->state && ((uintptr_t)st->state & 7) != 0) return NSVD_EINVAL;
    return 0;
}

// nsvd_optimizer -> the step the kernels take: any rule of opt_math.h
int opt_step_from(const nsvd_model_desc& d, const nsvd_optimizer& o, NsvdOptStep* st) {
    const nsvd_opt_config& c = o.cfg;
    const int rule = nsvd_opt_rule(c.kind, c.momentum);
    if (rule < 0) return NSVD_EINVAL;
    int rc;
    if (nsvd_rule_uses_sq(rule)) {
        rc = check_params(d, &o.sq, false);
        if (rc) return rc;
        st->sq = o.sq;
    }
    if (nsvd_rule_uses_mom(rule)) {
        rc = check_params(d, &o.mom, false);
        if (rc) return rc;
        st->mom = &o.mom;
    }
    if (o.has_ema) {
        rc = check_params(d, &o.ema, false);
        if (rc) return rc;
        st->ema = &o.ema;
    }
    if (o.state && ((uintptr_t)o.state & 7) != 0) return NSVD_EINVAL;
    st->rule = rule;
    if (rule == NSVD_RULE_RMSPROP) {
        if (o.state) return NSVD_EUNSUPPORTED;  // (its device-resident schedule is nsvd_rmsprop::state)
        st->h = nsvd_make_hyper(c.lr, c.alpha, c.eps, o.has_ema ? c.ema_decay : 0.0, 1.0);
    } else {
        st->oh = nsvd_make_opt_hyper(rule, c.lr, c.alpha, c.eps, c.momentum, c.beta1, c.beta2,
                                     o.has_ema ? c.ema_decay : 0.0, 1.0, o.steps_taken);
        st->ostate = o.state;
    }
    return 0;
}

// The trainable tensors of a model in the order of the optimiser table: W[i], b[i] per layer, then scales.
struct ParamTensors {
    int nlayers, count;
    size_t n[NSVD_OPT_TABLE_MAX];  // elements of tensor k
    explicit ParamTensors(const nsvd_model_desc& d)
        : nlayers(d.nlayers), count(2 * d.nlayers + (d.has_exp_mask ? 1 : 0)) {
        for (int i = 0; i < d.nlayers; ++i) {
            const size_t hin = i == 0 ? 2 * (size_t)d.m : (size_t)d.dims[i - 1], hout = (size_t)d.dims[i];
            n[2 * i] = (size_t)d.L * hout * hin;
            n[2 * i + 1] = (size_t)d.L * hout;
        }
        n[2 * d.nlayers] = (size_t)d.L;
    }
    // tensor k of a set laid out like the parameters (params, grads, optimiser state; no set: null)
    float* in(const nsvd_params* set, int k) const {
        if (!set) return nullptr;
        return k == 2 * nlayers ? set->scales : (k & 1) ? set->b[k / 2] : set->W[k / 2];
    }
};

// the optimiser step of the generic path: stand-alone launches behind the layer-by-layer backward
int generic_opt_step(const EvdCall& c, hipStream_t s) {
    const NsvdOptStep& st = c.opt;
    const ParamTensors t(*c.desc);
    int rc = 0;
    if (st.rule != NSVD_RULE_RMSPROP) {
        // the other rules: one stand-alone launch per tensor (scalars from the device-resident schedule when there is
        // one: derived first, advanced by the last launch)
        if (st.ostate) {
            rc = nsvd_opt_state_begin(st.ostate, c.stream);
            if (rc) return rc;
        }
        for (int k = 0; k < t.count && !rc; ++k)
            rc = nsvd_opt_launch(st.rule, t.in(c.params, k), t.in(c.grads, k), t.in(&st.sq, k), t.in(st.mom, k),
                                 t.in(st.ema, k), t.n[k], st.oh, s, st.ostate, k == t.count - 1);
        return rc;
    }
    // generic path + fused-step request: ONE stand-alone optimiser launch over the table of tensors (unaligned tensors -
    // never with torch allocations -: one launch per tensor)
    NsvdOptTable tab;
    memset(&tab, 0, sizeof(tab));
    for (int k = 0; k < t.count; ++k) {
        tab.p[k] = t.in(c.params, k); tab.g[k] = t.in(c.grads, k); tab.sq[k] = t.in(&st.sq, k);
        tab.ema[k] = t.in(st.ema, k); tab.n[k] = t.n[k];
    }
    tab.count = t.count;
    rc = nsvd_rmsprop_table_launch(tab, st.h, s);
    if (rc != NSVD_EUNSUPPORTED) return rc;  // (misaligned pointers: one launch per tensor below)
    rc = 0;
    for (int k = 0; k < t.count && !rc; ++k)
        rc = nsvd_rmsprop_launch(t.in(c.params, k), t.in(c.grads, k), t.in(&st.sq, k), t.in(st.ema, k), t.n[k], st.h, s);
    return rc;
}

// The conversion of the entry point's optimiser descriptor into c.opt stands between the checks of the inputs and those
// of the workspace and the path, where its refusals always stood; everything behind it sees c.opt alone.
int backward_evd(EvdCall& c) {
    const nsvd_model_desc* desc = c.desc;
    const int B = c.B;
    int rc = validate(desc, c.model_mode ? MODEL_MAX_D : NSVD_MAX_D);
    if (rc) return rc;
    if ((!c.prob && !c.model_mode) || !c.x || !c.f || !c.Tf || !c.ws || B <= 0) return NSVD_EINVAL;
    // direct mode (fused path): neither reduced moments nor partial sums - the backward kernel takes the moments it
    // needs from f itself; `moments` and `loss` are then not written
    const bool direct = !c.moments_reduced && !c.evd_scratch;
    if (!direct && !c.moments) return NSVD_EINVAL;
    if (c.mask_kind < 0 || c.mask_kind > NSVD_MASK_JOINT) return NSVD_EINVAL;
    if (c.mask_kind == NSVD_MASK_CUSTOM && (!c.v || !c.M)) return NSVD_EINVAL;
    rc = check_params(*desc, c.params, true);
    if (rc) return rc;
    c.take_step = c.rmsprop || c.optimizer;
    if (c.grads || !c.take_step) {
        rc = check_params(*desc, c.grads, false);
        if (rc) return rc;
    }
    if (c.take_step) {
        rc = c.rmsprop ? opt_step_from(*desc, *c.rmsprop, &c.opt) : opt_step_from(*desc, *c.optimizer, &c.opt);
        if (rc) return rc;
        c.opt.emit_planes = !c.model_mode && c.path == NSVD_PATH_FUSED_BF16X3;
    }
    hipStream_t s = (hipStream_t)c.stream;
    bool fused;
    if (c.model_mode) {
        if (!nsvd_ws_ok(c.ws, c.ws_bytes, nsvd_model_workspace_bytes(desc, B))) return NSVD_EINVAL;
        fused = nsvd_fused_model_supported(*desc, B);
        if (!fused) return NSVD_EUNSUPPORTED;  // plain-model training steps exist on the MFMA kernels only
    } else {
        rc = resolve_path(*desc, *c.prob, B, c.ws, c.ws_bytes, c.path, &fused);
        if (rc) return rc;
    }
    const int L = c.L_total <= 0 ? desc->L : c.L_total;  // f, Tf, moments and masks are indexed by GLOBAL head
    if (c.l_offset < 0 || c.l_offset + desc->L > L || L > 128) return NSVD_EINVAL;
    const NsvdEvdChunking ch = nsvd_evd_chunking(B);
    if (fused) {
        NsvdEvdIn in;
        memset(&in, 0, sizeof(in));
        in.f = c.f; in.Tf = c.Tf; in.v = c.v; in.M = c.M;
        in.kind = c.mask_kind;
        in.grad_scale = c.grad_scale;
        in.loss = c.loss;
        in.Lg = L;
        in.l_off = c.l_offset;
        if (direct) {
            // (the loss scalars come from per-head partials of the chain kernel, added by the weight-gradient kernel)
        } else if (c.moments_reduced) {
            in.moments = c.moments;
        } else {
            in.part = (const float*)c.evd_scratch;
            in.part_op = in.part + (size_t)(ch.n1 + ch.n2) * L * L;
            in.moments_out = c.moments;
        }
        if (c.l_count < 0 || c.l_begin < 0 || c.l_begin + c.l_count > desc->L) return NSVD_EINVAL;
        if (c.opt.ostate) {  // the step's scalars, derived before the step's first kernel
            rc = nsvd_opt_state_begin(c.opt.ostate, c.stream);
            if (rc) return rc;
        }
        NsvdFusedBwdReq req = NsvdFusedBwdReq();
        req.l_begin = c.l_begin; req.l_count = c.l_count;
        req.next = c.next.x ? &c.next : nullptr;
        req.window_of_step = c.window_of_step; req.not_last = c.not_last; req.ev_after_chain = c.ev_after_chain;
        return nsvd_fused_backward_evd(*desc, *c.params, B, in, c.grads, c.take_step ? &c.opt : nullptr, c.ws, s, req);
    }
    if (c.window_of_step) return NSVD_EUNSUPPORTED;  // windows of a fused step exist on the fused kernels only
    if (c.next.x) return NSVD_EUNSUPPORTED;  // guest feature workgroups exist on the fused kernels only
    if (c.opt.state) return NSVD_EUNSUPPORTED;  // the device-resident schedule is read by the fused kernels only
    if (c.l_count > 0 && c.l_count != desc->L) return NSVD_EUNSUPPORTED;  // head windows need the fused kernels
    // generic path: finish the loss with the stand-alone kernels, then the layer-by-layer backward
    if (direct) return NSVD_EINVAL;  // needs the partial moments (evd_scratch) or the reduced ones
    if (L != desc->L) return NSVD_EUNSUPPORTED;  // head-parallel sharding needs the fused kernels
    if (generic_exact(c.path) && generic_exact_status(*c.prob)) return NSVD_EUNSUPPORTED;
    const int erows = generic_erows(*desc, c.path);  // (the workspace of the forward call: jet blocks or stencil blocks)
    const GenericWs w = carve(*desc, B, c.ws, erows);
    if (!c.moments_reduced) {
        rc = nsvd_evd_reduce_partials(c.evd_scratch, B, L, c.moments, s);
        if (rc) return rc;
    }
    rc = nsvd_evd_loss_grad(c.f, c.Tf, B, L, c.mask_kind, c.v, c.M, c.moments, c.grad_scale, c.loss, w.df, c.stream);
    if (rc) return rc;
    if (!c.grads) return NSVD_EINVAL;  // the generic path needs somewhere to put the gradients
    rc = generic_backward(*desc, *c.params, c.x, B, w.df, *c.grads, c.ws, s, erows);
    if (rc || !c.take_step) return rc;
    return generic_opt_step(c, s);
}
}  // namespace

extern "C" int nsvd_operator_backward_evd(const nsvd_model_desc* desc, const nsvd_params* params,
                                          const nsvd_problem* prob, const float* x, int B, const float* f,
                                          const float* Tf, int mask_kind, const float* v, const float* M,
                                          float* moments, int moments_reduced, const void* evd_scratch,
                                          int L_total, int l_offset, float grad_scale, float* loss,
                                          const nsvd_params* grads, void* ws, size_t ws_bytes, int path,
                                          void* stream) {
    if (!grads) return NSVD_EINVAL;
    EvdCall c = evd_call(desc, params, prob, x, B, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch,
                         L_total, l_offset, grad_scale, loss, grads, ws, ws_bytes, path, stream);
    return backward_evd(c);
}

extern "C" int nsvd_operator_backward_evd_heads(const nsvd_model_desc* desc, const nsvd_params* params,
                                                const nsvd_problem* prob, const float* x, int B, const float* f,
                                                const float* Tf, int mask_kind, const float* v, const float* M,
                                                float* moments, int moments_reduced, const void* evd_scratch,
                                                int L_total, int l_offset, float grad_scale, float* loss,
                                                const nsvd_params* grads, void* ws, size_t ws_bytes, int path,
                                                int l_begin, int l_count, void* stream) {
    if (!grads || l_count <= 0) return NSVD_EINVAL;
    EvdCall c = evd_call(desc, params, prob, x, B, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch,
                         L_total, l_offset, grad_scale, loss, grads, ws, ws_bytes, path, stream);
    c.l_begin = l_begin;
    c.l_count = l_count;
    return backward_evd(c);
}

extern "C" int nsvd_backward_head_window_ok(const nsvd_model_desc* desc, const nsvd_problem* prob, int B, int path,
                                            int l_count) {
    if (validate(desc) != 0 || !prob || B <= 0) return 0;
    if (!want_fused(*desc, B, path, !(prob->eps > 0.f))) return l_count == desc->L;
    return nsvd_fused_backward_window_ok(*desc, B, l_count) ? 1 : 0;
}

extern "C" int nsvd_operator_backward_evd_step(const nsvd_model_desc* desc, const nsvd_params* params,
                                               const nsvd_problem* prob, const float* x, int B, const float* f,
                                               const float* Tf, int mask_kind, const float* v, const float* M,
                                               float* moments, int moments_reduced, const void* evd_scratch,
                                               int L_total, int l_offset, float grad_scale, float* loss,
                                               const nsvd_params* grads, const nsvd_rmsprop* opt, void* ws,
                                               size_t ws_bytes, int path, void* stream) {
    if (!opt) return NSVD_EINVAL;
    EvdCall c = evd_call(desc, params, prob, x, B, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch,
                         L_total, l_offset, grad_scale, loss, grads, ws, ws_bytes, path, stream);
    c.rmsprop = opt;
    return backward_evd(c);
}

extern "C" int nsvd_operator_backward_evd_step_window(const nsvd_model_desc* desc, const nsvd_params* params,
                                                      const nsvd_problem* prob, const float* x, int B, const float* f,
                                                      const float* Tf, int mask_kind, const float* v, const float* M,
                                                      float* moments, int moments_reduced, const void* evd_scratch,
                                                      int L_total, int l_offset, float grad_scale, float* loss,
                                                      const nsvd_params* grads, const nsvd_rmsprop* opt, void* ws,
                                                      size_t ws_bytes, int path, int l_begin, int l_count,
                                                      int last_window, void* ev_after_chain,
                                                      unsigned long long next_seed, unsigned long long next_offset,
                                                      float* x_next, void* ws_next, size_t ws_next_bytes,
                                                      void* stream) {
    if (!opt || !prob || l_count <= 0) return NSVD_EINVAL;
    EvdCall c = evd_call(desc, params, prob, x, B, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch,
                         L_total, l_offset, grad_scale, loss, grads, ws, ws_bytes, path, stream);
    // the next batch rides in THIS window's chain launch (pass it to one window of the step only)
    if (x_next)
        if (const int rc = next_batch(c, next_seed, next_offset, x_next, ws_next, ws_next_bytes)) return rc;
    c.l_begin = l_begin;
    c.l_count = l_count;
    c.window_of_step = 1;
    c.not_last = last_window ? 0 : 1;
    c.ev_after_chain = ev_after_chain;
    c.rmsprop = opt;
    return backward_evd(c);
}

extern "C" int nsvd_operator_backward_evd_step_next(const nsvd_model_desc* desc, const nsvd_params* params,
                                                    const nsvd_problem* prob, const float* x, int B, const float* f,
                                                    const float* Tf, int mask_kind, const float* v, const float* M,
                                                    float* moments, int moments_reduced, const void* evd_scratch,
                                                    int L_total, int l_offset, float grad_scale, float* loss,
                                                    const nsvd_params* grads, const nsvd_rmsprop* opt, void* ws,
                                                    size_t ws_bytes, int path, unsigned long long next_seed,
                                                    unsigned long long next_offset, float* x_next, void* ws_next,
                                                    size_t ws_next_bytes, void* stream) {
    if (!opt || !prob) return NSVD_EINVAL;
    EvdCall c = evd_call(desc, params, prob, x, B, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch,
                         L_total, l_offset, grad_scale, loss, grads, ws, ws_bytes, path, stream);
    if (const int rc = next_batch(c, next_seed, next_offset, x_next, ws_next, ws_next_bytes)) return rc;  // (mandatory)
    c.rmsprop = opt;
    return backward_evd(c);
}

extern "C" int nsvd_model_backward_evd_step(const nsvd_model_desc* desc, const nsvd_params* params, const float* x,
                                            int B, const float* f, const float* Tf, int mask_kind, const float* v,
                                            const float* M, float* moments, int moments_reduced,
                                            const void* evd_scratch, int L_total, int l_offset, float grad_scale,
                                            float* loss, const nsvd_params* grads, const nsvd_rmsprop* opt, void* ws,
                                            size_t ws_bytes, void* stream) {
    if (!opt && !grads) return NSVD_EINVAL;
    EvdCall c = evd_call(desc, params, nullptr, x, B, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch,
                         L_total, l_offset, grad_scale, loss, grads, ws, ws_bytes, NSVD_PATH_AUTO, stream);
    c.model_mode = true;
    c.rmsprop = opt;
    return backward_evd(c);
}

extern "C" int nsvd_operator_backward_evd_opt_step(const nsvd_model_desc* desc, const nsvd_params* params,
                                                   const nsvd_problem* prob, const float* x, int B, const float* f,
                                                   const float* Tf, int mask_kind, const float* v, const float* M,
                                                   float* moments, int moments_reduced, const void* evd_scratch,
                                                   int L_total, int l_offset, float grad_scale, float* loss,
                                                   const nsvd_params* grads, const nsvd_optimizer* opt, void* ws,
                                                   size_t ws_bytes, int path, unsigned long long next_seed,
                                                   unsigned long long next_offset, float* x_next, void* ws_next,
                                                   size_t ws_next_bytes, void* stream) {
    if (!opt || !prob) return NSVD_EINVAL;
    if (nsvd_opt_rule(opt->cfg.kind, opt->cfg.momentum) < 0) return NSVD_EINVAL;
    EvdCall c = evd_call(desc, params, prob, x, B, f, Tf, mask_kind, v, M, moments, moments_reduced, evd_scratch,
                         L_total, l_offset, grad_scale, loss, grads, ws, ws_bytes, path, stream);
    if (x_next)
        if (const int rc = next_batch(c, next_seed, next_offset, x_next, ws_next, ws_next_bytes)) return rc;
    c.optimizer = opt;
    return backward_evd(c);
}
