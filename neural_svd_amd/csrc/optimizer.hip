// Fused RMSprop + EMA over a flat parameter buffer: one pass, 16-byte accesses.
//   reference: torch.optim.RMSprop as configured at examples/utils.py:50-57 (alpha, eps=1e-10,
//              momentum 0, not centred), stepped at examples/operator/__init__.py:69-70;
//              torch_ema update at examples/operator/__init__.py:73.
// HBM-bound: reads p, g, sq, ema and writes p, sq, ema = 28 B per parameter.
#include <string.h>
#include "nsvd_kernels.h"
#include "opt_math.h"

namespace {

typedef NsvdHyper Hyper;
__device__ __forceinline__ void upd(float& p, float g, float& sq, float* ema, const Hyper& h) {
    float none = 0.f;
    nsvd_rmsprop_upd(p, g, sq, ema ? *ema : none, ema != nullptr, h);
}

template <bool HAS_EMA>
__global__ void __launch_bounds__(256) rmsprop_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ sq, float* __restrict__ ema, size_t n4,
                                                          size_t n, Hyper h, nsvd_step_state* state, int advance) {
    if (state) {  // device-resident schedule: the step's values from state->cur (grad_scale stays the caller's)
        const float gs = h.grad_scale;
        h = *nsvd_state_hyper(state);
        h.grad_scale = gs;
    }
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 sv = reinterpret_cast<float4*>(sq)[i];
        float4 ev = HAS_EMA ? reinterpret_cast<float4*>(ema)[i] : make_float4(0, 0, 0, 0);
        upd(pv.x, gv.x, sv.x, HAS_EMA ? &ev.x : nullptr, h);
        upd(pv.y, gv.y, sv.y, HAS_EMA ? &ev.y : nullptr, h);
        upd(pv.z, gv.z, sv.z, HAS_EMA ? &ev.z : nullptr, h);
        upd(pv.w, gv.w, sv.w, HAS_EMA ? &ev.w : nullptr, h);
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(sq)[i] = sv;
        if (HAS_EMA) reinterpret_cast<float4*>(ema)[i] = ev;
    }
    // tail (n not a multiple of 4, or unaligned buffers: n4 == 0 and everything goes through here)
    for (size_t t = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        float pv = p[t], sv = sq[t], ev = HAS_EMA ? ema[t] : 0.f;
        upd(pv, g[t], sv, HAS_EMA ? &ev : nullptr, h);
        p[t] = pv;
        sq[t] = sv;
        if (HAS_EMA) ema[t] = ev;
    }
    // last optimiser launch of the step: nothing in this kernel reads `step` (only `cur`, which the NEXT step's first
    // kernel rewrites after the kernel boundary)
    if (state && advance && blockIdx.x == 0 && threadIdx.x == 0) state->step += 1;
}

// The same update over a TABLE of tensors in one launch (the generic path's step: one launch instead of one per tensor -
// nine launches of ~5 us each at three hidden layers). Element for element the arithmetic of the kernel above.
template <bool HAS_EMA>
__global__ void __launch_bounds__(256) rmsprop_ema_table_kernel(NsvdOptTable t, Hyper h) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t total4 = t.start[t.count];
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += stride) {
        int k = 0;
        while (q >= t.start[k + 1]) ++k;
        const size_t e = (q - t.start[k]) * 4;
        const size_t left = t.n[k] - e;
        float* p = t.p[k] + e;
        const float* g = t.g[k] + e;
        float* sq = t.sq[k] + e;
        float* ema = HAS_EMA ? t.ema[k] + e : nullptr;
        if (left >= 4) {
            float4 pv = *reinterpret_cast<float4*>(p);
            const float4 gv = *reinterpret_cast<const float4*>(g);
            float4 sv = *reinterpret_cast<float4*>(sq);
            float4 ev = HAS_EMA ? *reinterpret_cast<float4*>(ema) : make_float4(0, 0, 0, 0);
            upd(pv.x, gv.x, sv.x, HAS_EMA ? &ev.x : nullptr, h);
            upd(pv.y, gv.y, sv.y, HAS_EMA ? &ev.y : nullptr, h);
            upd(pv.z, gv.z, sv.z, HAS_EMA ? &ev.z : nullptr, h);
            upd(pv.w, gv.w, sv.w, HAS_EMA ? &ev.w : nullptr, h);
            *reinterpret_cast<float4*>(p) = pv;
            *reinterpret_cast<float4*>(sq) = sv;
            if (HAS_EMA) *reinterpret_cast<float4*>(ema) = ev;
        } else {
            for (size_t c = 0; c < left; ++c) {
                float pv = p[c], sv = sq[c], ev = HAS_EMA ? ema[c] : 0.f;
                upd(pv, g[c], sv, HAS_EMA ? &ev : nullptr, h);
                p[c] = pv;
                sq[c] = sv;
                if (HAS_EMA) ema[c] = ev;
            }
        }
    }
}

__global__ void step_state_init_kernel(nsvd_step_state* st, nsvd_step_state v) {
    *st = v;
    nsvd_step_state_derive(st);
}
__global__ void step_state_begin_kernel(nsvd_step_state* st) { nsvd_step_state_derive(st); }


// ---- any rule of opt_math.h over n contiguous floats: p, g and up to three state streams (sq, mom, ema), 16-byte
// accesses, the rule and the EMA as compile-time kinds (slots a rule does not use are neither read nor written).
template <int RULE, bool HAS_EMA>
__global__ void __launch_bounds__(256) opt_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ sq, float* __restrict__ mom,
                                                  float* __restrict__ ema, size_t n4, size_t n, NsvdOptHyper h,
                                                  nsvd_opt_state* state, int advance) {
    constexpr bool SQ = RULE == NSVD_RULE_RMSPROP || RULE == NSVD_RULE_RMSPROP_MOM || RULE == NSVD_RULE_ADAM;
    constexpr bool MOM = RULE == NSVD_RULE_RMSPROP_MOM || RULE == NSVD_RULE_SGD_MOM || RULE == NSVD_RULE_ADAM;
    if (state) {  // device-resident schedule: the step's values from state->cur (grad_scale stays the caller's)
        const float gs = h.b.grad_scale;
        h = *nsvd_opt_state_hyper(state);
        h.b.grad_scale = gs;
        if (h.rule != RULE) {  // the state was initialised for another rule: touch nothing, leave a mark
            if (blockIdx.x == 0 && threadIdx.x == 0) state->mismatch = 1;
            return;
        }
    }
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 sv = SQ ? reinterpret_cast<float4*>(sq)[i] : zero4;
        float4 mv = MOM ? reinterpret_cast<float4*>(mom)[i] : zero4;
        float4 ev = HAS_EMA ? reinterpret_cast<float4*>(ema)[i] : zero4;
        nsvd_opt_upd<RULE>(pv.x, gv.x, sv.x, mv.x, ev.x, HAS_EMA, h);
        nsvd_opt_upd<RULE>(pv.y, gv.y, sv.y, mv.y, ev.y, HAS_EMA, h);
        nsvd_opt_upd<RULE>(pv.z, gv.z, sv.z, mv.z, ev.z, HAS_EMA, h);
        nsvd_opt_upd<RULE>(pv.w, gv.w, sv.w, mv.w, ev.w, HAS_EMA, h);
        reinterpret_cast<float4*>(p)[i] = pv;
        if (SQ) reinterpret_cast<float4*>(sq)[i] = sv;
        if (MOM) reinterpret_cast<float4*>(mom)[i] = mv;
        if (HAS_EMA) reinterpret_cast<float4*>(ema)[i] = ev;
    }
    // tail (n not a multiple of 4, or unaligned buffers: n4 == 0 and everything goes through here)
    for (size_t t = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        float pv = p[t], sv = SQ ? sq[t] : 0.f, mv = MOM ? mom[t] : 0.f, ev = HAS_EMA ? ema[t] : 0.f;
        nsvd_opt_upd<RULE>(pv, g[t], sv, mv, ev, HAS_EMA, h);
        p[t] = pv;
        if (SQ) sq[t] = sv;
        if (MOM) mom[t] = mv;
        if (HAS_EMA) ema[t] = ev;
    }
    // last optimiser launch of the step: nothing in this kernel reads `step` (only `cur`, which the NEXT step's
    // nsvd_opt_state_begin rewrites after the kernel boundary)
    if (state && advance && blockIdx.x == 0 && threadIdx.x == 0) state->step += 1;
}

__global__ void opt_state_init_kernel(nsvd_opt_state* st, nsvd_opt_state v) {
    *st = v;
    nsvd_opt_state_derive(st);
}
__global__ void opt_state_begin_kernel(nsvd_opt_state* st) { nsvd_opt_state_derive(st); }

template <int RULE>
int opt_launch_rule(float* p, const float* grad, float* sq, float* mom, float* ema, size_t n, const NsvdOptHyper& h,
                    hipStream_t s, nsvd_opt_state* state, int advance) {
    if (!nsvd_rule_uses_sq(RULE)) sq = nullptr;  // (never dereferenced: keep them out of the alignment test too)
    if (!nsvd_rule_uses_mom(RULE)) mom = nullptr;
    const uintptr_t al = (uintptr_t)p | (uintptr_t)grad | (uintptr_t)sq | (uintptr_t)mom | (uintptr_t)ema;
    const size_t n4 = (al & 15) ? 0 : n / 4;  // unaligned (never with torch allocations): scalar path
    const size_t work = n4 ? n4 : n;
    size_t blocks = (work + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (ema) hipLaunchKernelGGL((opt_kernel<RULE, true>), dim3((unsigned)blocks), dim3(256), 0, s, p, grad, sq, mom, ema,
                                n4, n, h, state, advance);
    else hipLaunchKernelGGL((opt_kernel<RULE, false>), dim3((unsigned)blocks), dim3(256), 0, s, p, grad, sq, mom,
                            (float*)nullptr, n4, n, h, state, advance);
    NSVD_CHECK_LAUNCH();
    return 0;
}

int opt_config_ok(const nsvd_opt_config* c) {
    if (!c || nsvd_opt_rule(c->kind, c->momentum) < 0) return NSVD_EINVAL;
    return 0;
}

}  // namespace

int nsvd_rmsprop_launch(float* p, const float* grad, float* sq, float* ema, size_t n, const NsvdHyper& h,
                        hipStream_t s, nsvd_step_state* state, int advance) {
    if (n == 0) return 0;
    const uintptr_t al = (uintptr_t)p | (uintptr_t)grad | (uintptr_t)sq | (uintptr_t)ema;
    const size_t n4 = (al & 15) ? 0 : n / 4;  // unaligned (never with torch allocations): scalar path
    const size_t work = n4 ? n4 : n;
    size_t blocks = (work + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (ema) hipLaunchKernelGGL(rmsprop_ema_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, p, grad, sq, ema,
                                n4, n, h, state, advance);
    else hipLaunchKernelGGL(rmsprop_ema_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, p, grad, sq,
                            (float*)nullptr, n4, n, h, state, advance);
    NSVD_CHECK_LAUNCH();
    return 0;
}

int nsvd_rmsprop_table_launch(NsvdOptTable& t, const NsvdHyper& h, hipStream_t s) {
    if (t.count <= 0 || t.count > NSVD_OPT_TABLE_MAX) return NSVD_EINVAL;
    bool has_ema = t.ema[0] != nullptr;
    size_t q4 = 0;
    for (int k = 0; k < t.count; ++k) {
        if (!t.p[k] || !t.g[k] || !t.sq[k] || (t.ema[k] != nullptr) != has_ema) return NSVD_EINVAL;
        const uintptr_t al = (uintptr_t)t.p[k] | (uintptr_t)t.g[k] | (uintptr_t)t.sq[k] | (uintptr_t)t.ema[k];
        if (al & 15) return NSVD_EUNSUPPORTED;  // (never with torch allocations; the caller launches per tensor then)
        t.start[k] = q4;
        q4 += (t.n[k] + 3) / 4;
    }
    t.start[t.count] = q4;
    if (q4 == 0) return 0;
    size_t blocks = (q4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (has_ema) hipLaunchKernelGGL(rmsprop_ema_table_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, t, h);
    else hipLaunchKernelGGL(rmsprop_ema_table_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, t, h);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_rmsprop_ema_step(float* p, const float* grad, float* sq, float* ema, size_t n, double lr,
                                     double alpha, double eps, double ema_decay, double grad_scale,
                                     void* stream) {
    if (!p || !grad || !sq) return NSVD_EINVAL;
    return nsvd_rmsprop_launch(p, grad, sq, ema, n, nsvd_make_hyper(lr, alpha, eps, ema_decay, grad_scale),
                               (hipStream_t)stream);
}

extern "C" int nsvd_rmsprop_ema_step_dev(float* p, const float* grad, float* sq, float* ema, size_t n,
                                         nsvd_step_state* state, double grad_scale, int advance, void* stream) {
    if (!p || !grad || !sq || !state || ((uintptr_t)state & 7) != 0) return NSVD_EINVAL;
    return nsvd_rmsprop_launch(p, grad, sq, ema, n, nsvd_make_hyper(0.0, 0.0, 0.0, 0.0, grad_scale),
                               (hipStream_t)stream, state, advance);
}

extern "C" int nsvd_step_state_init(nsvd_step_state* state, double lr0, double eta_min, unsigned long long T_max,
                                    double alpha, double eps, double ema_decay, unsigned long long step,
                                    void* stream) {
    if (!state || ((uintptr_t)state & 7) != 0) return NSVD_EINVAL;
    nsvd_step_state v;
    memset(&v, 0, sizeof(v));
    v.step = step;
    v.T_max = T_max;
    v.lr0 = lr0; v.eta_min = eta_min; v.alpha = alpha; v.eps = eps; v.ema_decay = ema_decay;
    hipLaunchKernelGGL(step_state_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, v);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_step_state_begin(nsvd_step_state* state, void* stream) {
    if (!state || ((uintptr_t)state & 7) != 0) return NSVD_EINVAL;
    hipLaunchKernelGGL(step_state_begin_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
    NSVD_CHECK_LAUNCH();
    return 0;
}

int nsvd_opt_launch(int rule, float* p, const float* grad, float* sq, float* mom, float* ema, size_t n,
                    const NsvdOptHyper& h, hipStream_t s, nsvd_opt_state* state, int advance) {
    if (!p || !grad || (nsvd_rule_uses_sq(rule) && !sq) || (nsvd_rule_uses_mom(rule) && !mom)) return NSVD_EINVAL;
    // nothing to update: nothing launched (as nsvd_rmsprop_launch; the step counter then stays where it is)
    if (n == 0) return 0;
    switch (rule) {
        case NSVD_RULE_RMSPROP: return opt_launch_rule<NSVD_RULE_RMSPROP>(p, grad, sq, mom, ema, n, h, s, state, advance);
        case NSVD_RULE_RMSPROP_MOM: return opt_launch_rule<NSVD_RULE_RMSPROP_MOM>(p, grad, sq, mom, ema, n, h, s, state, advance);
        case NSVD_RULE_SGD: return opt_launch_rule<NSVD_RULE_SGD>(p, grad, sq, mom, ema, n, h, s, state, advance);
        case NSVD_RULE_SGD_MOM: return opt_launch_rule<NSVD_RULE_SGD_MOM>(p, grad, sq, mom, ema, n, h, s, state, advance);
        case NSVD_RULE_ADAM: return opt_launch_rule<NSVD_RULE_ADAM>(p, grad, sq, mom, ema, n, h, s, state, advance);
    }
    return NSVD_EINVAL;
}

extern "C" int nsvd_opt_step(float* p, const float* grad, float* sq, float* mom, float* ema, size_t n,
                             const nsvd_opt_config* cfg, unsigned long long steps_taken, double grad_scale,
                             void* stream) {
    if (opt_config_ok(cfg)) return NSVD_EINVAL;
    const int rule = nsvd_opt_rule(cfg->kind, cfg->momentum);
    const NsvdOptHyper h = nsvd_make_opt_hyper(rule, cfg->lr, cfg->alpha, cfg->eps, cfg->momentum, cfg->beta1,
                                               cfg->beta2, cfg->ema_decay, grad_scale, steps_taken);
    return nsvd_opt_launch(rule, p, grad, sq, mom, ema, n, h, (hipStream_t)stream, nullptr, 0);
}

extern "C" int nsvd_opt_step_dev(float* p, const float* grad, float* sq, float* mom, float* ema, size_t n,
                                 const nsvd_opt_config* cfg, nsvd_opt_state* state, double grad_scale, int advance,
                                 void* stream) {
    if (opt_config_ok(cfg) || !state || ((uintptr_t)state & 7) != 0) return NSVD_EINVAL;
    const int rule = nsvd_opt_rule(cfg->kind, cfg->momentum);
    NsvdOptHyper h;
    memset(&h, 0, sizeof(h));
    h.b.grad_scale = (float)grad_scale;
    return nsvd_opt_launch(rule, p, grad, sq, mom, ema, n, h, (hipStream_t)stream, state, advance);
}

extern "C" int nsvd_opt_state_init(nsvd_opt_state* state, const nsvd_opt_config* cfg, double eta_min,
                                   unsigned long long T_max, unsigned long long step, void* stream) {
    if (opt_config_ok(cfg) || !state || ((uintptr_t)state & 7) != 0) return NSVD_EINVAL;
    nsvd_opt_state v;
    memset(&v, 0, sizeof(v));
    v.step = step;
    v.T_max = T_max;
    v.lr0 = cfg->lr; v.eta_min = eta_min; v.alpha = cfg->alpha; v.eps = cfg->eps; v.ema_decay = cfg->ema_decay;
    v.momentum = cfg->momentum; v.beta1 = cfg->beta1; v.beta2 = cfg->beta2;
    v.kind = cfg->kind;
    hipLaunchKernelGGL(opt_state_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, v);
    NSVD_CHECK_LAUNCH();
    return 0;
}

extern "C" int nsvd_opt_state_begin(nsvd_opt_state* state, void* stream) {
    if (!state || ((uintptr_t)state & 7) != 0) return NSVD_EINVAL;
    hipLaunchKernelGGL(opt_state_begin_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
    NSVD_CHECK_LAUNCH();
    return 0;
}
