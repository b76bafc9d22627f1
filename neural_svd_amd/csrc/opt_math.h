// RMSprop + EMA update of one parameter, shared by the stand-alone optimiser kernel (optimizer.hip) and the
// weight-gradient kernel's fused epilogue (pmlp_bwd.hip); and the other rules of the reference's get_optimizer
// (examples/utils.py:48-72: SGD with / without momentum, RMSprop with momentum, Adam), which the stand-alone kernel runs.
//   reference: torch.optim.RMSprop as configured at examples/utils.py:50-57 (alpha, eps = 1e-10, momentum 0,
//              not centred), stepped at examples/operator/__init__.py:69-70; torch_ema update at :73.
#pragma once
#include "nsvd_common.h"

struct NsvdHyper {
    float lr, alpha, one_minus_alpha, eps, one_minus_decay, grad_scale;
};

// parameter / square average (RMSprop's, Adam's exp_avg_sq; null for rules without one) / EMA shadow (null: none) of
// one tensor, element-aligned with its gradient. The `mom` slot (momentum buffer, Adam's exp_avg) of the rules that have
// one travels beside this struct, in arrays of its own: the struct keeps its size, and with it the RMSprop kernels keep
// their code (a 32-byte element changes the indexing arithmetic of every instance).
struct NsvdOptPtrs {
    float* p;
    float* sq;
    float* ema;
};

static_assert(sizeof(((nsvd_step_state*)0)->cur) == sizeof(NsvdHyper), "nsvd_step_state::cur is an NsvdHyper");
__device__ __forceinline__ const NsvdHyper* nsvd_state_hyper(const nsvd_step_state* st) {
    return reinterpret_cast<const NsvdHyper*>(&st->cur);
}

// cur <- the scheduled values of step st->step: CosineAnnealingLR's closed form after `step` scheduler steps
// (torch/optim/lr_scheduler.py; examples/operator/__init__.py:35,71-72) and torch_ema's decay at its (step + 1)-th
// update (:36,73), in the double-precision expressions trainer.cosine_lr / FusedTrainer._advance_schedule evaluate on
// the host, rounded to float32 where nsvd_make_hyper rounds. Called by ONE thread.
__device__ inline void nsvd_step_state_derive(nsvd_step_state* st) {
#pragma clang fp contract(off)
    const unsigned long long t = st->step;
    double lr = st->lr0;
    if (st->T_max) {
        const double c = cos((3.141592653589793 * (double)t) / (double)st->T_max);
        lr = st->eta_min + ((st->lr0 - st->eta_min) * (1.0 + c)) / 2.0;
    }
    const double n = (double)(t + 1);
    const double warm = (1.0 + n) / (10.0 + n);
    const double decay = st->ema_decay < warm ? st->ema_decay : warm;
    st->cur.lr = (float)lr;
    st->cur.alpha = (float)st->alpha;
    st->cur.one_minus_alpha = (float)(1.0 - st->alpha);
    st->cur.eps = (float)st->eps;
    st->cur.one_minus_decay = (float)(1.0 - decay);
    st->cur.grad_scale = 1.0f;
}

// host scalars are doubles (Python floats), rounded to float32 exactly where torch rounds them
static inline NsvdHyper nsvd_make_hyper(double lr, double alpha, double eps, double ema_decay, double grad_scale) {
    NsvdHyper h;
    h.lr = (float)lr;
    h.alpha = (float)alpha;
    h.one_minus_alpha = (float)(1.0 - alpha);
    h.eps = (float)eps;
    h.one_minus_decay = (float)(1.0 - ema_decay);
    h.grad_scale = (float)grad_scale;
    return h;
}

// ema by reference + flag (not an optional pointer: a conditionally taken address of a local keeps it in scratch)
__device__ __forceinline__ void nsvd_rmsprop_upd(float& p, float g, float& sq, float& ema, bool has_ema,
                                                 const NsvdHyper& h) {
    const float lr = h.lr, eps = h.eps, one_minus_decay = h.one_minus_decay;
    g *= h.grad_scale;
    sq = h.alpha * sq + h.one_minus_alpha * (g * g);  // square_avg.mul_(alpha).addcmul_(g, g, value=1-alpha)
    const float avg = sqrtf(sq) + eps;                // square_avg.sqrt().add_(eps)
    p = p - lr * (g / avg);                           // param.addcdiv_(g, avg, value=-lr)
    if (has_ema) ema = ema - one_minus_decay * (ema - p);
}

// ---------------------------------------------------------------------------------------------------------------------
// The other rules of examples/utils.py:48-72 (weight_decay 0, dampening 0, no Nesterov, no amsgrad, not centred), one
// update function each, in torch's single-tensor float32 sequence (torch/optim/{sgd,rmsprop,adam}.py). The rule is a
// compile-time kind; state is two optional slots beside p and ema: `sq` (RMSprop's square average, Adam's exp_avg_sq)
// and `mom` (the momentum buffers, Adam's exp_avg).
enum NsvdOptRule {
    NSVD_RULE_RMSPROP = 0,      // momentum 0: nsvd_rmsprop_upd above               state: sq
    NSVD_RULE_RMSPROP_MOM = 1,  //                                                  state: sq, mom
    NSVD_RULE_SGD = 2,          // momentum 0                                       state: none
    NSVD_RULE_SGD_MOM = 3,      //                                                  state: mom
    NSVD_RULE_ADAM = 4,         //                                                  state: sq (v), mom (m)
    NSVD_RULE_COUNT = 5
};
#if defined(__HIPCC__)
#define NSVD_HD __host__ __device__
#else
#define NSVD_HD
#endif
NSVD_HD static inline int nsvd_opt_rule(int kind, double momentum) {  // -1: unknown kind
    if (kind == NSVD_OPT_RMSPROP) return momentum != 0.0 ? NSVD_RULE_RMSPROP_MOM : NSVD_RULE_RMSPROP;
    if (kind == NSVD_OPT_SGD) return momentum != 0.0 ? NSVD_RULE_SGD_MOM : NSVD_RULE_SGD;
    if (kind == NSVD_OPT_ADAM) return NSVD_RULE_ADAM;
    return -1;
}
NSVD_HD static constexpr bool nsvd_rule_uses_sq(int rule) {
    return rule == NSVD_RULE_RMSPROP || rule == NSVD_RULE_RMSPROP_MOM || rule == NSVD_RULE_ADAM;
}
NSVD_HD static constexpr bool nsvd_rule_uses_mom(int rule) {
    return rule == NSVD_RULE_RMSPROP_MOM || rule == NSVD_RULE_SGD_MOM || rule == NSVD_RULE_ADAM;
}

// the float32 scalars of one step of any rule: NsvdHyper (same rounding points) and what the new rules add
struct NsvdOptHyper {
    NsvdHyper b;            // Adam: b.lr is the plain learning rate (unused by the update), b.eps is adam_eps
    float momentum;         // SGD / RMSprop
    float one_minus_beta1;  // Adam: exp_avg.lerp_(g, 1 - beta1)
    float beta2, one_minus_beta2;
    float step_size;        // Adam: lr / (1 - beta1^t), formed in double
    float bc2_sqrt;         // Adam: sqrt(1 - beta2^t), formed in double
    int first_step;         // SGD with momentum: no step taken yet - buf = g
    int rule;               // NsvdOptRule these scalars were derived for
};
static_assert(sizeof(((nsvd_opt_state*)0)->cur) == sizeof(NsvdOptHyper), "nsvd_opt_state::cur is an NsvdOptHyper");

// Scalars of the step taken after `step` earlier ones (Adam's t = step + 1), from the step's already scheduled learning
// rate and already warmed-up EMA decay. The SAME double-precision expressions on the host path (nsvd_opt_step) and on
// the device (nsvd_opt_state_derive); rounded to float32 where torch rounds its Python floats.
NSVD_HD static inline NsvdOptHyper nsvd_make_opt_hyper(int rule, double lr, double alpha, double eps, double momentum,
                                                       double beta1, double beta2, double ema_decay, double grad_scale,
                                                       unsigned long long step) {
    NsvdOptHyper h;
    h.b.lr = (float)lr;
    h.b.alpha = (float)alpha;
    h.b.one_minus_alpha = (float)(1.0 - alpha);
    h.b.eps = (float)eps;
    h.b.one_minus_decay = (float)(1.0 - ema_decay);
    h.b.grad_scale = (float)grad_scale;
    h.momentum = (float)momentum;
    h.one_minus_beta1 = (float)(1.0 - beta1);
    h.beta2 = (float)beta2;
    h.one_minus_beta2 = (float)(1.0 - beta2);
    h.step_size = 0.f;
    h.bc2_sqrt = 1.f;
    if (rule == NSVD_RULE_ADAM) {
        const double t = (double)(step + 1);
        const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
        h.step_size = (float)(lr / bc1);
        h.bc2_sqrt = (float)sqrt(bc2);
    }
    h.first_step = step == 0 ? 1 : 0;
    h.rule = rule;
    return h;
}

__device__ __forceinline__ NsvdOptHyper* nsvd_opt_state_hyper(nsvd_opt_state* st) {
    return reinterpret_cast<NsvdOptHyper*>(&st->cur);
}

// cur <- the scheduled values of step st->step: nsvd_step_state_derive's schedule expressions (cosine learning rate,
// torch_ema warm-up) followed by nsvd_make_opt_hyper. Called by ONE thread.
__device__ inline void nsvd_opt_state_derive(nsvd_opt_state* st) {
#pragma clang fp contract(off)
    const unsigned long long t = st->step;
    double lr = st->lr0;
    if (st->T_max) {
        const double c = cos((3.141592653589793 * (double)t) / (double)st->T_max);
        lr = st->eta_min + ((st->lr0 - st->eta_min) * (1.0 + c)) / 2.0;
    }
    const double n = (double)(t + 1);
    const double warm = (1.0 + n) / (10.0 + n);
    const double decay = st->ema_decay < warm ? st->ema_decay : warm;
    *nsvd_opt_state_hyper(st) = nsvd_make_opt_hyper(nsvd_opt_rule(st->kind, st->momentum), lr, st->alpha, st->eps,
                                                    st->momentum, st->beta1, st->beta2, decay, 1.0, t);
}

__device__ __forceinline__ void nsvd_ema_upd(float& ema, float p, bool has_ema, const NsvdHyper& h) {
    if (has_ema) ema = ema - h.one_minus_decay * (ema - p);
}

// torch.optim.SGD, momentum 0: param.add_(g, alpha=-lr)
__device__ __forceinline__ void nsvd_sgd_upd(float& p, float g, float& ema, bool has_ema, const NsvdOptHyper& h) {
    g *= h.b.grad_scale;
    p = p - h.b.lr * g;
    nsvd_ema_upd(ema, p, has_ema, h.b);
}

// torch.optim.SGD, momentum > 0: buf = clone(g) on the first step, else buf.mul_(momentum).add_(g); param.add_(buf, alpha=-lr)
__device__ __forceinline__ void nsvd_sgd_mom_upd(float& p, float g, float& mom, float& ema, bool has_ema,
                                                 const NsvdOptHyper& h) {
    g *= h.b.grad_scale;
    mom = h.first_step ? g : h.momentum * mom + g;
    p = p - h.b.lr * mom;
    nsvd_ema_upd(ema, p, has_ema, h.b);
}

// torch.optim.RMSprop, momentum > 0: square_avg as in nsvd_rmsprop_upd; buf.mul_(momentum).addcdiv_(g, avg);
// param.add_(buf, alpha=-lr)
__device__ __forceinline__ void nsvd_rmsprop_mom_upd(float& p, float g, float& sq, float& mom, float& ema, bool has_ema,
                                                     const NsvdOptHyper& h) {
    g *= h.b.grad_scale;
    sq = h.b.alpha * sq + h.b.one_minus_alpha * (g * g);
    const float avg = sqrtf(sq) + h.b.eps;
    mom = h.momentum * mom + g / avg;
    p = p - h.b.lr * mom;
    nsvd_ema_upd(ema, p, has_ema, h.b);
}

// torch.optim.Adam: exp_avg.lerp_(g, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2);
// denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps); param.addcdiv_(exp_avg, denom, value=-step_size)
__device__ __forceinline__ void nsvd_adam_upd(float& p, float g, float& v, float& m, float& ema, bool has_ema,
                                              const NsvdOptHyper& h) {
    g *= h.b.grad_scale;
    m = m + h.one_minus_beta1 * (g - m);
    v = h.beta2 * v + h.one_minus_beta2 * (g * g);
    const float denom = sqrtf(v) / h.bc2_sqrt + h.b.eps;
    p = p - h.step_size * (m / denom);
    nsvd_ema_upd(ema, p, has_ema, h.b);
}

// the rule as a compile-time kind (slots a rule does not use are passed as dummies and left alone)
template <int RULE>
__device__ __forceinline__ void nsvd_opt_upd(float& p, float g, float& sq, float& mom, float& ema, bool has_ema,
                                             const NsvdOptHyper& h) {
    if constexpr (RULE == NSVD_RULE_RMSPROP) nsvd_rmsprop_upd(p, g, sq, ema, has_ema, h.b);
    else if constexpr (RULE == NSVD_RULE_RMSPROP_MOM) nsvd_rmsprop_mom_upd(p, g, sq, mom, ema, has_ema, h);
    else if constexpr (RULE == NSVD_RULE_SGD) nsvd_sgd_upd(p, g, ema, has_ema, h);
    else if constexpr (RULE == NSVD_RULE_SGD_MOM) nsvd_sgd_mom_upd(p, g, mom, ema, has_ema, h);
    else nsvd_adam_upd(p, g, sq, mom, ema, has_ema, h);
}

// the scalars a rule's update reads: RMSprop without momentum keeps NsvdHyper (and with it the code it has always had)
template <int RULE> struct NsvdRuleHyper { typedef NsvdOptHyper type; };
template <> struct NsvdRuleHyper<NSVD_RULE_RMSPROP> { typedef NsvdHyper type; };
template <int RULE>
__device__ __forceinline__ void nsvd_rule_upd(float& p, float g, float& sq, float& mom, float& ema, bool has_ema,
                                              const typename NsvdRuleHyper<RULE>::type& h) {
    if constexpr (RULE == NSVD_RULE_RMSPROP) nsvd_rmsprop_upd(p, g, sq, ema, has_ema, h);
    else nsvd_opt_upd<RULE>(p, g, sq, mom, ema, has_ema, h);
}

// optimiser step fused into the backward: state tensors in the parameters' layouts
struct NsvdOptStep {
    NsvdHyper h;
    nsvd_params sq;          // (pointers null for rules without a square average)
    const nsvd_params* ema;  // null: no EMA
    nsvd_step_state* state;  // device-resident schedule (nsvd.h): h is then read from state->cur on the device
    int emit_planes;         // NSVD_PATH_FUSED_BF16X3 steps: the weight-gradient epilogue also writes the bf16 planes of
                             // the UPDATED hidden-layer weights (pmlp_layer0_bf3.h) into the workspace the next forward reads
    // rules other than RMSprop without momentum (rule != NSVD_RULE_RMSPROP): scalars in oh instead of h, or read from
    // ostate->cur (derived by nsvd_opt_state_begin before the step's first kernel; `state` is then null)
    int rule;
    NsvdOptHyper oh;
    const nsvd_params* mom;  // momentum buffers / Adam's exp_avg (null for rules without them)
    nsvd_opt_state* ostate;
};
