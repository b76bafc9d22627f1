// The optimiser rules of csrc/opt_math.h on the host, in float32, for tests/test_optim_host.py.
#include <string.h>
#include "opt_math.h"

template <int RULE>
static void apply_rule(int n, float* p, const float* g, float* sq, float* mom, float* ema, const NsvdOptHyper& h) {
    for (int i = 0; i < n; ++i) {
        float none_sq = 0.f, none_mom = 0.f, none_ema = 0.f;
        nsvd_opt_upd<RULE>(p[i], g[i], sq ? sq[i] : none_sq, mom ? mom[i] : none_mom, ema ? ema[i] : none_ema,
                           ema != nullptr, h);
    }
}

static int apply(int rule, int n, float* p, const float* g, float* sq, float* mom, float* ema, const NsvdOptHyper& h) {
    switch (rule) {
        case NSVD_RULE_RMSPROP: apply_rule<NSVD_RULE_RMSPROP>(n, p, g, sq, mom, ema, h); return 0;
        case NSVD_RULE_RMSPROP_MOM: apply_rule<NSVD_RULE_RMSPROP_MOM>(n, p, g, sq, mom, ema, h); return 0;
        case NSVD_RULE_SGD: apply_rule<NSVD_RULE_SGD>(n, p, g, sq, mom, ema, h); return 0;
        case NSVD_RULE_SGD_MOM: apply_rule<NSVD_RULE_SGD_MOM>(n, p, g, sq, mom, ema, h); return 0;
        case NSVD_RULE_ADAM: apply_rule<NSVD_RULE_ADAM>(n, p, g, sq, mom, ema, h); return 0;
    }
    return -1;
}

// `steps` scheduled steps over n elements; grads: (steps, n). use_state != 0: the device-resident form - an
// nsvd_opt_state advanced step by step through nsvd_opt_state_derive; else the host form - nsvd_make_opt_hyper from the
// host-scheduled lr[t] / decay[t]. Returns the number of steps taken, or -1 for an unknown kind.
extern "C" int run_rule(const nsvd_opt_config* cfg, double eta_min, unsigned long long T_max, int use_state,
                        const double* lr, const double* decay, double grad_scale, int n, int steps, const float* grads,
                        float* p, float* sq, float* mom, float* ema) {
    const int rule = nsvd_opt_rule(cfg->kind, cfg->momentum);
    if (rule < 0) return -1;
    nsvd_opt_state st;
    memset(&st, 0, sizeof(st));
    st.T_max = T_max;
    st.lr0 = cfg->lr; st.eta_min = eta_min; st.alpha = cfg->alpha; st.eps = cfg->eps; st.ema_decay = cfg->ema_decay;
    st.momentum = cfg->momentum; st.beta1 = cfg->beta1; st.beta2 = cfg->beta2;
    st.kind = cfg->kind;
    for (int t = 0; t < steps; ++t) {
        NsvdOptHyper h;
        if (use_state) {
            nsvd_opt_state_derive(&st);
            h = *nsvd_opt_state_hyper(&st);
            h.b.grad_scale = (float)grad_scale;
        } else {
            h = nsvd_make_opt_hyper(rule, lr[t], cfg->alpha, cfg->eps, cfg->momentum, cfg->beta1, cfg->beta2, decay[t],
                                    grad_scale, (unsigned long long)t);
        }
        if (h.rule != rule) return -1;
        if (apply(rule, n, p, grads + (size_t)t * n, sq, mom, ema, h)) return -1;
        st.step += 1;
    }
    return (int)st.step;
}

// nsvd_rmsprop_upd alone, with the six float32 scalars of NsvdHyper given as they are
extern "C" void run_rmsprop_upd(const float* hyper, int has_ema, int n, int steps, const float* grads, float* p,
                                float* sq, float* ema) {
    NsvdHyper h;
    memcpy(&h, hyper, sizeof(h));
    for (int t = 0; t < steps; ++t)
        for (int i = 0; i < n; ++i) nsvd_rmsprop_upd(p[i], grads[(size_t)t * n + i], sq[i], ema[i], has_ema != 0, h);
}

extern "C" int opt_rule_of(int kind, double momentum) { return nsvd_opt_rule(kind, momentum); }
